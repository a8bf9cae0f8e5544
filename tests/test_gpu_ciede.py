"""ciede2000 on the MI355X (csrc/ciede.hip, PQA_FEAT_CIEDE): the kernel's CIEDE2000 device function against Sharma et al.'s
pairs and the f64 restatement (tests/ciede_ref.py), the full path against the restatement over geometries, bit depths and
chroma formats, bit-identical results across every way frames reach the kernel, no effect on the other outputs, and the
pipeline / analyzer / two-rank paths."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import ciede_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN_REL, SCORE_ABS = 2e-5, 2e-4      # full path vs the f64 restatement
PAIR_TOL = 2e-5                       # debug hook vs the f64 restatement: absolute + relative


def _debug(pairs):
    from pqa2_amd import _native as N
    lib = N.load()
    lab = np.ascontiguousarray(pairs, np.float64).reshape(-1, 6)
    out = np.zeros(lab.shape[0])
    assert lib.pqa_debug_ciede2000(lab.ctypes.data, lab.shape[0], out.ctypes.data) == N.PQA_OK
    return out


def test_debug_hook_matches_the_sharma_pairs():
    d = np.loadtxt(os.path.join(ROOT, "tests", "golden", "ciede2000_sharma.csv"), delimiter=",", comments="#")
    got = _debug(d[:, :6])
    near = R.hue_delta_from_180(*d[:, :6].T) <= 1e-3
    for i in range(len(d)):
        if near[i]:   # at the 180-degree hue jump: either published value of the pair's group
            group = {7.1792, 7.2195} if d[i, 6] in (7.1792, 7.2195) else {4.8045, 4.7461}
            assert min(abs(got[i] - v) for v in group) <= 1e-4, (i, got[i])
        else:
            assert abs(got[i] - d[i, 6]) <= 1e-4, (i, got[i], d[i, 6])


def test_debug_hook_random_pairs_against_f64():
    rng = np.random.default_rng(11)
    n = 100_000
    L = rng.uniform(0, 100, (n, 2))
    ab = rng.uniform(-128, 128, (n, 4))
    # a quarter of the pairs close together (small differences: the cancellation-prone region), some achromatic ones
    close = rng.random(n) < 0.25
    L[close, 1] = L[close, 0] + rng.normal(0, 0.5, close.sum())
    ab[close, 2:] = ab[close, :2] + rng.normal(0, 0.5, (close.sum(), 2))
    ab[rng.random(n) < 0.01, :2] = 0.0
    pairs = np.column_stack([L[:, 0], ab[:, 0], ab[:, 1], L[:, 1], ab[:, 2], ab[:, 3]])
    f32 = pairs.astype(np.float32).astype(np.float64)       # the hook's inputs are f32
    want = R.de00(*f32.T)
    got = _debug(pairs)
    keep = R.hue_delta_from_180(*f32.T) > 1e-3
    err = np.abs(got - want) / (1.0 + np.abs(want))
    i = int(np.argmax(np.where(keep, err, 0)))
    print(f"\nworst |d| / (1 + dE) over {keep.sum()} pairs: {err[i]:.3e} (dE {want[i]:.5f}, pair {f32[i]})")
    assert err[keep].max() <= PAIR_TOL
    assert np.isfinite(got).all()


# ---- the full path ----------------------------------------------------------------------------------------------
def _planes(w, h, bpc, hs, vs, seed):
    """Synthetic {ref, dis} frames: smooth colour fields with texture, distorted by a chroma shift / gain, luma noise and
    blocks of sample extremes (0 / full scale in every plane)."""
    rng = np.random.default_rng(seed)
    top = (1 << bpc) - 1
    s = 1 << (bpc - 8)
    cw, ch = (w + (1 << hs) - 1) >> hs, (h + (1 << vs) - 1) >> vs
    dt = np.uint8 if bpc == 8 else np.uint16

    def field(pw, ph, base, amp):
        yy, xx = np.mgrid[0:ph, 0:pw]
        f = base + amp * np.sin(xx * 0.05 + rng.uniform(0, 6)) * np.cos(yy * 0.04 + rng.uniform(0, 6))
        return f + rng.normal(0, amp * 0.1, (ph, pw))

    ry, ru, rv = field(w, h, 120, 70), field(cw, ch, 128, 60), field(cw, ch, 128, 60)
    dy = ry + rng.normal(0, 3, ry.shape)
    du = 128 + (ru - 128) * 0.8 + 6
    dv = np.roll(rv, 2, axis=1) - 4
    planes = [[ry, ru, rv], [dy, du, dv]]
    out = [[np.clip(np.rint(p * s), 0, top).astype(dt) for p in fr] for fr in planes]
    for _ in range(3):
        bw, bh = int(rng.integers(4, max(5, cw // 3))), int(rng.integers(4, max(5, ch // 3)))
        x, y = int(rng.integers(0, cw - bw + 1)), int(rng.integers(0, ch - bh + 1))
        for side in (0, 1):
            for p in range(3):
                v = top if rng.random() < 0.5 else 0
                if p == 0:
                    out[side][0][y << vs:(y + bh) << vs, x << hs:(x + bw) << hs] = v
                else:
                    out[side][p][y:y + bh, x:x + bw] = v
    return out[0], out[1]


def _run(w, h, bpc, hs, vs, refs, diss, features=256, **kw):
    from pqa2_amd.engine import FeatureEngine
    with FeatureEngine(w, h, bit_depth=bpc, n_planes=3, chroma_shift=(hs, vs), features=features, **kw) as eng:
        for i in range(len(refs)):
            eng.submit(i, refs[i], diss[i])
        return eng.collect_ext(0, len(refs))


CASES = [(64, 48, 8, 1, 1), (161, 161, 10, 1, 0), (161, 161, 12, 0, 0), (352, 288, 12, 1, 1), (352, 288, 8, 1, 0),
         (1039, 913, 8, 1, 1), (1039, 913, 10, 0, 0), (1280, 720, 10, 1, 1), (1920, 1080, 12, 1, 1), (1920, 1080, 8, 1, 0),
         (3840, 2160, 8, 1, 1), (3840, 2160, 10, 1, 1)]
# the six layouts beside 4:4:4 / 4:2:2 / 4:2:0 (rolled pixel loops, `break` at the picture edge), at two odd sizes
CASES += [(w, h, bpc, hs, vs) for (hs, vs) in [(2, 2), (2, 1), (2, 0), (1, 2), (0, 1), (0, 2)]
          for (w, h) in [(161, 161), (1039, 913)] for bpc in ((8, 10, 12) if (hs, vs) in [(2, 2), (0, 1)] else (8, 10))]


@pytest.mark.parametrize("w,h,bpc,hs,vs", CASES)
def test_full_path_matches_the_restatement(w, h, bpc, hs, vs):
    n = 1 if w * h > 2e6 else 2
    frames = [_planes(w, h, bpc, hs, vs, seed=w + h + bpc + 7 * i + hs) for i in range(n)]
    refs, diss = [f[0] for f in frames], [f[1] for f in frames]
    _, ext = _run(w, h, bpc, hs, vs, refs, diss)
    for i in range(n):
        score, mean = R.frame_slots(refs[i], diss[i], bpc, hs, vs)
        s32, m32 = R.frame_slots(refs[i], diss[i], bpc, hs, vs, dtype=np.float32)
        rel = abs(ext[i, 21] - mean) / mean
        print(f"\n{w}x{h} {bpc}-bit shift ({hs},{vs}) frame {i}: mean dE {mean:.6f}, GPU rel {rel:.2e} "
              f"(numpy f32 rel {abs(m32 - mean) / mean:.2e}), score |d| {abs(ext[i, 20] - score):.2e}")
        assert rel <= MEAN_REL
        assert abs(ext[i, 20] - score) <= SCORE_ABS
        assert np.isnan(ext[i, :20]).all() and np.isnan(ext[i, 22:]).all()


def test_identical_frames_give_zero_and_inf():
    w, h, bpc = 352, 288, 10
    r, _ = _planes(w, h, bpc, 1, 1, seed=3)
    _, ext = _run(w, h, bpc, 1, 1, [r, r], [r, r])
    assert (ext[:, 21] == 0.0).all() and np.isposinf(ext[:, 20]).all()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("bpc", [8, 10])
def test_bit_identical_across_batches_submit_paths_and_alignment(bpc):
    import torch
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    w, h, n = 352, 288, 7
    frames = [_planes(w, h, bpc, 1, 1, seed=40 + i) for i in range(n)]
    refs, diss = [f[0] for f in frames], [f[1] for f in frames]
    feats = N.FEAT_VMAF | N.FEAT_CIEDE
    base = None
    for mb in (1, 3, 0):
        rec, ext = _run(w, h, bpc, 1, 1, refs, diss, features=feats, max_batch=mb)
        if base is None:
            base = ext
        assert np.array_equal(_bits(ext[:, 20:22]), _bits(base[:, 20:22])), f"max_batch {mb}"
    assert not np.isnan(base[:, 20:22]).any()
    es = 1 if bpc == 8 else 2
    dt = np.uint8 if bpc == 8 else np.uint16
    sizes = [(w, h), (w // 2, h // 2), (w // 2, h // 2)]
    # device-resident planes at odd pitches and base offsets (in elements)
    for off, pad in ((0, 0), (1, 3), (7, 13)):
        ptrs, keep, rps, fps = ([], []), [], [], []
        for p, (pw, ph) in enumerate(sizes):
            pitch = pw + pad + p
            rps.append(pitch * es)
            fps.append(ph * pitch * es)
            for side, src in enumerate((refs, diss)):
                buf = np.full(off + n * ph * pitch, 0xA5, dt)
                for i in range(n):
                    buf[off + i * ph * pitch: off + (i + 1) * ph * pitch].reshape(ph, pitch)[:, :pw] = src[i][p]
                t = torch.from_numpy(buf.view(np.uint8)).cuda()
                keep.append(t)
                ptrs[side].append(t.data_ptr() + off * es)
        torch.cuda.synchronize()
        with FeatureEngine(w, h, bit_depth=bpc, n_planes=3, features=feats, max_batch=3) as eng:
            eng.submit_resident(0, n, ptrs[0], ptrs[1], rps, fps)
            _, ext = eng.collect_ext(0, n)
        assert np.array_equal(_bits(ext[:, 20:22]), _bits(base[:, 20:22])), f"resident offset {off} pad {pad}"
    # decoder surfaces: NV12 (8-bit) / P010 (10-bit), chroma interleaved, 16-bit samples in the high bits
    lp = w + 5
    cp = w + 9            # bytes per chroma row are at least w * es; pad in samples
    sdt = np.uint8 if bpc == 8 else np.uint16
    shift = 0 if bpc == 8 else 16 - bpc
    L = np.full((2, n, h, lp), 0, sdt)
    CH = np.full((2, n, h // 2, cp), 0, sdt)
    for i in range(n):
        for side, src in enumerate((refs, diss)):
            L[side, i, :, :w] = src[i][0].astype(sdt) << shift
            CH[side, i, :, 0:w:2] = src[i][1].astype(sdt) << shift
            CH[side, i, :, 1:w:2] = src[i][2].astype(sdt) << shift
    tl, tc = torch.from_numpy(L.view(np.uint8)).cuda(), torch.from_numpy(CH.view(np.uint8)).cuda()
    torch.cuda.synchronize()
    fmt = N.SURFACE_NV12 if bpc == 8 else N.SURFACE_P01X
    lpb, cpb = lp * es, cp * es
    clip = [FeatureEngine.surface_clip(fmt, tl[s].data_ptr(), lpb, h * lpb, tc[s].data_ptr(), cpb, (h // 2) * cpb)
            for s in (0, 1)]
    with FeatureEngine(w, h, bit_depth=bpc, n_planes=3, features=feats, max_batch=2) as eng:
        eng.submit_surfaces(0, n, clip[0], clip[1])
        _, ext = eng.collect_ext(0, n)
    assert np.array_equal(_bits(ext[:, 20:22]), _bits(base[:, 20:22])), "submit_surfaces"


@pytest.mark.parametrize("bpc", [8, 10])
def test_no_effect_on_the_other_outputs(bpc):
    from pqa2_amd import _native as N
    w, h, n = 352, 288, 5
    frames = [_planes(w, h, bpc, 1, 1, seed=60 + i) for i in range(n)]
    refs, diss = [f[0] for f in frames], [f[1] for f in frames]
    ssf = N.FEAT_FLOAT_SSIM | N.FEAT_MS_SSIM
    plain = _run(w, h, bpc, 1, 1, refs, diss, features=N.FEAT_ALL | ssf, max_batch=2)
    both = _run(w, h, bpc, 1, 1, refs, diss, features=N.FEAT_ALL | ssf | N.FEAT_CIEDE, max_batch=2)
    only = _run(w, h, bpc, 1, 1, refs, diss, features=N.FEAT_CIEDE, max_batch=2)
    assert np.array_equal(_bits(plain[0]), _bits(both[0]))                    # the 24-double records
    assert np.array_equal(_bits(plain[1][:, :20]), _bits(both[1][:, :20]))    # the SSIM-family slots
    assert np.isnan(plain[1][:, 20:]).all()                                   # without the bit: NaN in 20..23
    assert not np.isnan(both[1][:, 20:22]).any() and np.isnan(both[1][:, 22:]).all()
    assert np.array_equal(_bits(only[1][:, 20:22]), _bits(both[1][:, 20:22]))  # CIEDE slots survive the SSIM epilogue
    assert np.isnan(only[1][:, :20]).all() and np.isnan(only[1][:, 22:]).all()


def test_n_subsample_three():
    w, h, n, bpc = 352, 288, 7, 10
    frames = [_planes(w, h, bpc, 1, 1, seed=80 + i) for i in range(n)]
    refs, diss = [f[0] for f in frames], [f[1] for f in frames]
    _, ext = _run(w, h, bpc, 1, 1, refs, diss, features=7 | 256, n_subsample=3, max_batch=4)
    for i in range(n):
        if i % 3:
            assert np.isnan(ext[i]).all(), i
        else:
            score, mean = R.frame_slots(refs[i], diss[i], bpc)
            assert abs(ext[i, 21] - mean) / mean <= MEAN_REL and abs(ext[i, 20] - score) <= SCORE_ABS, i


def test_analyzer_writes_ciede2000_per_frame_and_pooled(tmp_path):
    from pqa2_amd import yuvio
    from pqa2_amd.vmaf_analyzer import VMAFAnalyzer
    rp = os.path.join(ROOT, "tests", "golden", "clips", "c352x288_8_ref.y4m")
    dp = os.path.join(ROOT, "tests", "golden", "clips", "c352x288_8_dist.y4m")
    a = VMAFAnalyzer()
    a.set_output_directory(str(tmp_path))
    a.set_test_name("ciede")
    a.set_advanced_options(ciede_enabled=True)
    errors = []
    a.error_occurred.connect(errors.append)
    res = a.analyze_videos(rp, dp, "vmaf_v0.6.1")
    assert errors == [] and res is not None
    log = json.load(open(res["json_path"]))
    rr, dr = yuvio.open_video(rp), yuvio.open_video(dp)
    want = []
    for i, fr in enumerate(log["frames"]):
        s = R.frame_slots(rr.frame(i), dr.frame(i), 8)[0]
        assert abs(fr["metrics"]["ciede2000"] - s) <= SCORE_ABS + 5e-7, (i, fr["metrics"]["ciede2000"], s)
        want.append(s)
    assert "ciede2000" in log["pooled_metrics"]
    assert abs(res["ciede2000"] - np.mean(want)) <= SCORE_ABS + 1e-6


def test_two_ranks_give_the_single_process_ciede2000(tmp_path):
    """2-rank gloo job on one GPU (torchrun + pqa2_amd.score --ciede): the JSON equals the single-process run."""
    import socket
    from pqa2_amd import synth, yuvio
    w, h, n = 320, 180, 11
    refs, diss = synth.make_clip(w, h, n, 8, chroma=True)
    info = synth.clip_info(w, h, 8)
    rp, dp = str(tmp_path / "r.y4m"), str(tmp_path / "d.y4m")
    yuvio.write_y4m(rp, refs, info)
    yuvio.write_y4m(dp, diss, info)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, PYTHONPATH=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0")
    outs = {}
    for tag, launcher in (("one", []), ("two", ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                                                 "--master-addr", "127.0.0.1", "--master-port", str(port)])):
        j = str(tmp_path / f"{tag}.json")
        cmd = [sys.executable] + launcher + ["-m", "pqa2_amd.score", rp, dp, "--json", j, "--batch", "2", "--ciede"]
        if launcher:
            cmd += ["--backend", "gloo", "--share-device"]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        d = json.load(open(j))
        d.pop("fps", None)
        outs[tag] = d
    assert outs["one"] == outs["two"]
    assert "ciede2000" in outs["one"]["pooled_metrics"] and "ciede2000" in outs["one"]["frames"][5]["metrics"]
