"""psnr_hvs on the MI355X (csrc/psnr_hvs.hip, PQA_FEAT_PSNR_HVS): per-block error sums of the real kernel against the f64
restatement (tests/psnr_hvs_ref.py), the full path over geometries, bit depths, chroma formats and contents, bit-identical
ext2 rows across every way frames reach the kernel, and no effect on the other outputs."""
import ctypes as C

import numpy as np
import pytest

from tests import psnr_hvs_ref as R

pytestmark = pytest.mark.gpu
DB_ABS, MSE_REL = 1e-4, 1e-5          # full path vs the f64 restatement
BLOCK_REL, BLOCK_ABS = 2e-5, 1e-3     # per-block sums (f32 per block) vs f64
KEYS = ("psnr_hvs_y", "psnr_hvs_cb", "psnr_hvs_cr", "psnr_hvs")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _plane_pair(w, h, bpc, seed):
    """Textured plane with flat patches and sample extremes, and a distorted copy (noise, a shift, a flat offset)."""
    rng = np.random.default_rng(seed)
    top = (1 << bpc) - 1
    yy, xx = np.mgrid[0:h, 0:w]
    r = (0.5 + 0.35 * np.sin(xx * 0.09 + seed) * np.cos(yy * 0.06)) * top + rng.normal(0, top * 0.03, (h, w))
    r[h // 3: h // 3 + 9, :] = top * 0.25                       # flat stripe: g = 0 blocks
    r[:, w // 2: w // 2 + 3] = top                              # full-scale column
    d = r + rng.normal(0, top * 0.01, (h, w))
    d[: h // 4] = np.roll(d[: h // 4], 1, axis=1)
    d[h // 3: h // 3 + 9, :] += top * 0.01
    d[-5:, :] = r[-5:, :]                                       # identical rows: zero-error blocks at the bottom
    dt = np.uint8 if bpc == 8 else np.uint16
    return (np.clip(np.rint(r), 0, top).astype(dt), np.clip(np.rint(d), 0, top).astype(dt))


def _hook(ref, dis, bpc, kind, pad=0):
    from pqa2_amd import _native as N
    lib = N.load()
    h, w = ref.shape
    es = ref.itemsize
    rp = np.zeros((h, w + pad), ref.dtype)
    dp = np.zeros((h, w + pad), ref.dtype)
    rp[:, :w], dp[:, :w] = ref, dis
    nbx, nby = R.n_blocks(w, h)
    err = np.full(nbx * nby, -1.0, np.float32)
    mse = C.c_double()
    rc = lib.pqa_debug_psnr_hvs_plane(rp.ctypes.data, dp.ctypes.data, (w + pad) * es, w, h, bpc, kind, err.ctypes.data,
                                      C.byref(mse))
    assert rc == N.PQA_OK, lib.pqa_last_error(None)
    return err.reshape(nby, nbx), mse.value


# 232 = 33 blocks: one past a 32-block workgroup; 2160p rows straddle the 4-row workgroups; odd sizes leave remainders
@pytest.mark.parametrize("w,h,bpc,kind", [(8, 8, 8, 0), (232, 36, 8, 0), (232, 36, 10, 1), (233, 57, 12, 2),
                                          (1039, 913, 8, 1), (1039, 913, 12, 0), (3840, 2160, 8, 0), (1920, 1080, 10, 2)])
def test_block_sums_match_the_restatement(w, h, bpc, kind):
    ref, dis = _plane_pair(w, h, bpc, seed=w + h + bpc + kind)
    got, mse = _hook(ref, dis, bpc, kind, pad=3)
    want = R.block_errors(ref, dis, kind)
    assert (got >= 0).all(), "a block was not written"
    assert np.array_equal(got == 0, want == 0), "zero / non-zero pattern differs"
    rel = np.abs(got - want) / np.maximum(want, 1.0)
    print(f"\n{w}x{h} {bpc}-bit kind {kind}: {got.size} blocks, {int((want == 0).sum())} zero, worst rel {rel.max():.2e}")
    assert np.allclose(got, want, rtol=BLOCK_REL, atol=BLOCK_ABS)
    want_mse = R.plane_mse(ref, dis, kind)
    assert abs(mse - want_mse) <= MSE_REL * want_mse


def _frames(w, h, bpc, hs, vs, n, seed):
    cw, ch = (w + (1 << hs) - 1) >> hs, (h + (1 << vs) - 1) >> vs
    out = []
    for i in range(n):
        pl = [_plane_pair(pw, ph, bpc, seed + 13 * i + p) for p, (pw, ph) in enumerate(((w, h), (cw, ch), (cw, ch)))]
        out.append(([p[0] for p in pl], [p[1] for p in pl]))
    return [f[0] for f in out], [f[1] for f in out]


def _run(w, h, bpc, hs, vs, refs, diss, features=None, **kw):
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    feats = N.FEAT_PSNR_HVS if features is None else features
    with FeatureEngine(w, h, bit_depth=bpc, n_planes=3, chroma_shift=(hs, vs), features=feats, **kw) as eng:
        for i in range(len(refs)):
            eng.submit(i, refs[i], diss[i])
        return eng.collect_ext2(0, len(refs))


def _check(row, ref, dis, bpc, tag):
    want = R.psnr_hvs(ref, dis, bpc)
    for k, key in enumerate(KEYS):
        assert np.isfinite(row[k]) and row[k] > 0, (tag, key, row[k])
        assert abs(row[k] - want[key]) <= DB_ABS, (tag, key, row[k], want[key])
    for p in range(3):
        assert abs(row[4 + p] - want["mse"][p]) <= MSE_REL * want["mse"][p], (tag, p, row[4 + p], want["mse"][p])
    assert np.isnan(row[7])
    return want


CASES = [(16, 16, 8, 1, 1), (64, 48, 10, 1, 0), (161, 161, 12, 0, 0), (352, 288, 8, 1, 1), (1039, 913, 10, 1, 1),
         (1039, 913, 12, 1, 0), (1280, 720, 8, 0, 0), (1920, 1080, 12, 1, 1), (3840, 2160, 8, 1, 1), (3840, 2160, 10, 1, 1)]
# the mixed layouts (the two chroma shifts differ), at sizes that leave partial blocks in every plane
CASES += [(w, h, bpc, hs, vs) for (hs, vs) in [(2, 0), (0, 2), (1, 2), (2, 1), (0, 1)] for (w, h) in [(37, 41), (233, 57)]
          for bpc in (8, 12)]


@pytest.mark.parametrize("w,h,bpc,hs,vs", CASES)
def test_full_path_matches_the_restatement(w, h, bpc, hs, vs):
    n = 1 if w * h > 2e6 else 2
    refs, diss = _frames(w, h, bpc, hs, vs, n, seed=w + bpc + hs + vs)
    _, ext, ext2 = _run(w, h, bpc, hs, vs, refs, diss)
    assert np.isnan(ext).all()
    for i in range(n):
        want = _check(ext2[i], refs[i], diss[i], bpc, (w, h, bpc, hs, vs, i))
        print(f"\n{w}x{h} {bpc}-bit ({hs},{vs}) frame {i}: psnr_hvs {want['psnr_hvs']:.5f} dB, "
              f"|d| {abs(ext2[i, 3] - want['psnr_hvs']):.2e}")


@pytest.mark.parametrize("w,h,bpc", [(352, 288, 8), (1920, 1080, 8), (3840, 2160, 8), (1280, 720, 10)])
def test_natural_content(w, h, bpc):
    from pqa2_amd import synth
    refs, diss = synth.make_clip(w, h, 2 if w * h < 2e6 else 1, bpc, chroma=True)
    _, _, ext2 = _run(w, h, bpc, 1, 1, refs, diss)
    for i in range(len(refs)):
        _check(ext2[i], refs[i], diss[i], bpc, (w, h, bpc, i))


def test_identical_frames_give_inf():
    w, h, bpc = 352, 288, 10
    refs, _ = _frames(w, h, bpc, 1, 1, 2, seed=3)
    _, _, ext2 = _run(w, h, bpc, 1, 1, refs, refs)
    assert np.isposinf(ext2[:, :4]).all() and (ext2[:, 4:7] == 0).all()


@pytest.mark.parametrize("hs,vs", [(2, 0), (0, 2), (2, 2), (1, 2), (2, 1)])
def test_16x16_with_a_shift_of_two_is_rejected(hs, vs):
    from pqa2_amd import _native as N
    refs, diss = _frames(16, 16, 8, hs, vs, 1, seed=1)
    with pytest.raises(N.PqaError, match="psnr_hvs needs every plane >= 8x8") as e:
        _run(16, 16, 8, hs, vs, refs, diss)
    assert e.value.code == N.PQA_EINVAL


@pytest.mark.parametrize("bpc", [8, 10])
def test_bit_identical_across_batches_submit_paths_and_alignment(bpc):
    import torch
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    w, h, n = 352, 288, 7
    refs, diss = _frames(w, h, bpc, 1, 1, n, seed=40)
    feats = N.FEAT_VMAF | N.FEAT_PSNR_HVS
    base = None
    for mb in (1, 3, 0):
        _, _, ext2 = _run(w, h, bpc, 1, 1, refs, diss, features=feats, max_batch=mb)
        if base is None:
            base = ext2
        assert np.array_equal(_bits(ext2), _bits(base)), f"max_batch {mb}"
    assert np.isfinite(base[:, :7]).all()
    es = 1 if bpc == 8 else 2
    dt = np.uint8 if bpc == 8 else np.uint16
    sizes = [(w, h), (w // 2, h // 2), (w // 2, h // 2)]
    for off, pad in ((0, 0), (1, 3), (7, 13)):      # device-resident planes at odd pitches and base offsets (elements)
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
            ext2 = eng.collect_ext2(0, n)[2]
        assert np.array_equal(_bits(ext2), _bits(base)), f"resident offset {off} pad {pad}"
    # decoder surfaces: NV12 (8-bit) / P010 (10-bit), chroma interleaved, 16-bit samples in the high bits
    lp, cp = w + 5, w + 9
    sdt = np.uint8 if bpc == 8 else np.uint16
    shift = 0 if bpc == 8 else 16 - bpc
    L = np.zeros((2, n, h, lp), sdt)
    CH = np.zeros((2, n, h // 2, cp), sdt)
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
        ext2 = eng.collect_ext2(0, n)[2]
    assert np.array_equal(_bits(ext2), _bits(base)), "submit_surfaces"


def test_n_subsample_three():
    from pqa2_amd import _native as N
    w, h, n, bpc = 352, 288, 7, 10
    refs, diss = _frames(w, h, bpc, 1, 1, n, seed=80)
    _, _, base = _run(w, h, bpc, 1, 1, refs, diss, features=N.FEAT_VMAF | N.FEAT_PSNR_HVS)
    for mb in (4, 0):
        _, _, ext2 = _run(w, h, bpc, 1, 1, refs, diss, features=N.FEAT_VMAF | N.FEAT_PSNR_HVS, n_subsample=3, max_batch=mb)
        for i in range(n):
            if i % 3:
                assert np.isnan(ext2[i]).all(), (mb, i)
            else:
                assert np.array_equal(_bits(ext2[i]), _bits(base[i])), (mb, i)


@pytest.mark.parametrize("bpc", [8, 10])
def test_no_effect_on_the_other_outputs(bpc):
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    w, h, n = 352, 288, 5
    refs, diss = _frames(w, h, bpc, 1, 1, n, seed=60)
    others = N.FEAT_ALL | N.FEAT_FLOAT_SSIM | N.FEAT_MS_SSIM | N.FEAT_CIEDE | N.FEAT_CAMBI
    plain = _run(w, h, bpc, 1, 1, refs, diss, features=others, max_batch=2)
    both = _run(w, h, bpc, 1, 1, refs, diss, features=others | N.FEAT_PSNR_HVS, max_batch=2)
    assert np.array_equal(_bits(plain[0]), _bits(both[0]))          # the 24-double records
    assert np.array_equal(_bits(plain[1]), _bits(both[1]))          # every slot of the first extension record
    assert np.isnan(plain[2]).all()                                 # without the bit: no ring, NaN rows
    assert np.isfinite(both[2][:, :7]).all()
    # the older collect entry points give the same bytes as before on a context with the bit
    with FeatureEngine(w, h, bit_depth=bpc, n_planes=3, features=others | N.FEAT_PSNR_HVS, max_batch=2) as eng:
        for i in range(n):
            eng.submit(i, refs[i], diss[i])
        rec, ext = eng.collect_ext(0, n)
    assert np.array_equal(_bits(rec), _bits(plain[0])) and np.array_equal(_bits(ext), _bits(plain[1]))
    with FeatureEngine(w, h, bit_depth=bpc, n_planes=3, features=N.FEAT_ALL, max_batch=2) as eng:
        for i in range(n):
            eng.submit(i, refs[i], diss[i])
        rec = eng.collect(0, n)
    assert np.array_equal(_bits(rec), _bits(plain[0]))


def test_pipeline_and_score_cli(tmp_path):
    import json
    import os
    import subprocess
    import sys
    from pqa2_amd import yuvio
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rp = os.path.join(root, "tests", "golden", "clips", "c352x288_8_ref.y4m")
    dp = os.path.join(root, "tests", "golden", "clips", "c352x288_8_dist.y4m")
    j = str(tmp_path / "o.json")
    env = dict(os.environ, PYTHONPATH=root)
    r = subprocess.run([sys.executable, "-m", "pqa2_amd.score", rp, dp, "--json", j, "--psnr-hvs"], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    log = json.load(open(j))
    rr, dr = yuvio.open_video(rp), yuvio.open_video(dp)
    for i, fr in enumerate(log["frames"]):
        want = R.psnr_hvs(rr.frame(i), dr.frame(i), 8)
        for k in KEYS:
            assert abs(fr["metrics"][k] - want[k]) <= DB_ABS + 5e-7, (i, k)
    for k in KEYS:
        assert k in log["pooled_metrics"]
