"""float_ssim / float_ms_ssim on the MI355X (csrc/ssim_family.hip, PQA_FEAT_FLOAT_SSIM / PQA_FEAT_MS_SSIM): against the
f64 restatement (tests/ssim_family_ref.py), bit-identical across every way frames reach the kernels, and through the
pipeline, the analyzer and a two-rank job."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import ssim_family_ref as R

pytestmark = pytest.mark.gpu
TOL = 1e-5
BITS = 32 | 64   # N.FEAT_FLOAT_SSIM | N.FEAT_MS_SSIM
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _clip(w, h, n, bpc, seed=0):
    """Synthetic natural-looking pairs with sample extremes (0 and full scale blocks in both planes)."""
    from pqa2_amd import synth
    refs, diss = synth.make_clip(w, h, n, bpc, chroma=False)
    top = (1 << bpc) - 1
    rng = np.random.default_rng(seed)
    out_r, out_d = [], []
    for i in range(n):
        r, d = refs[i][0].copy(), diss[i][0].copy()
        for _ in range(4):
            bw, bh = rng.integers(8, max(9, w // 4)), rng.integers(8, max(9, h // 4))
            x, y = rng.integers(0, w - bw), rng.integers(0, h - bh)
            v = top if rng.random() < 0.5 else 0
            r[y:y + bh, x:x + bw] = v
            d[y:y + bh, x:x + bw] = top - v if rng.random() < 0.5 else v
        out_r.append(r); out_d.append(d)
    return out_r, out_d


def _engine_ext(w, h, bpc, refs, diss, features=BITS, **kw):
    from pqa2_amd.engine import FeatureEngine
    with FeatureEngine(w, h, bit_depth=bpc, features=features, **kw) as eng:
        for i in range(len(refs)):
            eng.submit(i, [refs[i]], [diss[i]])
        return eng.collect_ext(0, len(refs))


WORST = {}


@pytest.mark.parametrize("w,h,bpc", [(161, 161, 8), (176, 176, 10), (352, 288, 12), (1039, 913, 8), (1280, 720, 10),
                                     (1920, 1080, 12), (3840, 2160, 8), (161, 400, 10), (352, 288, 8)])
def test_matches_the_restatement(w, h, bpc):
    n = 1 if w * h > 4e6 else 2
    refs, diss = _clip(w, h, n, bpc, seed=w + h + bpc)
    _, ext = _engine_ext(w, h, bpc, refs, diss)
    worst = 0.0
    for i in range(n):
        want = R.ext_record(refs[i], diss[i], bpc)
        d = np.abs(ext[i, :20] - want[:20])
        worst = max(worst, float(np.nanmax(d)))
        assert np.array_equal(np.isnan(ext[i]), np.isnan(want)), (ext[i], want)
        assert np.nanmax(d) <= TOL, f"{w}x{h} {bpc}-bit frame {i}: worst |d| {np.nanmax(d):.3e} at slot {int(np.nanargmax(d))}"
    WORST[(w, h, bpc)] = worst
    print(f"\n{w}x{h} {bpc}-bit: worst |d| vs restatement {worst:.3e} "
          f"(float_ssim {ext[0, 0]:.6f}, float_ms_ssim {ext[0, 4]:.6f})")


def test_negative_scale_mean_gives_nan():
    """Anti-correlated frames: the s means are negative at the fine scales -> float_ms_ssim is NaN (C pow), as defined."""
    w, h = 176, 176
    rng = np.random.default_rng(3)
    r = rng.integers(0, 256, (h, w)).astype(np.uint8)
    d = (255 - r).astype(np.uint8)
    _, ext = _engine_ext(w, h, 8, [r], [d])
    want = R.ext_record(r, d, 8)
    assert np.isnan(want[4]) and np.isnan(ext[0, 4])
    assert np.abs(ext[0, 5:20] - want[5:20]).max() <= TOL
    assert abs(ext[0, 0] - want[0]) <= TOL


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def test_bit_identical_across_batches_submit_paths_and_alignment(tmp_path):
    import torch
    from pqa2_amd import _native as N, synth, yuvio
    from pqa2_amd.engine import FeatureEngine
    w, h, n, bpc = 352, 288, 7, 8
    refs, diss = synth.make_clip(w, h, n, bpc, chroma=True)
    feats = N.FEAT_VMAF | BITS
    base = None
    for mb in (1, 3, 0):
        with FeatureEngine(w, h, n_planes=1, features=feats, max_batch=mb) as eng:
            for i in range(n):
                eng.submit(i, refs[i][:1], diss[i][:1])
            rec, ext = eng.collect_ext(0, n)
        if base is None:
            base = (rec, ext)
        assert np.array_equal(_bits(ext), _bits(base[1])), f"max_batch {mb}"
        assert np.array_equal(_bits(rec), _bits(base[0])), f"max_batch {mb}"
    assert not np.isnan(base[1][:, :20]).any()
    # device-resident planes at odd pitch and base offset
    for off, pad in ((0, 0), (1, 3), (7, 13)):
        pitch = w + pad
        buf = np.full((2, off + n * h * pitch), 0xA5, np.uint8)
        for i in range(n):
            for side, src in enumerate((refs, diss)):
                v = buf[side, off + i * h * pitch: off + (i + 1) * h * pitch].reshape(h, pitch)
                v[:, :w] = src[i][0]
        t = torch.from_numpy(buf).cuda()
        torch.cuda.synchronize()
        with FeatureEngine(w, h, features=feats, max_batch=3) as eng:
            eng.submit_resident(0, n, [t[0].data_ptr() + off], [t[1].data_ptr() + off], [pitch], [h * pitch])
            rec, ext = eng.collect_ext(0, n)
        assert np.array_equal(_bits(ext), _bits(base[1])), f"resident offset {off} pad {pad}"
    # two files through pqa_submit_fd_run (the pipeline's path)
    info = synth.clip_info(w, h, bpc)
    rp, dp = str(tmp_path / "r.y4m"), str(tmp_path / "d.y4m")
    yuvio.write_y4m(rp, refs, info)
    yuvio.write_y4m(dp, diss, info)
    rr, dr = yuvio.open_video(rp), yuvio.open_video(dp)
    with FeatureEngine(w, h, n_planes=3, features=feats | N.FEAT_PSNR | N.FEAT_SSIM) as eng:
        eng.submit_file_run(0, n, rr.fileno(), rr.plane_offsets(0), rr.run_stride(0, n), dr.fileno(), dr.plane_offsets(0),
                            dr.run_stride(0, n))
        rec, ext = eng.collect_ext(0, n)
    assert np.array_equal(_bits(ext), _bits(base[1])), "submit_fd_run"
    # NV12 decoder surfaces (luma scored in place)
    lp = w + 5
    L = np.full((2, n, h, lp), 0x5A, np.uint8)
    for i in range(n):
        L[0, i, :, :w] = refs[i][0]
        L[1, i, :, :w] = diss[i][0]
    tl = torch.from_numpy(L).cuda()
    torch.cuda.synchronize()
    clip = [FeatureEngine.surface_clip(N.SURFACE_NV12, tl[s].data_ptr(), lp, h * lp) for s in (0, 1)]
    with FeatureEngine(w, h, features=feats, max_batch=2) as eng:
        eng.submit_surfaces(0, n, clip[0], clip[1])
        rec, ext = eng.collect_ext(0, n)
    assert np.array_equal(_bits(ext), _bits(base[1])), "submit_surfaces"


@pytest.mark.parametrize("bpc", [8, 10])
def test_default_records_untouched_by_the_new_bits(bpc):
    from pqa2_amd import _native as N, synth
    from pqa2_amd.engine import FeatureEngine
    w, h, n = 352, 288, 5
    refs, diss = synth.make_clip(w, h, n, bpc, chroma=True)
    out = {}
    for tag, f in (("plain", N.FEAT_ALL), ("ext", N.FEAT_ALL | BITS)):
        with FeatureEngine(w, h, bit_depth=bpc, n_planes=3, features=f, max_batch=2) as eng:
            for i in range(n):
                eng.submit(i, refs[i], diss[i])
            out[tag] = eng.collect_ext(0, n)
    assert np.array_equal(_bits(out["plain"][0]), _bits(out["ext"][0]))
    assert np.isnan(out["plain"][1]).all()          # a context without the bits: all-NaN extension rows
    assert not np.isnan(out["ext"][1][:, :20]).any() and np.isnan(out["ext"][1][:, 20:]).all()
    # only the new bits, one at a time: the other feature's slots are NaN
    with FeatureEngine(w, h, bit_depth=bpc, features=N.FEAT_FLOAT_SSIM) as eng:
        for i in range(n):
            eng.submit(i, refs[i][:1], diss[i][:1])
        _, e = eng.collect_ext(0, n)
    assert np.array_equal(_bits(e[:, :4]), _bits(out["ext"][1][:, :4])) and np.isnan(e[:, 4:]).all()
    # pqa_collect is pqa_collect_ext without the extension rows
    with FeatureEngine(w, h, bit_depth=bpc, n_planes=3, features=N.FEAT_ALL | BITS, max_batch=2) as eng:
        for i in range(n):
            eng.submit(i, refs[i], diss[i])
        rec = eng.collect(0, n)
    assert np.array_equal(_bits(rec), _bits(out["plain"][0]))


def test_n_subsample_three():
    w, h, n, bpc = 352, 288, 7, 10
    refs, diss = _clip(w, h, n, bpc, seed=5)
    rec, ext = _engine_ext(w, h, bpc, refs, diss, features=7 | BITS, n_subsample=3, max_batch=4)
    for i in range(n):
        if i % 3:
            assert np.isnan(ext[i]).all(), i
        else:
            want = R.ext_record(refs[i], diss[i], bpc)
            assert np.array_equal(np.isnan(ext[i]), np.isnan(want)), i
            assert np.nanmax(np.abs(ext[i, :20] - want[:20])) <= TOL, i


@pytest.mark.parametrize("w,h,feat,name", [(176, 144, 64, "float_ms_ssim"), (160, 400, 64, "float_ms_ssim"),
                                           (400, 160, 96, "float_ms_ssim")])
def test_too_small_is_einval_naming_the_feature(w, h, feat, name):
    """(float_ssim alone fits every geometry the library accepts: w, h >= 16 leave a decimated plane of >= 11.)"""
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    with pytest.raises(N.PqaError) as ei:
        FeatureEngine(w, h, features=N.FEAT_VMAF | feat)
    assert ei.value.code == N.PQA_EINVAL and name in str(ei.value)
    FeatureEngine(w, h, features=N.FEAT_VMAF).close()      # the same geometry without the bit still works


def test_analyzer_writes_float_ms_ssim_per_frame(tmp_path):
    import json
    from pqa2_amd import yuvio
    from pqa2_amd.vmaf_analyzer import VMAFAnalyzer
    rp = os.path.join(ROOT, "tests", "golden", "clips", "c352x288_8_ref.y4m")
    dp = os.path.join(ROOT, "tests", "golden", "clips", "c352x288_8_dist.y4m")
    a = VMAFAnalyzer()
    a.set_output_directory(str(tmp_path))
    a.set_test_name("ssf")
    a.set_advanced_options(ms_ssim_enabled=True, float_ssim_enabled=True)
    errors = []
    a.error_occurred.connect(errors.append)
    res = a.analyze_videos(rp, dp, "vmaf_v0.6.1")
    assert errors == [] and res is not None
    log = json.load(open(res["json_path"]))
    rr, dr = yuvio.open_video(rp), yuvio.open_video(dp)
    ms, fs = [], []
    for i, fr in enumerate(log["frames"]):
        want = R.ext_record(rr.frame(i)[0], dr.frame(i)[0], 8)
        got = fr["metrics"]["float_ms_ssim"]   # %.6f in the log: equal to the restatement's, short of a rounding tie
        assert got == float(f"{want[4]:.6f}") or abs(got - want[4]) <= 5e-7 + 1e-9, (got, want[4])
        assert abs(fr["metrics"]["float_ssim"] - want[0]) <= 1.5e-6
        ms.append(want[4]); fs.append(want[0])
    assert abs(res["float_ms_ssim"] - np.mean(ms)) <= 2e-6 and abs(res["float_ssim"] - np.mean(fs)) <= 2e-6


def test_two_ranks_give_the_single_process_extension_records(tmp_path):
    """2-rank gloo job on one GPU (torchrun + pqa2_amd.score --ms-ssim --float-ssim): the JSON, extension columns included,
    equals the single-process run (wall-clock fps aside)."""
    import json
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
        cmd = [sys.executable] + launcher + ["-m", "pqa2_amd.score", rp, dp, "--json", j, "--batch", "2", "--ms-ssim",
                                            "--float-ssim"]
        if launcher:
            cmd += ["--backend", "gloo", "--share-device"]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        d = json.load(open(j))
        d.pop("fps", None)
        outs[tag] = d
    assert outs["one"] == outs["two"]
    assert "float_ms_ssim" in outs["one"]["pooled_metrics"] and "float_ssim" in outs["one"]["frames"][5]["metrics"]
