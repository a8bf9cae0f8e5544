"""Temporal alignment on the MI355X (csrc/cross_sse.hip, pqa_cross_sse / pqa_cross_sse_device): the banded cross-frame SSE
equals the numpy restatement (tests/align_ref.py) as integers -- smallest call, row tails / pitches / odd base addresses,
the 32-frame tile edge, frames above the i32 accumulator limit at the sample extremes, 10 and 12 bit; the MFMA and the
VALU path agree (child process with PQA_XSSE_MFMA=0); the calls leave the scoring chain alone; and a mistimed Y4M pair
through score_files(align=) and VMAFAnalyzer.  The clips are random and asymmetric (reference and capture differ, frames
differ), so a transposed C tile or swapped operands cannot pass."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import align_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _engine(w, h, bpc=8, **kw):
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    return FeatureEngine(w, h, bit_depth=bpc, n_planes=1, features=kw.pop("features", N.FEAT_PSNR), **kw)


def _padded(frames, pad=5, lead=1):
    """the same frames as views into one buffer: rows `pad` samples apart more than a row, base `lead` samples in"""
    h, w = frames[0].shape
    buf = np.zeros((len(frames), h, w + pad), frames[0].dtype)
    buf[:, :, lead:lead + w] = np.stack(frames)
    return buf, [buf[i, :, lead:lead + w] for i in range(len(frames))]


def _resident(eng, ref_buf, dis_buf, lead, n_ref, n_dis, k_lo, k_hi):
    import torch
    es = ref_buf.dtype.itemsize
    tr = torch.from_numpy(ref_buf.view(np.uint8).reshape(-1)).cuda()
    td = torch.from_numpy(dis_buf.view(np.uint8).reshape(-1)).cuda()
    torch.cuda.synchronize()
    rp, fp = ref_buf.strides[1], ref_buf.strides[0]
    return eng.cross_sse_resident(tr.data_ptr() + lead * es, rp, fp, n_ref, td.data_ptr() + lead * es, dis_buf.strides[1],
                                  dis_buf.strides[0], n_dis, k_lo, k_hi)


def test_smallest_call():
    ref, dis, (k_lo, k_hi) = R.gpu_clip("smallest")
    with _engine(16, 16) as eng:
        got = eng.cross_sse(ref, dis, k_lo, k_hi)
        assert got.dtype == np.uint64 and np.array_equal(got, R.cross_sse(ref, dis, k_lo, k_hi))
        assert eng.cross_sse([], dis, k_lo, k_hi).shape == (0, 3)
        assert np.array_equal(eng.cross_sse(ref, dis, 1, 1), R.cross_sse(ref, dis, 1, 1))


@pytest.mark.parametrize("name", ["tails", "depth10", "depth12"])
def test_tails_pitches_and_depths(name):
    """50 x 18: a row is no multiple of the 16-sample lane run; rows padded by 5 samples, base one sample in; the
    device-resident and the host entry agree"""
    ref, dis, (k_lo, k_hi) = R.gpu_clip(name)
    bpc = R.GPU_CLIPS[name][0]["bpc"]
    assert (len(ref), len(dis)) == ((5, 7) if name == "tails" else (5, len(dis)))
    want = R.cross_sse(ref, dis, k_lo, k_hi)
    rbuf, rv = _padded(ref)
    dbuf, dv = _padded(dis)
    with _engine(50, 18, bpc) as eng:
        assert np.array_equal(eng.cross_sse(ref, dis, k_lo, k_hi), want)
        assert np.array_equal(eng.cross_sse(rv, dv, k_lo, k_hi), want)
        assert np.array_equal(_resident(eng, rbuf, dbuf, 1, len(ref), len(dis), k_lo, k_hi), want)
        abuf, _ = _padded(ref, pad=14, lead=0)    # 64-byte rows at 8 bit: the aligned loads, with a row tail
        bbuf, _ = _padded(dis, pad=14, lead=0)
        assert np.array_equal(_resident(eng, abuf, bbuf, 0, len(ref), len(dis), k_lo, k_hi), want)


def test_tile_edge():
    """40 reference and 45 captured frames, band -9 ... 9: the band crosses the 32-frame tile boundary on both clips and
    the last tile is partial"""
    ref, dis, (k_lo, k_hi) = R.gpu_clip("tile_edge")
    assert (len(ref), len(dis)) == (40, 45)
    want = R.cross_sse(ref, dis, k_lo, k_hi)
    rbuf, _ = _padded(ref, pad=0, lead=0)
    dbuf, _ = _padded(dis, pad=0, lead=0)
    with _engine(48, 32) as eng:
        assert np.array_equal(eng.cross_sse(ref, dis, k_lo, k_hi), want)
        assert np.array_equal(_resident(eng, rbuf, dbuf, 0, 40, 45, k_lo, k_hi), want)
        assert np.array_equal(eng.cross_sse(dis, ref, -64, 64), R.cross_sse(dis, ref, -64, 64))   # the widest band


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_accumulator_limit_at_the_extremes(bpc):
    """512 x 288 = 147 456 pixels, more than the 131 072 an i32 accumulator of centred products may take"""
    dt, top = (np.uint8 if bpc == 8 else np.uint16), (1 << bpc) - 1
    zero, full = np.zeros((288, 512), dt), np.full((288, 512), top, dt)
    with _engine(512, 288, bpc) as eng:
        got = eng.cross_sse([zero, zero], [zero, zero], 0, 0)
        assert got.tolist() == [[0], [0]]
        got = eng.cross_sse([zero, zero], [full, full], -1, 0)
        assert got.tolist() == [[(1 << 64) - 1, 147456 * top * top], [147456 * top * top] * 2]
        got = eng.cross_sse([full, zero], [full, zero], 0, 1)
        assert got.tolist() == [[0, 147456 * top * top], [0, (1 << 64) - 1]]


_CHILD = """
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
from tests import align_ref as R
from tests.test_gpu_align import _engine
out = {}
for name in ("tile_edge", "tails"):
    ref, dis, (k_lo, k_hi) = R.gpu_clip(name)
    a = R.GPU_CLIPS[name][0]
    with _engine(a["w"], a["h"], a["bpc"]) as eng:
        out[name] = eng.cross_sse(ref, dis, k_lo, k_hi)
np.savez(sys.argv[2], **out)
"""


def test_partner_paths_agree(tmp_path):
    """the plain-VALU kernel (PQA_XSSE_MFMA=0, read at pqa_create) returns the arrays of the MFMA kernel"""
    script, res = tmp_path / "child.py", tmp_path / "valu.npz"
    script.write_text(_CHILD)
    env = dict(os.environ, PQA_XSSE_MFMA="0")
    r = subprocess.run([sys.executable, str(script), ROOT, str(res)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    valu = np.load(res)
    for name in ("tile_edge", "tails"):
        ref, dis, (k_lo, k_hi) = R.gpu_clip(name)
        a = R.GPU_CLIPS[name][0]
        with _engine(a["w"], a["h"], a["bpc"]) as eng:
            mfma = eng.cross_sse(ref, dis, k_lo, k_hi)
        assert np.array_equal(mfma, valu[name]) and np.array_equal(mfma, R.cross_sse(ref, dis, k_lo, k_hi))


def test_independent_of_the_scoring_chain():
    from pqa2_amd import _native as N
    rng = np.random.default_rng(7)
    ref = [rng.integers(0, 256, (48, 64)).astype(np.uint8) for _ in range(6)]
    dis = [np.clip(r.astype(int) + rng.integers(-9, 10, r.shape), 0, 255).astype(np.uint8) for r in ref]

    def run(with_call):
        with _engine(64, 48, features=N.FEAT_VMAF | N.FEAT_PSNR | N.FEAT_SSIM, max_batch=4) as eng:
            mats = []
            for i in range(6):
                eng.submit(i, [ref[i]], [dis[i]])
                if with_call and i in (0, 2, 4):    # inside a pending batch, and right after one was launched
                    mats.append(eng.cross_sse(ref, dis, -2, 2))
                    mats.append(eng.cross_sse(ref, dis, -2, 2))
            return eng.collect(0, 6), mats
    plain, _ = run(False)
    mixed, mats = run(True)
    assert np.array_equal(plain.view(np.uint64), mixed.view(np.uint64))
    want = R.cross_sse(ref, dis, -2, 2)
    assert all(np.array_equal(m, want) for m in mats)


def _write_pair(tmp_path):
    from pqa2_amd.yuvio import VideoInfo, write_y4m
    ref, dis, _ = R.gpu_clip("end_to_end")
    assert len(ref) == 24 and len(dis) == 28
    info = VideoInfo(width=64, height=48, fps_num=24, fps_den=1, bit_depth=8, mono=True, hshift=0, vshift=0, chroma_tag="mono")
    paths = {}
    for key, frames in (("ref", ref), ("dis", dis), ("ref_cut", ref[:24]), ("dis_cut", dis[3:27])):
        paths[key] = str(tmp_path / (key + ".y4m"))
        write_y4m(paths[key], [[f] for f in frames], info)
    return paths


def test_end_to_end_offset_repeat_and_trimmed_records(tmp_path):
    from pqa2_amd.pipeline import score_files
    p = _write_pair(tmp_path)
    res = score_files(p["ref"], p["dis"], "vmaf_v0.6.1", align=8)
    al = res["alignment"]
    assert al["offset_frames"] == 3 and al["repeated"] == [26] and al["dropped"] == [] and al["searched"] == [-8, 8]
    assert al["offset_seconds"] == 3 / 24 and al["mse"] < 1000 and al["confidence"] > 10
    by_hand = score_files(p["ref_cut"], p["dis_cut"], "vmaf_v0.6.1")
    assert res["records"].shape == by_hand["records"].shape == (24, 24)
    assert np.array_equal(res["records"].view(np.uint64), by_hand["records"].view(np.uint64))
    assert "alignment" not in by_hand


def test_analyzer_writes_the_alignment_key(tmp_path):
    from pqa2_amd.vmaf_analyzer import VMAFAnalyzer
    p = _write_pair(tmp_path)
    an = VMAFAnalyzer()
    an.set_output_directory(str(tmp_path))
    an.set_test_name("align")
    an.set_advanced_options(align_enabled=True, align_max_offset=8)
    lines = []
    an.status_update.connect(lines.append)
    results = an.analyze_videos(p["ref"], p["dis"])
    assert results and results["alignment"]["offset_frames"] == 3 and results["alignment"]["repeated"] == [26]
    assert json.load(open(results["json_path"]))["alignment"]["searched"] == [-8, 8]
    assert len(results["raw_results"]["frames"]) == 24
    assert any("offset +3 frames" in s for s in lines)
