"""The table apply on the MI355X (csrc/table_apply.hip, pqa_table_apply / pqa_table_apply_device) against numpy.take
(tests/curve_ref.py): equality, no tolerance, everywhere.  A lane owns 16 bytes of a row -- 16 samples at 8 bit, 8 otherwise --
and stores them whole only when they lie inside the row, so the widths below are a single sample, end one short of, on and
one past a lane's span (15, 16, 17; 31, 33), end inside one (50) and take several lanes and a tail (257); 1030 x 19 passes a
wave's 64 lanes in a row and the 1024 items of a workgroup (test_frames_cross_the_chunk_and_a_workgroup).  The tables are random
permutations unless said otherwise: not monotone, so a mixed-up index shows.  On the parent commit there is no FeatureEngine.table_apply
and score_files has no level_curve."""
import ctypes as C
import json

import numpy as np
import pytest

from tests import curve_ref as CR
from tests import level_ref as R

pytestmark = pytest.mark.gpu

DEPTHS = (8, 10, 12)
SENTINEL = 0xA5


def _dt(bits):
    return np.uint8 if bits == 8 else np.uint16


def _engine(bits=8, **kw):
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    return FeatureEngine(64, 48, bit_depth=bits, n_planes=1, features=kw.pop("features", N.FEAT_PSNR), **kw)


@pytest.fixture(scope="module")
def engs():
    made = {b: _engine(b) for b in DEPTHS}   # the context gives the depth; its size does not matter (plane=None)
    yield made
    for e in made.values():
        e.close()


def _perm(seed, bits):
    return np.random.default_rng(seed).permutation(1 << bits).astype(_dt(bits))


def _noise(seed, bits, shape, n=2):
    """n different planes of noise over the depth's range with a 0 and a maximum in each"""
    rng = np.random.default_rng(seed)
    out = []
    for f in range(n):
        p = rng.integers(0, 1 << bits, shape).astype(_dt(bits))
        flat = p.reshape(-1)
        flat[f % flat.size] = 0
        flat[-1 - (f % flat.size)] = (1 << bits) - 1
        out.append(p)
    return out


def _device(eng, planes, table, pad, lead, in_place=False, spare_rows=1):
    """through pqa_table_apply_device: rows `pad` samples longer than a row, bases `lead` samples in, `spare_rows` rows between
    the frames; source and destination of one layout.  Returns the planes; every destination byte outside the rows' samples
    must have kept the sentinel."""
    import torch
    es = planes[0].dtype.itemsize
    n, (h, w) = len(planes), planes[0].shape
    pitch = (w + pad) * es
    fp = (h + spare_rows) * pitch
    sbuf = np.full(lead * es + n * fp, SENTINEL, np.uint8)
    for f, p in enumerate(planes):
        rows = sbuf[lead * es + f * fp:lead * es + f * fp + h * pitch].reshape(h, pitch)
        rows[:, :w * es] = np.ascontiguousarray(p).view(np.uint8).reshape(h, w * es)
    ts = torch.from_numpy(sbuf).cuda()
    td = ts if in_place else torch.full((lead * es + n * fp,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    eng.table_apply_resident(table, (h, w), ts.data_ptr() + lead * es, pitch, fp, td.data_ptr() + lead * es, pitch, fp, n)
    raw = td.cpu().numpy()
    assert (raw[:lead * es] == SENTINEL).all()
    out = raw[lead * es:].reshape(n, h + spare_rows, pitch)
    assert (out[:, :h, w * es:] == SENTINEL).all() and (out[:, h:, :] == SENTINEL).all(), (w, h, pad, lead)
    if not in_place:     # the source is only read
        assert np.array_equal(ts.cpu().numpy(), sbuf)
    return [np.ascontiguousarray(out[f, :h, :w * es]).view(planes[0].dtype).reshape(h, w) for f in range(n)]


# ---- the smallest call and the argument rules ------------------------------------------------------------------------------
def test_smallest_call_and_no_frames(engs):
    for bits in DEPTHS:
        eng, table = engs[bits], _perm(bits, bits)
        for v in (0, 1, (1 << bits) - 1):
            got = eng.table_apply([np.full((1, 1), v, _dt(bits))], table, plane=None)
            assert len(got) == 1 and got[0].shape == (1, 1) and got[0].dtype == _dt(bits) and got[0][0, 0] == table[v]
            assert _device(eng, [np.full((1, 1), v, _dt(bits))], table, 0, 0)[0][0, 0] == table[v]
        assert eng.table_apply([], table, plane=None) == []
        eng.table_apply_resident(table, (4, 4), 0, 8, 32, 0, 8, 32, 0)      # no frames: nothing is touched, not even the pointers
    got = engs[8].table_apply([np.zeros((48, 64), np.uint8)], _perm(1, 8))   # plane=0: the context's own luma size
    assert got[0].shape == (48, 64) and (got[0] == _perm(1, 8)[0]).all()
    with pytest.raises(ValueError):
        engs[8].table_apply([np.zeros((4, 4), np.uint8)], _perm(1, 8))
    with pytest.raises(ValueError):
        engs[8].table_apply([np.zeros((4, 4), np.uint8)], np.arange(255), plane=None)


@pytest.mark.parametrize("bits", [8, 10])
def test_argument_rules(engs, bits):
    import torch
    from pqa2_amd import _native as N
    eng, es = engs[bits], (1 if bits == 8 else 2)
    w, h = 18, 10
    row = w * es
    buf = torch.zeros(1 << 13, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    q = p + 4096
    table = np.arange(1 << bits).astype(_dt(bits))
    tp = table.ctypes.data

    def spec(**kw):
        sp = eng._plane_spec(N.PqaTableSpec, (h, w))
        for k, v in kw.items():
            setattr(sp, k, v)
        return sp

    def refused(rc_call, word):
        with pytest.raises(N.PqaError) as e:
            eng._check(rc_call())
        assert e.value.code == N.PQA_EINVAL and word in str(e.value), str(e.value)

    dev = lambda sp, t=tp, s=p, srp=row, sfp=row * h, d=q, drp=row, dfp=row * h, n=1: (
        lambda: eng.lib.pqa_table_apply_device(eng._ctx, C.byref(sp) if sp is not None else None, t or None, s or None, srp, sfp, d or None, drp, dfp, n))
    refused(dev(None), "null spec")
    refused(dev(spec(struct_size=8)), "struct_size")
    for k in ("width", "height"):
        for v in (0, 8193):
            refused(dev(spec(**{k: v})), "size")
    refused(dev(spec(), n=-1), "negative")
    refused(dev(spec(), t=0), "null table")
    refused(dev(spec(), s=0), "null")
    refused(dev(spec(), d=0), "null")
    refused(dev(spec(), srp=row - es), "source pitch")
    refused(dev(spec(), drp=row - es), "destination pitch")
    if es == 2:      # an odd device base or pitch at 16 bit
        refused(dev(spec(), srp=row + 1), "sample size")
        refused(dev(spec(), drp=row + 1), "sample size")
        refused(dev(spec(), sfp=row * h + 1), "sample size")
        refused(dev(spec(), dfp=row * h + 1), "sample size")
        refused(dev(spec(), s=p + 1), "sample size")
        refused(dev(spec(), d=q + 1), "sample size")
        for at, v in ((0, 1024), (1023, 1024), (517, 65535)):     # a 10-bit table holding 1024
            bad = table.copy()
            bad[at] = v
            refused(dev(spec(), t=bad.ctypes.data), "table entry")
            with pytest.raises(N.PqaError, match="table entry"):
                eng.table_apply([np.zeros((h, w), np.uint16)], bad, plane=None)
    else:            # an 8-bit table cannot hold an entry above 255: the binding refuses what does not fit the sample type
        with pytest.raises(N.PqaError, match="table entry"):
            eng.table_apply([np.zeros((h, w), np.uint8)], np.arange(256) + 1, plane=None)
    # the host entry: a null list, a null frame, short rows
    a, o = np.zeros((h, w), _dt(bits)), np.zeros((h, w), _dt(bits))
    sptr, dptr, null = (C.c_void_p * 1)(a.ctypes.data), (C.c_void_p * 1)(o.ctypes.data), (C.c_void_p * 1)(None)
    host = lambda sp, t=tp, s=sptr, ss=row, d=dptr, ds=row, n=1: (lambda: eng.lib.pqa_table_apply(eng._ctx, C.byref(sp), t or None, s, ss, d, ds, n))
    refused(host(spec(), s=None), "null")
    refused(host(spec(), d=None), "null")
    refused(host(spec(), s=null), "null")
    refused(host(spec(), d=null), "null")
    refused(host(spec(), t=0), "null table")
    refused(host(spec(), ss=row - 1), "stride")
    refused(host(spec(), ds=row - 1), "stride")
    refused(host(spec(), n=-2), "negative")
    refused(host(spec(width=0)), "size")
    # nothing was written, and both entries work afterwards: a refused call leaves the context usable
    assert not o.any() and not buf.cpu().numpy().any()
    assert eng.lib.pqa_table_apply_device(eng._ctx, C.byref(spec()), tp, None, row, row * h, None, row, row * h, 0) == 0
    a[:] = 7
    flipped = table[::-1].copy()
    eng._check(host(spec(), t=flipped.ctypes.data)())
    assert (o == (1 << bits) - 1 - 7).all()
    eng._check(dev(spec())())


# ---- tails, pitches and depths -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", [1, 3])
@pytest.mark.parametrize("w", [1, 15, 16, 17, 31, 33, 50, 257])
def test_tails_pitches_and_depths(engs, w, h):
    """the host entry on contiguous frames, the host entry on views (5 samples of sentinel padding, the base one sample in)
    and the resident entry on such views and on rows that allow the 16-byte path all agree with numpy.take"""
    for bits in DEPTHS:
        eng, table = engs[bits], _perm(w * 3 + h + bits, bits)
        planes = _noise(w + 100 * h + bits, bits, (h, w), n=2)
        want = [CR.table_apply(p, table, bits) for p in planes]
        got = eng.table_apply(planes, table, plane=None)
        assert all(np.array_equal(g, x) and g.dtype == x.dtype for g, x in zip(got, want)), (bits, w, h)
        buf = np.full((2, h, w + 5), SENTINEL * 0x0101 & ((1 << 8 * planes[0].itemsize) - 1), _dt(bits))
        buf[:, :, 1:w + 1] = np.stack(planes)
        keep = buf.copy()
        got = eng.table_apply([buf[f, :, 1:w + 1] for f in range(2)], table, plane=None)
        assert all(np.array_equal(g, x) for g, x in zip(got, want)) and np.array_equal(buf, keep), (bits, w, h)
        es = planes[0].itemsize
        for pad, lead in ((5, 1), (0, 0), (16 // es - w % (16 // es), 0), (3, 3)):     # the third: a pitch that is a multiple of 16 bytes
            got = _device(eng, planes, table, pad, lead)
            assert all(np.array_equal(g, x) for g, x in zip(got, want)), (bits, w, h, pad, lead)


# ---- every level ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits, side", [(8, 16), (10, 32), (12, 64)])
def test_every_level_through_a_permutation(engs, bits, side):
    eng = engs[bits]
    rng = np.random.default_rng(bits)
    plane = rng.permutation(1 << bits).astype(_dt(bits)).reshape(side, side)       # every level once, shuffled over the plane
    for seed in (1, 2):
        table = _perm(seed + bits, bits)
        want = table[plane]
        assert sorted(want.ravel().tolist()) == list(range(1 << bits))
        assert np.array_equal(eng.table_apply([plane], table, plane=None)[0], want)
        assert np.array_equal(_device(eng, [plane], table, 0, 0)[0], want)
        assert np.array_equal(_device(eng, [plane], table, 1, 1)[0], want)


# ---- containers and in place ---------------------------------------------------------------------------------------------------
def test_samples_above_the_depth_read_the_last_entry(engs):
    eng, table = engs[10], _perm(77, 10)
    plane = _noise(5, 10, (5, 21), n=1)[0]
    plane[0, 0], plane[2, 7], plane[4, 20], plane[3, 16] = 1024, 65535, 1024, 0x8000
    want = CR.table_apply(plane, table, 10)
    assert want[0, 0] == want[2, 7] == want[4, 20] == want[3, 16] == table[1023]
    assert np.array_equal(eng.table_apply([plane], table, plane=None)[0], want)
    for pad, lead in ((0, 0), (3, 0), (2, 1)):
        assert np.array_equal(_device(eng, [plane], table, pad, lead)[0], want)


@pytest.mark.parametrize("bits", DEPTHS)
def test_in_place_and_identity(engs, bits):
    eng = engs[bits]
    planes = _noise(bits, bits, (7, 83), n=3)
    table = _perm(bits + 40, bits)
    want = [CR.table_apply(p, table, bits) for p in planes]
    for pad, lead in ((0, 0), (5, 1), (16 // planes[0].itemsize - 83 % (16 // planes[0].itemsize), 0)):
        got = _device(eng, planes, table, pad, lead, in_place=True)
        assert all(np.array_equal(g, x) for g, x in zip(got, want)), (bits, pad, lead)
    ident = np.arange(1 << bits).astype(_dt(bits))
    assert all(g.tobytes() == p.tobytes() for g, p in zip(eng.table_apply(planes, ident, plane=None), planes))
    assert all(g.tobytes() == p.tobytes() for g, p in zip(_device(eng, planes, ident, 5, 1), planes))


# ---- frames ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [9, 17])
def test_frames_cross_the_chunk(engs, n):
    """9 and 17 frames of 16 x 16, each different, cross the host entry's chunk of 8; in device memory a frame pitch larger
    than the plane (three spare rows)"""
    for bits in (8, 10):
        eng, table = engs[bits], _perm(n + bits, bits)
        planes = _noise(n, bits, (16, 16), n=n)
        assert len({p.tobytes() for p in planes}) == n
        want = [CR.table_apply(p, table, bits) for p in planes]
        got = eng.table_apply(planes, table, plane=None)
        assert len(got) == n and all(np.array_equal(g, x) for g, x in zip(got, want))
        got = _device(eng, planes, table, 0, 0, spare_rows=3)
        assert len(got) == n and all(np.array_equal(g, x) for g, x in zip(got, want))


def test_frames_cross_the_chunk_and_a_workgroup(engs):
    """1030 x 19 at 8 bit: 65 lanes a row, 1235 items of 16 bytes, more than the 1024 of one workgroup, rows that start in the
    middle of a wave"""
    eng, table = engs[8], _perm(3, 8)
    planes = _noise(9, 8, (19, 1030), n=2)
    want = [CR.table_apply(p, table, 8) for p in planes]
    assert all(np.array_equal(g, x) for g, x in zip(eng.table_apply(planes, table, plane=None), want))
    for pad, lead in ((0, 0), (10, 0), (5, 1)):
        assert all(np.array_equal(g, x) for g, x in zip(_device(eng, planes, table, pad, lead), want))


# ---- independence ----------------------------------------------------------------------------------------------------------------
def test_independent_of_the_scoring_chain():
    from pqa2_amd import _native as N
    rng = np.random.default_rng(7)
    ref = [rng.integers(0, 256, (48, 64)).astype(np.uint8) for _ in range(6)]
    dis = [np.clip(r.astype(int) + rng.integers(-9, 10, r.shape), 0, 255).astype(np.uint8) for r in ref]
    planes, table = _noise(11, 8, (37, 130), n=3), _perm(12, 8)

    def run(with_call):
        with _engine(features=N.FEAT_VMAF | N.FEAT_PSNR | N.FEAT_SSIM, max_batch=4) as e:
            outs = []
            for i in range(6):
                e.submit(i, [ref[i]], [dis[i]])
                if with_call and i in (0, 2, 4):    # inside a pending batch, and right after one was launched
                    outs.append(e.table_apply(planes, table, plane=None))
                    outs.append(e.table_apply([dis[i]], table))
            return e.collect(0, 6), outs
    plain, _ = run(False)
    mixed, outs = run(True)
    assert np.array_equal(plain.view(np.uint64), mixed.view(np.uint64))
    want = [CR.table_apply(p, table, 8) for p in planes]
    assert len(outs) == 6 and all(np.array_equal(g, x) for o in outs[0::2] for g, x in zip(o, want))
    assert all(np.array_equal(o[0], table[dis[i]]) for o, i in zip(outs[1::2], (0, 2, 4)))


# ---- end to end --------------------------------------------------------------------------------------------------------------------
W, H, N_FRAMES = 64, 48, 6


def _write_pairs(tmp_path, gamma=1.3):
    """a full-range 4:2:0 reference, its capture with a gamma leg on the luma, and the capture mapped back by hand through
    align.curve_lut of the restated transfer table"""
    from pqa2_amd import align as AL
    from pqa2_amd.yuvio import VideoInfo, write_y4m
    info = VideoInfo(width=W, height=H, fps_num=24, fps_den=1, bit_depth=8, mono=False, hshift=1, vshift=1, chroma_tag="420",
                     color_range="full")
    ref = [[R.smooth_field(70 + t, W, H, 0, 255, t)] + [R.smooth_field(80 + 7 * p + t, W // 2, H // 2, 16, 240, t) for p in range(2)]
           for t in range(N_FRAMES)]
    cap = [[CR.gamma_capture(f[0], gamma), f[1].copy(), f[2].copy()] for f in ref]
    table = AL.curve_lut(R.level_stats([f[0] for f in ref], [f[0] for f in cap], 8), 8)
    back = [[CR.table_apply(f[0], table, 8), f[1], f[2]] for f in cap]
    paths = {}
    for key, clip in (("ref", ref), ("dis", cap), ("dis_back", back)):
        paths[key] = str(tmp_path / (key + ".y4m"))
        write_y4m(paths[key], clip, info)
    return paths


def test_end_to_end_report_and_apply(tmp_path):
    from pqa2_amd.pipeline import score_files
    p = _write_pairs(tmp_path)
    plain = score_files(p["ref"], p["dis"], "vmaf_v0.6.1")
    rep = score_files(p["ref"], p["dis"], "vmaf_v0.6.1", level_align="report", level_curve=True)
    lv = rep["alignment"]["levels"]
    assert (lv["kind"], lv["mismatch"], lv["applied"], lv["curve_applied"], lv["mse_after"]) == ("curve", True, False, False, None)
    assert abs(lv["gamma"] - 1.3) < 0.02 and [lv["planes"][k]["kind"] for k in "yuv"] == ["curve", "identity", "identity"]
    assert np.array_equal(rep["records"].view(np.uint64), plain["records"].view(np.uint64))
    off = score_files(p["ref"], p["dis"], "vmaf_v0.6.1", level_align="apply")
    assert off["alignment"]["levels"]["kind"] != "curve" and "mse_monotone" not in off["alignment"]["levels"]
    done = score_files(p["ref"], p["dis"], "vmaf_v0.6.1", level_align="apply", level_curve=True)
    lv = done["alignment"]["levels"]
    assert [lv["planes"][k]["applied"] for k in "yuv"] == [True, False, False] and lv["curve_applied"]
    assert lv["mse_after"] < lv["mse_identity"] and lv["mse_after"] < lv["mse_affine"]
    by_hand = score_files(p["ref"], p["dis_back"], "vmaf_v0.6.1")
    assert done["records"].shape == by_hand["records"].shape == (N_FRAMES, 24)
    assert np.array_equal(done["records"].view(np.uint64), by_hand["records"].view(np.uint64))
    assert not np.array_equal(done["records"].view(np.uint64), plain["records"].view(np.uint64))
    assert not np.array_equal(done["records"].view(np.uint64), off["records"].view(np.uint64))
    for k in done["metrics"]:
        assert np.array_equal(np.asarray(done["metrics"][k]), np.asarray(by_hand["metrics"][k])), k


def test_analyzer_corrects_and_writes_the_curve(tmp_path):
    from pqa2_amd.pipeline import score_files
    from pqa2_amd.vmaf_analyzer import VMAFAnalyzer
    p = _write_pairs(tmp_path)
    an = VMAFAnalyzer()
    an.set_output_directory(str(tmp_path))
    an.set_test_name("curve")
    an.set_advanced_options(level_correct_enabled=True, level_curve_enabled=True)
    lines = []
    an.status_update.connect(lines.append)
    results = an.analyze_videos(p["ref"], p["dis"])
    assert results and results["alignment"]["levels"]["kind"] == "curve"
    lv = json.load(open(results["json_path"]))["alignment"]["levels"]
    assert lv["applied"] is True and lv["curve_applied"] is True and lv["frames"] == N_FRAMES and lv["planes"]["u"]["applied"] is False
    assert any("transfer curve" in s and "gamma 1.3" in s and "corrected on Y" in s for s in lines)
    by_hand = score_files(p["ref"], p["dis_back"], "vmaf_v0.6.1")
    want = [float(v) for v in by_hand["metrics"]["vmaf"]]
    got = [fr["metrics"]["vmaf"] for fr in results["raw_results"]["frames"]]
    assert got == pytest.approx(want, abs=1e-6)     # the log is written with six decimals
