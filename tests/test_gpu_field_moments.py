"""The field moments on the MI355X (csrc/field_moments.hip, pqa_field_moments / pqa_field_moments_device): the 14 words of every
transition equal the numpy restatement (tests/field_ref.py) bit for bit -- smallest calls and argument rules, tails, every load
width on padded and offset layouts, every depth and the clamp, the seams of the kernel's block with a bright sample at every
seam position of each of the four planes, the accumulator limits against the closed form, the STAGING SEAM of the host entry
(the last pair of a chunk is the predecessor of the next chunk's first), a plane size other than the context's; the calls
leave the scoring chain alone, and score_files re-weaves a field-shifted Y4M back to the records of the progressive capture."""
import ctypes as C

import numpy as np
import pytest

from tests import field_ref as R

pytestmark = pytest.mark.gpu


def _engine(w, h, bpc=8, **kw):
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    return FeatureEngine(w, h, bit_depth=bpc, n_planes=kw.pop("n_planes", 1), features=kw.pop("features", N.FEAT_PSNR), **kw)


def _dt(bpc):
    return np.uint8 if bpc == 8 else np.uint16


def _padded(frames, pad=5, lead=1):
    """the same frames as views into one buffer: rows `pad` samples longer than a row, base `lead` samples in"""
    h, w = frames[0].shape
    buf = np.zeros((len(frames), h, w + pad), frames[0].dtype)
    buf[:, :, lead:lead + w] = np.stack(frames)
    return buf, [buf[i, :, lead:lead + w] for i in range(len(frames))]


def _resident(eng, rbuf, rlead, dbuf, dlead, n, shape):
    """(moments, bytes of one load the launch takes) of two clips uploaded as they lie in their buffers"""
    import torch
    es = rbuf.dtype.itemsize
    tr = torch.from_numpy(rbuf.view(np.uint8).reshape(-1)).cuda()
    td = torch.from_numpy(dbuf.view(np.uint8).reshape(-1)).cuda()
    torch.cuda.synchronize()
    pr, pd = tr.data_ptr() + rlead * es, td.data_ptr() + dlead * es
    bits = pr | pd | rbuf.strides[1] | rbuf.strides[0] | dbuf.strides[1] | dbuf.strides[0]
    load = 16 if bits % 16 == 0 else 4 if bits % 4 == 0 else es      # load_bytes of plane_scan.h
    got = eng.field_moments_resident(pr, rbuf.strides[1], rbuf.strides[0], pd, dbuf.strides[1], dbuf.strides[0], shape, n)
    return got, load


def _equal(got, want):
    return got.dtype == np.uint64 and got.shape == want.shape and np.array_equal(got, want)


def test_the_binding_states_the_kernels_constants():
    import os
    import re
    from pqa2_amd import _native as N
    src = open(os.path.join(os.path.dirname(N.LIB_PATH), "kernels.h")).read()
    assert int(re.search(r"kFieldChunk\s*=\s*(\d+)", src).group(1)) == N.FIELD_CHUNK == 8
    assert int(re.search(r"kFieldSums\s*=\s*(\d+)", src).group(1)) == N.FIELD_SUMS == R.SUMS == 14
    assert int(re.search(r"kFieldCols\s*=\s*(\d+)", src).group(1)) == N.FIELD_COLS
    assert int(re.search(r"kFieldRows\s*=\s*(\d+)", src).group(1)) == N.FIELD_ROWS and N.FIELD_ROWS % 2 == 0
    assert C.sizeof(N.PqaFieldSpec) == 12


@pytest.mark.parametrize("bpc", [8, 10])
def test_smallest_calls_and_argument_rules(bpc):
    from pqa2_amd import _native as N
    ref, dis = R.random_pairs(bpc, 3, 16, 16, bpc)
    es = ref[0].itemsize
    with _engine(64, 48, bpc) as eng:
        got = eng.field_moments(ref, dis)
        assert got.shape == (2, 14) and _equal(got, R.field_moments(ref, dis, bpc))
        assert _equal(eng.field_moments(ref[:2], dis[:2]), R.field_moments(ref[:2], dis[:2], bpc))      # n = 2
        for w, h in ((1, 2), (1, 3), (2, 2), (17, 5)):
            sr, sd = R.random_pairs(3 + w + h, 3, w, h, bpc, noise=100)
            assert _equal(eng.field_moments(sr, sd), R.field_moments(sr, sd, bpc)), (w, h)
        assert eng.field_moments([], []).shape == (0, 14) and eng.field_moments(ref[:1], dis[:1]).shape == (0, 14)
        for n in (0, 1):
            assert eng.field_moments_resident(0 if n == 0 else 4096, 16 * es, 256 * es, 0 if n == 0 else 4096, 16 * es, 256 * es,
                                              (16, 16), n).shape == (0, 14)

        sp = eng._field_spec((16, 16))
        out = np.zeros((2, 14), np.uint64)
        keep_r, rp, rs = eng._luma_list(ref, "reference", (16, 16))
        keep_d, dp, ds = eng._luma_list(dis, "captured", (16, 16))
        lib, ctx = eng.lib, eng._ctx

        def spec(**kw):
            s = eng._field_spec((kw.pop("height", 16), kw.pop("width", 16)))
            for k, v in kw.items():
                setattr(s, k, v)
            return C.byref(s)
        null_frame = (C.c_void_p * 3)(rp[0], None, rp[2])
        dev = 4096      # never dereferenced: every call below is refused before any device call
        o = out.ctypes.data

        def host(s=None, r=rp, rst=rs, d=dp, dst=ds, n=3, to=o):
            return lib.pqa_field_moments(ctx, C.byref(sp) if s is None else s, r, rst, d, dst, n, to)

        def device(s=None, r=dev, rrp=16 * es, rfp=256 * es, d=dev, drp=16 * es, dfp=256 * es, n=3, to=o):
            return lib.pqa_field_moments_device(ctx, C.byref(sp) if s is None else s, r, rrp, rfp, d, drp, dfp, n, to)
        calls = {
            "null spec": lambda: lib.pqa_field_moments(ctx, None, rp, rs, dp, ds, 3, o),
            "null spec, device": lambda: lib.pqa_field_moments_device(ctx, None, dev, 16 * es, 256 * es, dev, 16 * es, 256 * es, 3, o),
            "null reference list": lambda: host(r=None),
            "null captured list": lambda: host(d=None),
            "null reference frame": lambda: host(r=null_frame),
            "null captured frame": lambda: host(d=null_frame),
            "null output": lambda: host(to=None),
            "null reference clip": lambda: device(r=None),
            "null captured clip": lambda: device(d=None),
            "null output, device": lambda: device(to=None),
            "struct_size": lambda: host(spec(struct_size=8)),
            "struct_size, device": lambda: device(spec(struct_size=16)),
            "height 1": lambda: host(spec(height=1)),
            "height 1, device": lambda: device(spec(height=1)),
            "height 0": lambda: host(spec(height=0)),
            "width 0": lambda: host(spec(width=0)),
            "width 8193": lambda: host(spec(width=8193), rst=8193 * es, dst=8193 * es),
            "height 8193": lambda: device(spec(height=8193)),
            "short reference stride": lambda: host(rst=16 * es - 1),
            "short captured stride": lambda: host(dst=16 * es - 1),
            "negative stride": lambda: host(rst=-16 * es),
            "short reference pitch": lambda: device(rrp=15 * es),
            "short captured pitch": lambda: device(drp=15 * es),
            "negative pitch": lambda: device(rrp=-16 * es),
            "negative frame count": lambda: host(n=-1),
            "negative frame count, device": lambda: device(n=-1),
        }
        if es == 2:      # a pitch that is no multiple of the sample size
            calls["odd stride"] = lambda: host(rst=33)
            calls["odd captured stride"] = lambda: host(dst=35)
            calls["odd row pitch"] = lambda: device(rrp=33)
            calls["odd frame pitch"] = lambda: device(dfp=513)
        for name, call in calls.items():
            assert call() == N.PQA_EINVAL, name
        assert host(spec(height=1)) == N.PQA_EINVAL and b"row pair" in lib.pqa_last_error(ctx)      # the entry's own rule
        assert not out.any()
        assert _equal(eng.field_moments(ref, dis), got)      # refused calls leave the context usable
        assert host(n=0) == N.PQA_OK and device(n=0) == N.PQA_OK and not out.any()
        assert host(n=1) == N.PQA_OK and device(n=1) == N.PQA_OK and not out.any()      # one frame: no transition, nothing written
        assert host(n=1, to=None) == N.PQA_OK and device(n=1, to=None) == N.PQA_OK and host(n=0, to=None) == N.PQA_OK
        del keep_r, keep_d
        with pytest.raises(ValueError):
            eng.field_moments(ref, dis[:1])


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_tails_pitches_and_depths(bpc):
    """widths around the lanes' 16 bytes and one past the column block, on 7 rows (an odd height); a contiguous clip, rows padded
    to a multiple of 16 bytes (16-byte loads), a base 4 samples in with rows 4-byte aligned (4-byte loads), rows padded by 5
    samples and a base one sample in (sample by sample), and the two clips on different layouts"""
    from pqa2_amd import _native as N
    es = 1 if bpc == 8 else 2
    seen = set()
    with _engine(64, 48, bpc) as eng:
        for w in (15, 16, 17, 31, 33, 63, 65, N.FIELD_COLS + 1):
            ref, dis = R.random_pairs(w + bpc, 3, w, 7, bpc, noise=200)
            want = R.field_moments(ref, dis, bpc)
            assert _equal(eng.field_moments(ref, dis), want), w
            a16 = -w % 16 or 16      # rows a multiple of 16 samples: 16-byte loads at either sample size
            a4 = -(w + 4) % 4 + 4
            for (rpad, rlead), (dpad, dlead) in (((a16, 0), (a16, 0)), ((a4, 4), (a4, 4)), ((5, 1), (5, 1)), ((a16, 0), (5, 1))):
                rbuf, rviews = _padded(ref, rpad, rlead)
                dbuf, dviews = _padded(dis, dpad, dlead)
                assert _equal(eng.field_moments(rviews, dviews), want), (w, rpad, rlead, dpad, dlead)
                got, load = _resident(eng, rbuf, rlead, dbuf, dlead, 3, (7, w))
                assert _equal(got, want), (w, rpad, rlead, dpad, dlead, load)
                seen.add(load)
    assert seen == {16, 4, es}


def test_samples_above_the_maximum_are_clamped():
    rng = np.random.default_rng(5)
    ref = [rng.integers(0, 1 << 16, (40, 70)).astype(np.uint16) for _ in range(3)]
    dis = [rng.integers(0, 1 << 16, (40, 70)).astype(np.uint16) for _ in range(3)]
    assert (ref[0] > 1023).any() and (dis[0] > 1023).any()
    clamped = R.field_moments([np.minimum(f, 1023) for f in ref], [np.minimum(f, 1023) for f in dis], 10)
    with _engine(70, 40, 10) as eng:
        got = eng.field_moments(ref, dis)
    assert _equal(got, clamped) and _equal(got, R.field_moments(ref, dis, 10))


@pytest.mark.parametrize("bpc", [8, 10])
def test_seams_of_the_block(bpc):
    """plane sizes at block - 1, block, block + 1 and 2 block + 1 each way on random planes"""
    from pqa2_amd import _native as N
    bc, br = N.FIELD_COLS, N.FIELD_ROWS
    with _engine(64, 64, bpc) as eng:
        for w, h in ((bc - 1, br - 1), (bc, br), (bc + 1, br + 1), (2 * bc + 1, 20), (20, 2 * br + 1), (bc + 1, br - 1)):
            ref, dis = R.random_pairs(w * 7 + h + bpc, 3, w, h, bpc, noise=300)
            assert _equal(eng.field_moments(ref, dis), R.field_moments(ref, dis, bpc)), (w, h)


@pytest.mark.parametrize("bpc", [8, 10])
def test_a_bright_sample_at_every_seam_position(bpc):
    """flat planes of 2 block + 1 each way with one bright sample at every seam position in turn, in each of the four planes a
    transition reads: a row or column counted twice or not at all changes a word.  Every word is a known multiple of the
    squared step; the planes of all positions go through two calls, one per clip"""
    from pqa2_amd import _native as N
    bc, br = N.FIELD_COLS, N.FIELD_ROWS
    w, h = 2 * bc + 1, 2 * br + 1
    lanes = 16 if bpc == 8 else 8
    xs = sorted({0, lanes - 1, lanes, bc - 1, bc, bc + 1, 2 * bc - 1, 2 * bc})
    ys = sorted({0, 1, 2, br - 2, br - 1, br, br + 1, 2 * br - 2, 2 * br - 1, 2 * br})      # the last: the uncounted row
    step = 7 if bpc == 8 else 600
    flat = np.full((h, w), 50, _dt(bpc))
    spots = [(y, x) for y in ys for x in xs]
    # the clip flat, spot, flat, spot, ...: every spot frame is R_k / D_k of one transition and R_{k-1} / D_{k-1} of the next
    frames = [flat]
    for y, x in spots:
        f = flat.copy()
        f[y, x] += step
        frames += [f, flat]
    n = len(frames)
    with _engine(w, h, bpc) as eng:
        in_ref = eng.field_moments(frames, [flat] * n)
        in_dis = eng.field_moments([flat] * n, frames)
    assert _equal(in_ref, R.field_moments(frames, [flat] * n, bpc)) and _equal(in_dis, R.field_moments([flat] * n, frames, bpc))
    e = step * step
    for i, (y, x) in enumerate(spots):
        p, counted = y & 1, y < 2 * (h // 2)
        as_k, as_prev = in_ref[2 * i], in_ref[2 * i + 1]      # the spot in R_k, then in R_{k-1}
        assert sorted(np.flatnonzero(as_k).tolist()) == (sorted([p, 2 + p, 8 + p, 10 + p, 13]) if counted else []), (y, x)
        assert sorted(np.flatnonzero(as_prev).tolist()) == (sorted([4 + p, 6 + p]) if counted else []), (y, x)
        as_k, as_prev = in_dis[2 * i], in_dis[2 * i + 1]      # the spot in D_k, then in D_{k-1}
        assert sorted(np.flatnonzero(as_k).tolist()) == (sorted([2 * p, 2 * p + 1, 4 + 2 * p, 5 + 2 * p, 12]) if counted else []), (y, x)
        assert sorted(np.flatnonzero(as_prev).tolist()) == (sorted([8 + 2 * p, 9 + 2 * p]) if counted else []), (y, x)
        for rec in (in_ref[2 * i], in_ref[2 * i + 1], in_dis[2 * i], in_dis[2 * i + 1]):
            assert set(rec.tolist()) <= {0, e}, (y, x)


@pytest.mark.parametrize("bpc", [8, 12])
def test_accumulator_limits_against_the_closed_form(bpc):
    """2048 x 256: sixteen blocks across and two down, every lane's share full.  Parities set to top and 0 so that each of the
    14 words reaches h2 * W * top^2 in some frame"""
    top = (1 << bpc) - 1
    w, h = 2048, 256
    full = h // 2 * w * top * top
    zero, one = np.zeros((h, w), _dt(bpc)), np.full((h, w), top, _dt(bpc))
    even, odd = zero.copy(), zero.copy()
    even[0::2] = top      # parity 0 at the top, parity 1 at 0
    odd[1::2] = top
    if bpc == 12:
        assert full > 1 << 40 and 32 * top * top > (1 << 32) // 16      # past 32 bits within 16 lanes' shares
    with _engine(w, h, bpc) as eng:
        # captured all top against a reference all 0: the twelve cross words; the combs are 0
        got = eng.field_moments([zero, zero], [one, one])
        assert got[0].tolist() == [full] * 12 + [0, 0]
        # both clips with one parity at the top: the combs, and the words of unequal levels
        got = eng.field_moments([even, even], [even, even])
        assert got[0].tolist() == [0, full, full, 0] * 3 + [full, full]
        got = eng.field_moments([even, even], [odd, odd])
        assert got[0].tolist() == [full, 0, 0, full] * 3 + [full, full]
        seq_r, seq_d = [zero, one, even, odd, zero], [one, odd, zero, even, even]
        assert _equal(eng.field_moments(seq_r, seq_d), R.field_moments(seq_r, seq_d, bpc))


@pytest.mark.parametrize("bpc", [8, 10])
def test_the_staging_seam(bpc):
    """random frames, n = FIELD_CHUNK + 2 and 2 FIELD_CHUNK + 1 and their neighbours: the host entry uploads chunks of
    FIELD_CHUNK pairs and keeps the last pair of a chunk on the device as the predecessor of the next chunk's first; it equals
    the resident entry and the restatement transition by transition"""
    from pqa2_amd import _native as N
    K = N.FIELD_CHUNK
    ref, dis = R.random_pairs(50 + bpc, 2 * K + 2, 48, 32, bpc, noise=100)
    want = R.field_moments(ref, dis, bpc)
    assert len({want[t].tobytes() for t in range(len(want))}) == len(want)
    rbuf, _ = _padded(ref, pad=0, lead=0)
    dbuf, _ = _padded(dis, pad=0, lead=0)
    with _engine(48, 32, bpc) as eng:
        for n in (2 * K + 2, K, K + 1, K + 2, 2 * K + 1):      # the longest first: the buffers then hold stale frames of a longer call
            host = eng.field_moments(ref[:n], dis[:n])
            res = _resident(eng, rbuf, 0, dbuf, 0, n, (32, 48))[0]
            assert host.shape == res.shape == (n - 1, 14)
            for t in range(n - 1):
                assert np.array_equal(host[t], want[t]), (n, t)
                assert np.array_equal(res[t], want[t]), (n, t)
        # a clip that starts inside the other one: the first chunk must not see a predecessor left behind
        assert _equal(eng.field_moments(ref[5:16], dis[5:16]), want[5:15])
        assert _equal(eng.field_moments(ref[:2], dis[:2]), want[:1])      # a shorter call after a longer one


@pytest.mark.parametrize("bpc", [8, 10])
def test_a_plane_size_other_than_the_contexts(bpc):
    with _engine(50, 18, bpc) as eng:
        for w, h in ((25, 9), (100, 70)):
            ref, dis = R.random_pairs(70 + w, 3, w, h, bpc)
            assert _equal(eng.field_moments(ref, dis), R.field_moments(ref, dis, bpc)), (w, h)


def test_independent_of_the_scoring_chain():
    from pqa2_amd import _native as N
    rng = np.random.default_rng(7)
    ref = [rng.integers(0, 256, (48, 64)).astype(np.uint8) for _ in range(6)]
    dis = [np.clip(r.astype(int) + rng.integers(-9, 10, r.shape), 0, 255).astype(np.uint8) for r in ref]
    oref, odis = R.random_pairs(8, 3, 100, 30)

    def run(with_call):
        with _engine(64, 48, features=N.FEAT_VMAF | N.FEAT_PSNR | N.FEAT_SSIM, max_batch=4) as eng:
            got = []
            for i in range(6):
                eng.submit(i, [ref[i]], [dis[i]])
                if with_call and i in (0, 2, 4):    # inside a pending batch, and right after one was launched
                    got.append(eng.field_moments(ref, dis))
                    got.append(eng.field_moments(oref, odis))
            return eng.collect(0, 6), got
    plain, _ = run(False)
    mixed, got = run(True)
    assert np.array_equal(plain.view(np.uint64), mixed.view(np.uint64))
    assert len(got) == 6
    assert all(_equal(g, R.field_moments(ref, dis)) for g in got[0::2])
    assert all(_equal(g, R.field_moments(oref, odis)) for g in got[1::2])


def test_score_files_reweaves_a_late_bottom_field(tmp_path):
    """96 x 64 4:2:0, 10 frames, bottom field late: "apply" gives the records of the progressive capture scored from u_lo on,
    "report" those of the option off"""
    from pqa2_amd.pipeline import score_files
    from pqa2_amd.yuvio import VideoInfo, write_y4m
    n = 10
    info = VideoInfo(width=96, height=64, fps_num=25, fps_den=1, bit_depth=8, mono=False, hshift=1, vshift=1, chroma_tag="420")
    ref = R.moving_clip(5, n, 96, 64)
    cap = R.with_noise(ref, 105)
    paths = {}
    for name, frames in (("ref", ref), ("cap", cap), ("late", R.field_late(cap, 1))):
        paths[name] = str(tmp_path / (name + ".y4m"))
        write_y4m(paths[name], frames, info)
    kw = dict(psnr=True, ssim=True)
    plain = score_files(paths["ref"], paths["late"], "vmaf_v0.6.1", **kw)
    rep = score_files(paths["ref"], paths["late"], "vmaf_v0.6.1", field_align="report", **kw)
    assert np.array_equal(rep["records"].view(np.uint64), plain["records"].view(np.uint64))
    f = rep["alignment"]["fields"]
    assert f["kind"] == "field_shift" and f["state"] == [0, 0, 1, -1] and not f["applied"] and "alignment" not in plain
    fixed = score_files(paths["ref"], paths["late"], "vmaf_v0.6.1", field_align="apply", **kw)
    f = fixed["alignment"]["fields"]
    assert f["applied"] and (f["u_lo"], f["u_hi"], f["unfilled"]) == (0, n - 1, [])
    good = score_files(paths["ref"], paths["cap"], "vmaf_v0.6.1", **kw)
    assert len(fixed["records"]) == n - 1
    assert np.array_equal(fixed["records"].view(np.uint64), good["records"][f["u_lo"]:f["u_lo"] + n - 1].view(np.uint64))
