"""The band moments on the MI355X (csrc/band_moments.hip, pqa_band_moments / pqa_band_moments_device): the twelve sums of every
level equal the restatement (tests/spectrum_ref.py) as integers -- smallest calls and argument rules, the seams of the
kernel's 64 x 64 block and of the levels' coverage, every load width on padded and offset layouts, the accumulator limits on
flat frames, stripes and checkerboards, the clamp, long and tall planes, the stated bound at 8192 x 8192, more frames than two
staging chunks, a plane size other than the context's; the calls leave the scoring chain alone and agree with the engine's
own SSE and with the tile moments."""
import ctypes as C

import numpy as np
import pytest

from tests import spectrum_ref as R

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


def _resident(eng, rbuf, rlead, dbuf, dlead, n, shape, levels):
    """(moments, bytes of one load the launch takes) of two clips uploaded as they lie in their buffers"""
    import torch
    es = rbuf.dtype.itemsize
    tr = torch.from_numpy(rbuf.view(np.uint8).reshape(-1)).cuda()
    td = torch.from_numpy(dbuf.view(np.uint8).reshape(-1)).cuda()
    torch.cuda.synchronize()
    pr, pd = tr.data_ptr() + rlead * es, td.data_ptr() + dlead * es
    bits = pr | pd | rbuf.strides[1] | rbuf.strides[0] | dbuf.strides[1] | dbuf.strides[0]
    load = 16 if bits % 16 == 0 else 4 if bits % 4 == 0 else es      # load_bytes of plane_scan.h
    got = eng.band_moments_resident(pr, rbuf.strides[1], rbuf.strides[0], pd, dbuf.strides[1], dbuf.strides[0], shape, n, levels)
    return got, load


def _equal(got, want):
    return got.dtype == np.uint64 and got.shape == want.shape and np.array_equal(got, want)


def test_the_binding_states_the_kernels_constants():
    import os
    import re
    from pqa2_amd import _native as N
    src = open(os.path.join(os.path.dirname(N.LIB_PATH), "kernels.h")).read()
    assert int(re.search(r"kBandChunk\s*=\s*(\d+)", src).group(1)) == N.BAND_CHUNK == 8
    assert int(re.search(r"kBandSums\s*=\s*(\d+)", src).group(1)) == N.BAND_SUMS == 3 == N.load().pqa_band_sums()
    assert C.sizeof(N.PqaBandSpec) == 16


@pytest.mark.parametrize("bpc", [8, 10])
def test_smallest_calls_and_argument_rules(bpc):
    from pqa2_amd import _native as N
    ref, dis = R.random_pairs(bpc, 2, 16, 16, bpc)
    es = ref[0].itemsize
    with _engine(16, 16, bpc) as eng:
        for L in range(1, 7):
            for w, h in ((1, 1), (2, 2), (3, 3), (2, 66), (66, 2), (16, 16)):
                sr, sd = R.random_pairs(3 + w + h, 2, w, h, bpc)
                got = eng.band_moments(sr, sd, L)
                assert got.shape == (2, L, 4, 3) and _equal(got, R.band_moments(sr, sd, L, bpc)), (L, w, h)
                assert (w, h) != (1, 1) or not got.any()
            assert eng.band_moments([], [], L).shape == (0, L, 4, 3)
            assert eng.band_moments_resident(0, 16 * es, 256 * es, 0, 16 * es, 256 * es, (16, 16), 0, L).shape[0] == 0
        got = eng.band_moments(ref, dis, 3)

        sp = eng._band_spec((16, 16), 3)
        out = np.zeros((2, 3, 4, 3), np.uint64)
        keep_r, rp, rs = eng._luma_list(ref, "reference", (16, 16))
        keep_d, dp, ds = eng._luma_list(dis, "captured", (16, 16))
        lib, ctx = eng.lib, eng._ctx

        def spec(**kw):
            s = eng._band_spec((kw.pop("height", 16), kw.pop("width", 16)), kw.pop("levels", 3))
            for k, v in kw.items():
                setattr(s, k, v)
            return C.byref(s)
        null_frame = (C.c_void_p * 2)(rp[0], None)
        dev = 4096      # never dereferenced: every call below is refused before any device call
        o = out.ctypes.data

        def host(s=None, r=rp, rst=rs, d=dp, dst=ds, n=2, to=o):
            return lib.pqa_band_moments(ctx, C.byref(sp) if s is None else s, r, rst, d, dst, n, to)

        def device(s=None, r=dev, rrp=16 * es, rfp=256 * es, d=dev, drp=16 * es, dfp=256 * es, n=2, to=o):
            return lib.pqa_band_moments_device(ctx, C.byref(sp) if s is None else s, r, rrp, rfp, d, drp, dfp, n, to)
        calls = {
            "null spec": lambda: lib.pqa_band_moments(ctx, None, rp, rs, dp, ds, 2, o),
            "null spec, device": lambda: lib.pqa_band_moments_device(ctx, None, dev, 16 * es, 256 * es, dev, 16 * es, 256 * es, 2, o),
            "null reference list": lambda: host(r=None),
            "null captured list": lambda: host(d=None),
            "null reference frame": lambda: host(r=null_frame),
            "null captured frame": lambda: host(d=null_frame),
            "null output": lambda: host(to=None),
            "null reference clip": lambda: device(r=None),
            "null captured clip": lambda: device(d=None),
            "null output, device": lambda: device(to=None),
            "struct_size": lambda: host(spec(struct_size=12)),
            "struct_size, device": lambda: device(spec(struct_size=20)),
            "levels 0": lambda: host(spec(levels=0)),
            "levels 7": lambda: host(spec(levels=7)),
            "levels 0, device": lambda: device(spec(levels=0)),
            "levels 2^31, device": lambda: device(spec(levels=1 << 31)),
            "width 0": lambda: host(spec(width=0)),
            "height 0": lambda: host(spec(height=0)),
            "width 8193": lambda: host(spec(width=8193), rst=8193 * es, dst=8193 * es),
            "height 8193": lambda: device(spec(height=8193)),
            "short reference stride": lambda: host(rst=16 * es - 1),
            "short captured stride": lambda: host(dst=16 * es - 1),
            "negative stride": lambda: host(rst=-16 * es),
            "negative captured stride": lambda: host(dst=-16 * es),
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
            assert _equal(eng.band_moments(ref, dis, 3), got), name      # a refused call leaves the context usable
        assert not out.any()
        assert host(n=0) == N.PQA_OK and device(n=0) == N.PQA_OK and not out.any()
        del keep_r, keep_d
        with pytest.raises(ValueError):
            eng.band_moments(ref, dis[:1], 3)
        with pytest.raises(ValueError):
            eng.band_moments(ref, [dis[0], dis[1][:8]], 3)      # planes of two sizes


SEAMS = (63, 64, 65, 127, 129, 191)


@pytest.mark.parametrize("bpc", [8, 10])
def test_seams_of_block_and_coverage(bpc):
    """every width and height of SEAMS at six levels: blocks that are partly outside, coefficients that exist at level l but
    not at l + 1, a last odd row or column that the levels above use and the levels below ignore; every width meets every
    height once in the six cyclic pairings, half of them resident on an offset layout"""
    with _engine(64, 64, bpc) as eng:
        for k in range(len(SEAMS)):
            for n, w in enumerate(SEAMS):
                h = SEAMS[(n + k) % len(SEAMS)]
                ref, dis = R.random_pairs(w * 7 + h + bpc, 1, w, h, bpc)
                want = R.band_moments(ref, dis, 6, bpc)
                if k % 2 == 0:
                    assert _equal(eng.band_moments(ref, dis, 6), want), (w, h)
                else:
                    rbuf, _ = _padded(ref, pad=0, lead=0)
                    dbuf, _ = _padded(dis, pad=3, lead=1)
                    assert _equal(_resident(eng, rbuf, 0, dbuf, 1, 1, (h, w), 6)[0], want), (w, h)


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_a_plane_with_tails_at_every_depth(bpc):
    """200 x 70: two workgroups and a tail of 8 columns, one block and a tail of 6 rows; every number of levels"""
    ref, dis = R.random_pairs(20 + bpc, 2, 200, 70, bpc)
    with _engine(200, 70, bpc) as eng:
        for L in range(1, 7):
            assert _equal(eng.band_moments(ref, dis, L), R.band_moments(ref, dis, L, bpc)), L


@pytest.mark.parametrize("bpc", [8, 10])
def test_every_load_width(bpc):
    """50 x 18 (a row is no whole number of 16-byte loads) as a contiguous 16-byte-aligned clip with row padding to 64 samples
    (the 16-byte loads), with a base 4 samples in and 56-sample rows (the 4-byte loads), with rows padded by 5 samples and a
    base one sample in (sample by sample), and with the two clips on different pitches; host and resident entries agree"""
    ref, dis = R.random_pairs(30 + bpc, 3, 50, 18, bpc)
    want = R.band_moments(ref, dis, 4, bpc)
    es = ref[0].itemsize
    seen = set()
    with _engine(50, 18, bpc) as eng:
        assert _equal(eng.band_moments(ref, dis, 4), want)
        for (rpad, rlead), (dpad, dlead) in (((14, 0), (14, 0)), ((6, 4), (6, 4)), ((5, 1), (5, 1)), ((14, 0), (6, 4)),
                                              ((14, 0), (5, 1)), ((30, 0), (14, 0))):
            rbuf, rviews = _padded(ref, rpad, rlead)
            dbuf, dviews = _padded(dis, dpad, dlead)
            assert _equal(eng.band_moments(rviews, dviews, 4), want), (rpad, rlead, dpad, dlead)
            got, load = _resident(eng, rbuf, rlead, dbuf, dlead, 3, (18, 50), 4)
            assert _equal(got, want), (rpad, rlead, dpad, dlead, load)
            seen.add(load)
    assert seen == {16, 4, es}


def _patterns(top, dt, size=128):
    """flat top, then per level vertical stripes, horizontal stripes and checkerboards of 0 / top with period 2^l: H, V and D
    of level l at their maxima"""
    y, x = np.mgrid[0:size, 0:size]
    out = [np.full((size, size), top, dt)]
    for l in range(1, 7):
        half = 1 << (l - 1)
        sx, sy = (x // half) % 2, (y // half) % 2
        out += [(top * (1 - sx)).astype(dt), (top * (1 - sy)).astype(dt), (top * (1 - (sx ^ sy))).astype(dt)]
    return out


@pytest.mark.parametrize("bpc", [8, 12])
def test_accumulator_limits(bpc):
    """128 x 128, six levels: both clips at the pattern (the largest squares and products), and the reference at the pattern
    against its inverse (sum r d of a detail band at its negative extreme)"""
    top = (1 << bpc) - 1
    pats = _patterns(top, _dt(bpc))
    ref = pats + pats[1:]
    dis = pats + [(top - p).astype(_dt(bpc)) for p in pats[1:]]
    with _engine(128, 128, bpc) as eng:
        got = eng.band_moments(ref, dis, 6)
    assert _equal(got, R.band_moments(ref, dis, 6, bpc))
    S = R.signed(got)
    for l in range(1, 7):
        n = (128 >> l) ** 2
        assert S[0, l - 1, 3].tolist() == [n * (top * 4 ** l) ** 2] * 3      # A at its maximum
        for o in range(3):
            amp = 2 * top * 4 ** (l - 1)
            same, inv = S[1 + 3 * (l - 1) + o, l - 1, o], S[len(pats) + 3 * (l - 1) + o, l - 1, o]
            assert same.tolist() == [n * amp * amp] * 3 and inv.tolist() == [n * amp * amp, n * amp * amp, -n * amp * amp], (l, o)


def test_samples_above_the_maximum_are_clamped():
    rng = np.random.default_rng(5)
    ref = [rng.integers(0, 1 << 16, (40, 70)).astype(np.uint16)]
    dis = [rng.integers(0, 1 << 16, (40, 70)).astype(np.uint16)]
    assert (ref[0] > 1023).any() and (dis[0] > 1023).any()
    clamped = R.band_moments([np.minimum(f, 1023) for f in ref], [np.minimum(f, 1023) for f in dis], 3, 10)
    with _engine(70, 40, 10) as eng:
        got = eng.band_moments(ref, dis, 3)
    assert _equal(got, clamped) and _equal(got, R.band_moments(ref, dis, 3, 10))


@pytest.mark.parametrize("w,h", [(8192, 64), (64, 8192)])
def test_long_and_tall_planes_at_12_bit(w, h):
    ref, dis = R.random_pairs(w + 1, 1, w, h, 12)
    with _engine(64, 64, 12) as eng:
        assert _equal(eng.band_moments(ref, dis, 6), R.band_moments(ref, dis, 6, 12))


def test_the_stated_bound_at_8192_x_8192_and_12_bit():
    """flat top: every A band is n_l (top 4^l)^2 three times, the details are zero; the largest is just below 2^62"""
    top = 4095
    plane = np.full((8192, 8192), top, np.uint16)
    with _engine(64, 64, 12) as eng:
        got = eng.band_moments([plane], [plane], 6)
    want = np.zeros((1, 6, 4, 3), np.uint64)
    for l in range(1, 7):
        want[0, l - 1, 3, :] = np.uint64((8192 >> l) ** 2 * (top * 4 ** l) ** 2)
    assert _equal(got, want) and (1 << 61) < int(got[0, 5, 3, 0]) < (1 << 62)


def test_more_frames_than_two_staging_chunks():
    ref, dis = R.random_pairs(50, 17, 16, 16)
    want = R.band_moments(ref, dis, 4)
    assert len({want[f].tobytes() for f in range(17)}) == 17
    rbuf, _ = _padded(ref, pad=0, lead=0)
    dbuf, _ = _padded(dis, pad=0, lead=0)
    with _engine(16, 16) as eng:
        assert _equal(eng.band_moments(ref, dis, 4), want)
        assert _equal(_resident(eng, rbuf, 0, dbuf, 0, 17, (16, 16), 4)[0], want)
        assert _equal(eng.band_moments(ref[:2], dis[:2], 4), want[:2])      # a shorter call after a longer one


@pytest.mark.parametrize("bpc", [8, 10])
def test_a_plane_size_other_than_the_contexts(bpc):
    with _engine(50, 18, bpc) as eng:
        for w, h in ((25, 9), (300, 140)):
            ref, dis = R.random_pairs(70 + w, 2, w, h, bpc)
            assert _equal(eng.band_moments(ref, dis, 5), R.band_moments(ref, dis, 5, bpc)), (w, h)


def _scored_clip(w=64, h=48):
    rng = np.random.default_rng(7)
    ref = [rng.integers(0, 256, (h, w)).astype(np.uint8) for _ in range(6)]
    dis = [np.clip(r.astype(int) + rng.integers(-9, 10, r.shape), 0, 255).astype(np.uint8) for r in ref]
    return ref, dis


def test_independent_of_the_scoring_chain():
    from pqa2_amd import _native as N
    ref, dis = _scored_clip()
    oref, odis = R.random_pairs(8, 2, 100, 30)

    def run(with_call):
        with _engine(64, 48, features=N.FEAT_VMAF | N.FEAT_PSNR | N.FEAT_SSIM, max_batch=4) as eng:
            got = []
            for i in range(6):
                eng.submit(i, [ref[i]], [dis[i]])
                if with_call and i in (0, 2, 4):    # inside a pending batch, and right after one was launched
                    got.append(eng.band_moments(ref, dis, 4))
                    got.append(eng.band_moments(oref, odis, 2))
            return eng.collect(0, 6), got
    plain, _ = run(False)
    mixed, got = run(True)
    assert np.array_equal(plain.view(np.uint64), mixed.view(np.uint64))
    assert len(got) == 6
    assert all(_equal(g, R.band_moments(ref, dis, 4)) for g in got[0::2])
    assert all(_equal(g, R.band_moments(oref, odis, 2)) for g in got[1::2])


def test_parseval_against_the_engines_own_sse():
    """kernel against kernel, 128 x 192 and six levels: sum_l 4^(L-l) (E_H + E_V + E_D)_l + E_A,L == 4^L SSE, with E = sum r^2 -
    2 sum r d + sum d^2 of a band and SSE the slot of the scoring chain"""
    from pqa2_amd import _native as N
    from pqa2_amd.engine import sse_from_records
    ref, dis = _scored_clip(128, 192)
    with _engine(128, 192, features=N.FEAT_VMAF | N.FEAT_PSNR) as eng:
        for i in range(6):
            eng.submit(i, [ref[i]], [dis[i]])
        sse = sse_from_records(eng.collect(0, 6))[:, 0]
        S = R.signed(eng.band_moments(ref, dis, 6))
    E = S[..., 0] + S[..., 1] - 2 * S[..., 2]
    for f in range(6):
        lhs = sum(4 ** (6 - l) * int(E[f, l - 1, :3].sum()) for l in range(1, 7)) + int(E[f, 5, 3])
        assert lhs == 4 ** 6 * int(sse[f])


def test_the_approximations_against_the_tile_moments():
    """kernel against kernel: sum A_l^2, l = 3 ... 6, is the sum of (tile sum r)^2 of pqa_tile_moments with T = 2^l over the
    complete tiles; 200 x 150 has incomplete tiles at every T"""
    ref, dis = R.random_pairs(90, 2, 200, 150)
    with _engine(200, 150) as eng:
        S = R.signed(eng.band_moments(ref, dis, 6))
        for l in range(3, 7):
            T = 1 << l
            M = eng.tile_moments(ref, dis, T).astype(object)[:, :150 // T, :200 // T]
            for f in range(2):
                assert int((M[f, ..., 0] ** 2).sum()) == S[f, l - 1, 3, 0], (l, f)
                assert int((M[f, ..., 1] ** 2).sum()) == S[f, l - 1, 3, 1], (l, f)
                assert int((M[f, ..., 0] * M[f, ..., 1]).sum()) == S[f, l - 1, 3, 2], (l, f)
