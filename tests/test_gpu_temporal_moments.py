"""The temporal moments on the MI355X (csrc/temporal_moments.hip, pqa_temporal_moments / pqa_temporal_moments_device): the seven
sums of every tile and transition equal the numpy restatement (tests/temporal_ref.py) bit for bit -- smallest calls and
argument rules, the seams of the kernel's 64 x 64 block and of the tiles, every load width on padded and offset layouts, the
accumulator limits on flat frames in both orders and the clamp, the STAGING SEAM of the host entry (the last pair of a chunk of
8 is the predecessor of the next chunk's first), a plane size other than the context's; the calls leave the scoring chain
alone and agree with the project's older kernels (tile_moments, cross_sse)."""
import ctypes as C

import numpy as np
import pytest

from tests import temporal_ref as R
from tests import tile_ref

pytestmark = pytest.mark.gpu

TILES = (8, 16, 32, 64)


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


def _resident(eng, rbuf, rlead, dbuf, dlead, n, shape, tile):
    """(moments, bytes of one load the launch takes) of two clips uploaded as they lie in their buffers"""
    import torch
    es = rbuf.dtype.itemsize
    tr = torch.from_numpy(rbuf.view(np.uint8).reshape(-1)).cuda()
    td = torch.from_numpy(dbuf.view(np.uint8).reshape(-1)).cuda()
    torch.cuda.synchronize()
    pr, pd = tr.data_ptr() + rlead * es, td.data_ptr() + dlead * es
    bits = pr | pd | rbuf.strides[1] | rbuf.strides[0] | dbuf.strides[1] | dbuf.strides[0]
    load = 16 if bits % 16 == 0 else 4 if bits % 4 == 0 else es      # load_bytes of plane_scan.h
    got = eng.temporal_moments_resident(pr, rbuf.strides[1], rbuf.strides[0], pd, dbuf.strides[1], dbuf.strides[0], shape, n, tile)
    return got, load


def _equal(got, want):
    return got.dtype == np.uint64 and got.shape == want.shape and np.array_equal(got, want)


def test_the_binding_states_the_kernels_constants():
    import os
    import re
    from pqa2_amd import _native as N
    src = open(os.path.join(os.path.dirname(N.LIB_PATH), "kernels.h")).read()
    assert int(re.search(r"kTemporalChunk\s*=\s*(\d+)", src).group(1)) == N.TEMPORAL_CHUNK == 8
    assert int(re.search(r"kTemporalSums\s*=\s*(\d+)", src).group(1)) == N.TEMPORAL_SUMS == 7
    assert N.load().pqa_temporal_sums() == 7 and N.TEMPORAL_SIGNED == R.SIGNED == (0, 1, 4, 5)
    assert C.sizeof(N.PqaTemporalSpec) == 16


@pytest.mark.parametrize("bpc", [8, 10])
def test_smallest_calls_and_argument_rules(bpc):
    from pqa2_amd import _native as N
    ref, dis = tile_ref.random_pairs(bpc, 3, 16, 16, bpc)
    es = ref[0].itemsize
    sref, sdis = tile_ref.random_pairs(1, 2, 64, 48, bpc, noise=9)      # what the context scores afterwards
    with _engine(64, 48, bpc, features=N.FEAT_VMAF | N.FEAT_PSNR) as eng:
        for i in range(2):
            eng.submit(i, [sref[i]], [sdis[i]])
        fresh = eng.collect(0, 2)
    with _engine(64, 48, bpc, features=N.FEAT_VMAF | N.FEAT_PSNR) as eng:
        for T in TILES:
            got = eng.temporal_moments(ref, dis, T)
            assert got.shape == (2, -(-16 // T), -(-16 // T), 7) and _equal(got, R.temporal_moments(ref, dis, T, bpc)), T
            for w, h in ((1, 1), (9, 1), (1, 9)):      # 1 x 1 with n = 2: one transition of one pixel
                sr, sd = tile_ref.random_pairs(3 + w + h, 2, w, h, bpc)
                assert _equal(eng.temporal_moments(sr, sd, T), R.temporal_moments(sr, sd, T, bpc)), (T, w, h)
            assert eng.temporal_moments([], [], T).shape == (0, -(-48 // T), -(-64 // T), 7)      # the context's size
            assert eng.temporal_moments(ref[:1], dis[:1], T).shape == (0, -(-16 // T), -(-16 // T), 7)
            for n in (0, 1):
                assert eng.temporal_moments_resident(0 if n == 0 else 4096, 16 * es, 256 * es, 0 if n == 0 else 4096, 16 * es,
                                                     256 * es, (16, 16), n, T).shape[0] == 0
        got = eng.temporal_moments(ref, dis, 8)

        sp = eng._temporal_spec((16, 16), 8)
        out = np.zeros((2, 2, 2, 7), np.uint64)
        keep_r, rp, rs = eng._luma_list(ref, "reference", (16, 16))
        keep_d, dp, ds = eng._luma_list(dis, "captured", (16, 16))
        lib, ctx = eng.lib, eng._ctx

        def spec(**kw):
            s = eng._temporal_spec((kw.pop("height", 16), kw.pop("width", 16)), kw.pop("tile", 8))
            for k, v in kw.items():
                setattr(s, k, v)
            return C.byref(s)
        null_frame = (C.c_void_p * 3)(rp[0], None, rp[2])
        dev = 4096      # never dereferenced: every call below is refused before any device call
        o = out.ctypes.data

        def host(s=None, r=rp, rst=rs, d=dp, dst=ds, n=3, to=o):
            return lib.pqa_temporal_moments(ctx, C.byref(sp) if s is None else s, r, rst, d, dst, n, to)

        def device(s=None, r=dev, rrp=16 * es, rfp=256 * es, d=dev, drp=16 * es, dfp=256 * es, n=3, to=o):
            return lib.pqa_temporal_moments_device(ctx, C.byref(sp) if s is None else s, r, rrp, rfp, d, drp, dfp, n, to)
        calls = {
            "null spec": lambda: lib.pqa_temporal_moments(ctx, None, rp, rs, dp, ds, 3, o),
            "null spec, device": lambda: lib.pqa_temporal_moments_device(ctx, None, dev, 16 * es, 256 * es, dev, 16 * es, 256 * es, 3, o),
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
            "tile 0": lambda: host(spec(tile=0)),
            "tile 12": lambda: host(spec(tile=12)),
            "tile 4": lambda: device(spec(tile=4)),
            "tile 128": lambda: device(spec(tile=128)),
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
            assert _equal(eng.temporal_moments(ref, dis, 8), got), name      # a refused call leaves the context usable
        assert not out.any()
        assert host(n=0) == N.PQA_OK and device(n=0) == N.PQA_OK and not out.any()
        assert host(n=1) == N.PQA_OK and device(n=1) == N.PQA_OK and not out.any()      # one frame: no transition, nothing written
        assert host(n=1, to=None) == N.PQA_OK
        del keep_r, keep_d
        with pytest.raises(ValueError):
            eng.temporal_moments(ref, dis[:1], 8)
        with pytest.raises(ValueError):
            eng.temporal_moments(ref, [dis[0], dis[1], dis[2][:8]], 8)      # planes of two sizes
        # ... and then it still scores
        for i in range(2):
            eng.submit(i, [sref[i]], [sdis[i]])
        assert np.array_equal(eng.collect(0, 2).view(np.uint64), fresh.view(np.uint64))


@pytest.mark.parametrize("bpc", [8, 10])
@pytest.mark.parametrize("T", [8, 64])
def test_seams_of_block_and_tile(bpc, T):
    """widths and heights at, one short of and one past the kernel's 64 x 64 block, and two blocks plus one by one block plus
    two"""
    sizes = ((63, 63), (64, 64), (65, 65), (63, 65), (65, 63), (129, 66))
    with _engine(64, 64, bpc) as eng:
        for w, h in sizes:
            ref, dis = tile_ref.random_pairs(w * 7 + h + bpc, 3, w, h, bpc)
            want = R.temporal_moments(ref, dis, T, bpc)
            assert _equal(eng.temporal_moments(ref, dis, T), want), (w, h)
            rbuf, _ = _padded(ref, pad=0, lead=0)
            dbuf, _ = _padded(dis, pad=3, lead=1)
            assert _equal(_resident(eng, rbuf, 0, dbuf, 1, 3, (h, w), T)[0], want), (w, h)


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_a_plane_with_tails_at_every_depth(bpc):
    """131 x 67: two blocks and a tail of 3 columns, one block and a tail of 3 rows; every tile size"""
    ref, dis = tile_ref.random_pairs(20 + bpc, 3, 131, 67, bpc)
    with _engine(131, 67, bpc) as eng:
        for T in TILES:
            assert _equal(eng.temporal_moments(ref, dis, T), R.temporal_moments(ref, dis, T, bpc)), T


@pytest.mark.parametrize("bpc", [8, 10])
@pytest.mark.parametrize("T", [8, 32])
def test_every_load_width(bpc, T):
    """50 x 18 (a row is no whole number of 16-byte loads) as a contiguous 16-byte-aligned clip with row padding to 64 samples
    (the 16-byte loads), with a base 4 samples in and 56-sample rows (the 4-byte loads), with rows padded by 5 samples and a
    base one sample in (sample by sample), and with the two clips on different pitches; host and resident entries agree"""
    ref, dis = tile_ref.random_pairs(30 + bpc, 4, 50, 18, bpc)
    want = R.temporal_moments(ref, dis, T, bpc)
    es = ref[0].itemsize
    seen = set()
    with _engine(50, 18, bpc) as eng:
        assert _equal(eng.temporal_moments(ref, dis, T), want)
        for (rpad, rlead), (dpad, dlead) in (((14, 0), (14, 0)), ((6, 4), (6, 4)), ((5, 1), (5, 1)), ((14, 0), (6, 4)),
                                              ((14, 0), (5, 1)), ((30, 0), (14, 0))):
            rbuf, rviews = _padded(ref, rpad, rlead)
            dbuf, dviews = _padded(dis, dpad, dlead)
            assert _equal(eng.temporal_moments(rviews, dviews, T), want), (rpad, rlead, dpad, dlead)
            got, load = _resident(eng, rbuf, rlead, dbuf, dlead, 4, (18, 50), T)
            assert _equal(got, want), (rpad, rlead, dpad, dlead, load)
            seen.add(load)
    assert seen == {16, 4, es}


@pytest.mark.parametrize("bpc", [8, 12])
def test_accumulator_limits_on_flat_frames(bpc):
    """256 x 256 with tiles of 64, flat frames: reference and capture alternating 0 / top in step (a = b = +- top, the largest
    sums of squares and of a b: 4096 * 4095^2 > 2^35, past 32 bits between the lanes), the reference 0 / top against the
    capture top / 0 (a b and a e at their most negative, e^2 at its largest), both in both orders, and a reference that rises
    to half where the capture is at the top (a e near its most positive, top^2 / 4 a pixel)"""
    top = (1 << bpc) - 1
    w = h = 256
    full, zero, half = (np.full((h, w), v, _dt(bpc)) for v in (top, 0, top // 2))
    n = 64 * 64
    with _engine(w, h, bpc) as eng:
        for order in ((zero, full), (full, zero)):
            lo, hi = order
            sign = 1 if lo is zero else -1
            ref, dis = [lo, hi, lo, hi], [lo, hi, lo, hi]
            got = eng.temporal_moments(ref, dis, 64)
            assert _equal(got, R.temporal_moments(ref, dis, 64, bpc))
            S = R.signed(got)
            assert S.shape == (3, 4, 4, 7)
            assert S[0, 0, 0].tolist() == [sign * n * top, sign * n * top, n * top * top, n * top * top, n * top * top, 0, 0]
            assert S[1, 3, 3].tolist() == [-sign * n * top, -sign * n * top, n * top * top, n * top * top, n * top * top, 0, 0]
            ref, dis = [lo, hi, lo], [hi, lo, hi]
            got = eng.temporal_moments(ref, dis, 64)
            assert _equal(got, R.temporal_moments(ref, dis, 64, bpc))
            S = R.signed(got)
            assert S[0, 1, 2].tolist() == [sign * n * top, -sign * n * top, n * top * top, n * top * top, -n * top * top,
                                           -n * top * top, n * top * top]
        ref, dis = [zero, half, zero], [zero, full, full]
        got = eng.temporal_moments(ref, dis, 64)
        assert _equal(got, R.temporal_moments(ref, dis, 64, bpc))
        assert R.signed(got)[0, 0, 0, 5] == n * (top // 2) * (top - top // 2)
    if bpc == 12:
        assert n * top * top > 1 << 35


def test_samples_above_the_maximum_are_clamped():
    rng = np.random.default_rng(5)
    ref = [rng.integers(0, 1 << 16, (40, 70)).astype(np.uint16) for _ in range(3)]
    dis = [rng.integers(0, 1 << 16, (40, 70)).astype(np.uint16) for _ in range(3)]
    assert (ref[0] > 1023).any() and (dis[0] > 1023).any()
    clamped = R.temporal_moments([np.minimum(f, 1023) for f in ref], [np.minimum(f, 1023) for f in dis], 16, 10)
    with _engine(70, 40, 10) as eng:
        got = eng.temporal_moments(ref, dis, 16)
    assert _equal(got, clamped) and _equal(got, R.temporal_moments(ref, dis, 16, 10))


@pytest.mark.parametrize("bpc", [8, 10])
def test_the_staging_seam(bpc):
    """random frames, n = 8, 9, 10, 17 and 18: the host entry uploads chunks of 8 pairs and keeps the last pair of a chunk on
    the device as the predecessor of the next chunk's first; it equals the resident entry and the restatement transition by
    transition"""
    ref, dis = tile_ref.random_pairs(50 + bpc, 18, 48, 32, bpc)
    want = R.temporal_moments(ref, dis, 16, bpc)
    assert len({want[t].tobytes() for t in range(17)}) == 17
    rbuf, _ = _padded(ref, pad=0, lead=0)
    dbuf, _ = _padded(dis, pad=0, lead=0)
    with _engine(48, 32, bpc) as eng:
        for n in (18, 8, 9, 10, 17):      # the longest first: the buffers then hold stale frames of a longer call
            host = eng.temporal_moments(ref[:n], dis[:n], 16)
            res = _resident(eng, rbuf, 0, dbuf, 0, n, (32, 48), 16)[0]
            for t in range(n - 1):
                assert np.array_equal(host[t], want[t]), (n, t)
                assert np.array_equal(res[t], want[t]), (n, t)
            assert host.shape == res.shape == (n - 1, 2, 3, 7)
        # a clip that starts inside the other one: the first chunk must not see a predecessor left behind
        assert _equal(eng.temporal_moments(ref[5:16], dis[5:16], 16), want[5:15])
        assert _equal(eng.temporal_moments(ref[:2], dis[:2], 16), want[:1])      # a shorter call after a longer one


@pytest.mark.parametrize("bpc", [8, 10])
def test_a_plane_size_other_than_the_contexts(bpc):
    with _engine(50, 18, bpc) as eng:
        for w, h in ((25, 9), (100, 70)):
            ref, dis = tile_ref.random_pairs(70 + w, 3, w, h, bpc)
            assert _equal(eng.temporal_moments(ref, dis, 16), R.temporal_moments(ref, dis, 16, bpc)), (w, h)


def _scored_clip():
    rng = np.random.default_rng(7)
    ref = [rng.integers(0, 256, (48, 64)).astype(np.uint8) for _ in range(6)]
    dis = [np.clip(r.astype(int) + rng.integers(-9, 10, r.shape), 0, 255).astype(np.uint8) for r in ref]
    return ref, dis


def test_independent_of_the_scoring_chain():
    from pqa2_amd import _native as N
    ref, dis = _scored_clip()
    oref, odis = tile_ref.random_pairs(8, 3, 100, 30)

    def run(with_call):
        with _engine(64, 48, features=N.FEAT_VMAF | N.FEAT_PSNR | N.FEAT_SSIM, max_batch=4) as eng:
            got = []
            for i in range(6):
                eng.submit(i, [ref[i]], [dis[i]])
                if with_call and i in (0, 2, 4):    # inside a pending batch, and right after one was launched
                    got.append(eng.temporal_moments(ref, dis, 16))
                    got.append(eng.temporal_moments(oref, odis, 8))
            return eng.collect(0, 6), got
    plain, _ = run(False)
    mixed, got = run(True)
    assert np.array_equal(plain.view(np.uint64), mixed.view(np.uint64))
    assert len(got) == 6
    assert all(_equal(g, R.temporal_moments(ref, dis, 16)) for g in got[0::2])
    assert all(_equal(g, R.temporal_moments(oref, odis, 8)) for g in got[1::2])


@pytest.mark.parametrize("T", [8, 64])
def test_against_the_older_kernels(T):
    """kernel against kernel: word 6 of transition k is the tile SSE that tile_moments gives for frame k; words 2 and 3 summed
    over the tiles are cross_sse of the reference (the captured clip) with itself at offset -1"""
    ref, dis = _scored_clip()
    with _engine(64, 48) as eng:
        M = eng.temporal_moments(ref, dis, T)
        tm = eng.tile_moments(ref, dis, T)
        xr = eng.cross_sse(ref, ref, -1, -1)
        xd = eng.cross_sse(dis, dis, -1, -1)
    sse = tm[..., 2] + tm[..., 3] - np.uint64(2) * tm[..., 4]
    assert np.array_equal(M[..., 6], sse[1:])
    assert np.array_equal(M[..., 2].sum(axis=(1, 2), dtype=np.uint64), xr[1:, 0])
    assert np.array_equal(M[..., 3].sum(axis=(1, 2), dtype=np.uint64), xd[1:, 0])
    assert xr[0, 0] == np.uint64(2 ** 64 - 1)      # frame 0 has no predecessor there either


@pytest.mark.parametrize("bpc", [8, 10])
def test_the_walking_form_returns_the_same_integers(bpc, monkeypatch):
    """PQA_TEMPORAL_WALK=1 (read at pqa_create): a workgroup walks through the launch's transitions with its block of the
    previous pair in registers -- the A/B partner of a workgroup per transition.  Block and tile seams, every load width,
    launches of 1, 7 and 8 transitions and the staging seam"""
    monkeypatch.setenv("PQA_TEMPORAL_WALK", "1")
    with _engine(64, 64, bpc) as eng:
        monkeypatch.delenv("PQA_TEMPORAL_WALK")
        for w, h in ((65, 63), (129, 66)):
            ref, dis = tile_ref.random_pairs(w + h + bpc, 4, w, h, bpc)
            for T in (8, 64):
                assert _equal(eng.temporal_moments(ref, dis, T), R.temporal_moments(ref, dis, T, bpc)), (w, h, T)
        ref, dis = tile_ref.random_pairs(90 + bpc, 18, 50, 18, bpc)
        want = R.temporal_moments(ref, dis, 16, bpc)
        for n in (18, 2, 8, 9):
            assert _equal(eng.temporal_moments(ref[:n], dis[:n], 16), want[:n - 1]), n
        for (rpad, rlead), (dpad, dlead) in (((14, 0), (14, 0)), ((6, 4), (6, 4)), ((5, 1), (14, 0))):
            rbuf, _ = _padded(ref, rpad, rlead)
            dbuf, _ = _padded(dis, dpad, dlead)
            assert _equal(_resident(eng, rbuf, rlead, dbuf, dlead, 18, (18, 50), 16)[0], want), (rpad, rlead, dpad, dlead)
