"""The tile moments on the MI355X (csrc/tile_moments.hip, pqa_tile_moments / pqa_tile_moments_device): the six sums of every
tile equal the numpy restatement (tests/tile_ref.py) as integers -- smallest calls and argument rules, the seams of the
kernel's 64 x 64 block and of the tiles, every load width on padded and offset layouts, the accumulator limits on flat frames
and the clamp, more frames than two staging chunks, a plane size other than the context's; the calls leave the scoring chain
alone and add up to the engine's own SSE."""
import ctypes as C

import numpy as np
import pytest

from tests import tile_ref as R

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
    got = eng.tile_moments_resident(pr, rbuf.strides[1], rbuf.strides[0], pd, dbuf.strides[1], dbuf.strides[0], shape, n, tile)
    return got, load


def _equal(got, want):
    return got.dtype == np.uint64 and got.shape == want.shape and np.array_equal(got, want)


def test_the_binding_states_the_kernels_constants():
    import os
    import re
    from pqa2_amd import _native as N
    src = open(os.path.join(os.path.dirname(N.LIB_PATH), "kernels.h")).read()
    assert int(re.search(r"kTileChunk\s*=\s*(\d+)", src).group(1)) == N.TILE_CHUNK == 8
    assert int(re.search(r"kTileSums\s*=\s*(\d+)", src).group(1)) == N.TILE_SUMS == 6
    assert C.sizeof(N.PqaTileSpec) == 16


@pytest.mark.parametrize("bpc", [8, 10])
def test_smallest_calls_and_argument_rules(bpc):
    from pqa2_amd import _native as N
    ref, dis = R.random_pairs(bpc, 2, 16, 16, bpc)
    with _engine(16, 16, bpc) as eng:
        for T in TILES:
            got = eng.tile_moments(ref, dis, T)
            assert got.shape == (2, -(-16 // T), -(-16 // T), 6) and _equal(got, R.tile_moments(ref, dis, T, bpc)), T
            for w, h in ((1, 1), (9, 1), (1, 9)):
                sr, sd = R.random_pairs(3 + w + h, 2, w, h, bpc)
                assert _equal(eng.tile_moments(sr, sd, T), R.tile_moments(sr, sd, T, bpc)), (T, w, h)
            assert eng.tile_moments([], [], T).shape == (0, -(-16 // T), -(-16 // T), 6)
            es = ref[0].itemsize
            assert eng.tile_moments_resident(0, 16 * es, 256 * es, 0, 16 * es, 256 * es, (16, 16), 0, T).shape[0] == 0
        got = eng.tile_moments(ref, dis, 8)

        sp = eng._tile_spec((16, 16), 8)
        out = np.zeros((2, 2, 2, 6), np.uint64)
        keep_r, rp, rs = eng._luma_list(ref, "reference", (16, 16))
        keep_d, dp, ds = eng._luma_list(dis, "captured", (16, 16))
        lib, ctx = eng.lib, eng._ctx

        def spec(**kw):
            s = eng._tile_spec((kw.pop("height", 16), kw.pop("width", 16)), kw.pop("tile", 8))
            for k, v in kw.items():
                setattr(s, k, v)
            return C.byref(s)
        null_frame = (C.c_void_p * 2)(rp[0], None)
        dev = 4096      # never dereferenced: every call below is refused before any device call
        o = out.ctypes.data

        def host(s=None, r=rp, rst=rs, d=dp, dst=ds, n=2, to=o):
            return lib.pqa_tile_moments(ctx, C.byref(sp) if s is None else s, r, rst, d, dst, n, to)

        def device(s=None, r=dev, rrp=16 * es, rfp=256 * es, d=dev, drp=16 * es, dfp=256 * es, n=2, to=o):
            return lib.pqa_tile_moments_device(ctx, C.byref(sp) if s is None else s, r, rrp, rfp, d, drp, dfp, n, to)
        calls = {
            "null spec": lambda: lib.pqa_tile_moments(ctx, None, rp, rs, dp, ds, 2, o),
            "null spec, device": lambda: lib.pqa_tile_moments_device(ctx, None, dev, 16 * es, 256 * es, dev, 16 * es, 256 * es, 2, o),
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
            assert _equal(eng.tile_moments(ref, dis, 8), got), name      # a refused call leaves the context usable
        assert not out.any()
        assert host(n=0) == N.PQA_OK and device(n=0) == N.PQA_OK and not out.any()
        del keep_r, keep_d
        with pytest.raises(ValueError):
            eng.tile_moments(ref, dis[:1], 8)
        with pytest.raises(ValueError):
            eng.tile_moments(ref, [dis[0], dis[1][:8]], 8)      # planes of two sizes


@pytest.mark.parametrize("bpc", [8, 10])
@pytest.mark.parametrize("T", [8, 64])
def test_seams_of_block_and_tile(bpc, T):
    """widths and heights at, one short of and one past the kernel's 64 x 64 block and two blocks plus one; width 9 with
    tiles of 8: a tile of one column"""
    sizes = ((63, 63), (64, 64), (65, 65), (129, 129), (63, 65), (65, 63), (129, 64), (64, 129), (9, 17))
    with _engine(64, 64, bpc) as eng:
        for w, h in sizes:
            ref, dis = R.random_pairs(w * 7 + h + bpc, 2, w, h, bpc)
            want = R.tile_moments(ref, dis, T, bpc)
            assert _equal(eng.tile_moments(ref, dis, T), want), (w, h)
            rbuf, _ = _padded(ref, pad=0, lead=0)
            dbuf, _ = _padded(dis, pad=3, lead=1)
            assert _equal(_resident(eng, rbuf, 0, dbuf, 1, 2, (h, w), T)[0], want), (w, h)


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_a_plane_with_tails_at_every_depth(bpc):
    """200 x 70: three blocks and a tail of 8 columns, one block and a tail of 6 rows; every tile size"""
    ref, dis = R.random_pairs(20 + bpc, 2, 200, 70, bpc)
    with _engine(200, 70, bpc) as eng:
        for T in TILES:
            assert _equal(eng.tile_moments(ref, dis, T), R.tile_moments(ref, dis, T, bpc)), T


@pytest.mark.parametrize("bpc", [8, 10])
@pytest.mark.parametrize("T", [8, 32])
def test_every_load_width(bpc, T):
    """50 x 18 (a row is no whole number of 16-byte loads) as a contiguous 16-byte-aligned clip with row padding to 64 samples
    (the 16-byte loads), with a base 4 samples in and 56-sample rows (the 4-byte loads), with rows padded by 5 samples and a
    base one sample in (sample by sample), and with the two clips on different pitches; host and resident entries agree"""
    ref, dis = R.random_pairs(30 + bpc, 3, 50, 18, bpc)
    want = R.tile_moments(ref, dis, T, bpc)
    es = ref[0].itemsize
    seen = set()
    with _engine(50, 18, bpc) as eng:
        assert _equal(eng.tile_moments(ref, dis, T), want)
        for (rpad, rlead), (dpad, dlead) in (((14, 0), (14, 0)), ((6, 4), (6, 4)), ((5, 1), (5, 1)), ((14, 0), (6, 4)),
                                              ((14, 0), (5, 1)), ((30, 0), (14, 0))):
            rbuf, rviews = _padded(ref, rpad, rlead)
            dbuf, dviews = _padded(dis, dpad, dlead)
            assert _equal(eng.tile_moments(rviews, dviews, T), want), (rpad, rlead, dpad, dlead)
            got, load = _resident(eng, rbuf, rlead, dbuf, dlead, 3, (18, 50), T)
            assert _equal(got, want), (rpad, rlead, dpad, dlead, load)
            seen.add(load)
    assert seen == {16, 4, es}


@pytest.mark.parametrize("bpc", [8, 12])
def test_accumulator_limits_on_flat_frames(bpc):
    """64 x 64 and 128 x 70 with tiles of 64: all samples at the maximum (the largest sums of squares and products: a tile of
    4096 samples of 4095 sums to 68 685 926 400 > 2^35, past 32 bits between the lanes) and r = top against d = 0 (the largest
    differences)"""
    top = (1 << bpc) - 1
    with _engine(64, 64, bpc) as eng:
        for w, h in ((64, 64), (128, 70)):
            full, zero = np.full((h, w), top, _dt(bpc)), np.zeros((h, w), _dt(bpc))
            ref, dis = [full, full, zero], [full, zero, full]
            got = eng.tile_moments(ref, dis, 64)
            assert _equal(got, R.tile_moments(ref, dis, 64, bpc))
            assert got[0, 0, 0].tolist() == [4096 * top, 4096 * top] + [4096 * top * top] * 3 + [0]
            assert got[1, 0, 0].tolist() == [4096 * top, 0, 4096 * top * top, 0, 0, 4096 * top]
    if bpc == 12:
        assert 4096 * top * top > 1 << 35


def test_samples_above_the_maximum_are_clamped():
    rng = np.random.default_rng(5)
    ref = [rng.integers(0, 1 << 16, (40, 70)).astype(np.uint16) for _ in range(2)]
    dis = [rng.integers(0, 1 << 16, (40, 70)).astype(np.uint16) for _ in range(2)]
    assert (ref[0] > 1023).any() and (dis[0] > 1023).any()
    clamped = R.tile_moments([np.minimum(f, 1023) for f in ref], [np.minimum(f, 1023) for f in dis], 16, 10)
    with _engine(70, 40, 10) as eng:
        got = eng.tile_moments(ref, dis, 16)
    assert _equal(got, clamped) and _equal(got, R.tile_moments(ref, dis, 16, 10))


def test_more_frames_than_two_staging_chunks():
    ref, dis = R.random_pairs(50, 17, 48, 32)
    want = R.tile_moments(ref, dis, 16)
    assert len({want[f].tobytes() for f in range(17)}) == 17
    rbuf, _ = _padded(ref, pad=0, lead=0)
    dbuf, _ = _padded(dis, pad=0, lead=0)
    with _engine(48, 32) as eng:
        assert _equal(eng.tile_moments(ref, dis, 16), want)
        assert _equal(_resident(eng, rbuf, 0, dbuf, 0, 17, (32, 48), 16)[0], want)
        assert _equal(eng.tile_moments(ref[:2], dis[:2], 16), want[:2])      # a shorter call after a longer one


@pytest.mark.parametrize("bpc", [8, 10])
def test_a_plane_size_other_than_the_contexts(bpc):
    with _engine(50, 18, bpc) as eng:
        for w, h in ((25, 9), (100, 70)):
            ref, dis = R.random_pairs(70 + w, 2, w, h, bpc)
            assert _equal(eng.tile_moments(ref, dis, 16), R.tile_moments(ref, dis, 16, bpc)), (w, h)


def _scored_clip():
    rng = np.random.default_rng(7)
    ref = [rng.integers(0, 256, (48, 64)).astype(np.uint8) for _ in range(6)]
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
                    got.append(eng.tile_moments(ref, dis, 16))
                    got.append(eng.tile_moments(oref, odis, 8))
            return eng.collect(0, 6), got
    plain, _ = run(False)
    mixed, got = run(True)
    assert np.array_equal(plain.view(np.uint64), mixed.view(np.uint64))
    assert len(got) == 6
    assert all(_equal(g, R.tile_moments(ref, dis, 16)) for g in got[0::2])
    assert all(_equal(g, R.tile_moments(oref, odis, 8)) for g in got[1::2])


@pytest.mark.parametrize("T", [8, 64])
def test_the_tiles_add_up_to_the_engines_own_sse(T):
    """kernel against kernel: the sum over the tiles of sum r^2 - 2 sum r d + sum d^2 is the SSE slot of the scoring chain"""
    from pqa2_amd import _native as N
    from pqa2_amd.engine import sse_from_records
    ref, dis = _scored_clip()
    with _engine(64, 48, features=N.FEAT_VMAF | N.FEAT_PSNR) as eng:
        for i in range(6):
            eng.submit(i, [ref[i]], [dis[i]])
        sse = sse_from_records(eng.collect(0, 6))[:, 0]
        M = eng.tile_moments(ref, dis, T)
    S = M[..., 2] + M[..., 3] - np.uint64(2) * M[..., 4]
    assert S.dtype == np.uint64 and np.array_equal(S.sum(axis=(1, 2), dtype=np.uint64), sse)
