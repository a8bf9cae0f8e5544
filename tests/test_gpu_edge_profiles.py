"""The edge profiles on the MI355X (csrc/edge_profiles.hip, pqa_edge_profiles / pqa_edge_profiles_device): the gradient energy
of both clips and their cross term per row and column line equal the numpy restatement (tests/edge_ref.py) as integers --
smallest calls and argument rules, row tails / pitches / odd base addresses at 8 / 10 / 12 bit with DIFFERENT layouts for the two
clips, every seam of the kernel's decomposition, the accumulator limits on checkerboards and the clamp, more frames than a
staging chunk, a plane size other than the context's; the calls leave the scoring chain alone."""
import ctypes as C

import numpy as np
import pytest

from tests import edge_ref as R

pytestmark = pytest.mark.gpu

STRIPE, BAND, RUN = 1024, 64, 16      # kEdgeStripe, kEdgeBand of csrc/kernels.h; the consecutive rows of one wave (BAND / 4)


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
    import torch
    tr = torch.from_numpy(rbuf.view(np.uint8).reshape(-1)).cuda()
    td = torch.from_numpy(dbuf.view(np.uint8).reshape(-1)).cuda()
    torch.cuda.synchronize()
    return eng.edge_profiles_resident(tr.data_ptr() + rlead * rbuf.dtype.itemsize, rbuf.strides[1], rbuf.strides[0],
                                      td.data_ptr() + dlead * dbuf.dtype.itemsize, dbuf.strides[1], dbuf.strides[0], shape, n)


def _equal(got, want):
    return all(g.dtype == np.uint64 and g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))


def test_the_binding_states_the_kernels_constants():
    import os
    import re
    from pqa2_amd import _native as N
    src = open(os.path.join(os.path.dirname(N.LIB_PATH), "kernels.h")).read()
    assert int(re.search(r"kEdgeStripe\s*=\s*(\d+)", src).group(1)) == STRIPE == N.EDGE_STRIPE
    assert int(re.search(r"kEdgeBand\s*=\s*(\d+)", src).group(1)) == BAND == N.EDGE_BAND
    assert int(re.search(r"kEdgeSums\s*=\s*(\d+)", src).group(1)) == R.SUMS == N.EDGE_SUMS == N.load().pqa_edge_sums()
    assert int(re.search(r"kEdgeChunk\s*=\s*(\d+)", src).group(1)) == N.EDGE_CHUNK


@pytest.mark.parametrize("bpc", [8, 10])
def test_smallest_calls_and_argument_rules(bpc):
    from pqa2_amd import _native as N
    ref, dis = R.random_frames(2, 16, 16, bpc, seed=bpc), R.random_frames(2, 16, 16, bpc, seed=bpc + 1)
    with _engine(16, 16, bpc) as eng:
        got = eng.edge_profiles(ref, dis)
        assert got[0].shape == (2, 16, 3) and got[1].shape == (2, 16, 3) and _equal(got, R.edge_profiles(ref, dis, bpc))
        assert not got[0][:, 0].any() and not got[1][:, 0].any() and got[0][:, 1:, :2].all() and got[1][:, 1:, :2].all()
        for w, h in ((1, 1), (2, 1), (1, 2), (9, 1), (1, 9)):
            sr, sd = R.random_frames(2, h, w, bpc, seed=3 + w + h), R.random_frames(2, h, w, bpc, seed=4 + w + h)
            small = eng.edge_profiles(sr, sd)
            assert _equal(small, R.edge_profiles(sr, sd, bpc)), (w, h)
            assert (h > 1 or not small[0].any()) and (w > 1 or not small[1].any())      # a 1-wide / 1-high plane: zeros that way
        rows, cols = eng.edge_profiles([], [])
        assert rows.shape == (0, 16, 3) and cols.shape == (0, 16, 3)
        es = ref[0].itemsize
        rows, cols = eng.edge_profiles_resident(0, 16 * es, 256 * es, 0, 16 * es, 256 * es, (16, 16), 0)
        assert rows.shape == (0, 16, 3) and cols.shape == (0, 16, 3)

        sp = eng._edge_spec((16, 16))
        out = np.zeros((2, 32, 3), np.uint64)
        keep_r, rp, rs = eng._luma_list(ref, "reference", (16, 16))
        keep_d, dp, ds = eng._luma_list(dis, "captured", (16, 16))
        lib, ctx, o = eng.lib, eng._ctx, out.ctypes.data

        def spec(**kw):
            s = eng._edge_spec((kw.pop("height", 16), kw.pop("width", 16)))
            for k, v in kw.items():
                setattr(s, k, v)
            return C.byref(s)
        null_frame = (C.c_void_p * 2)(rp[0], None)
        dev = 4096      # never dereferenced: every call below is refused before any device call
        rpb, fpb = 16 * es, 256 * es

        def device(spc=None, r=dev, rrp=rpb, rfp=fpb, d=dev, drp=rpb, dfp=fpb, n=2, to=o):
            return lib.pqa_edge_profiles_device(ctx, spc if spc is not None else C.byref(sp), r, rrp, rfp, d, drp, dfp, n, to)
        calls = {
            "null spec": lambda: lib.pqa_edge_profiles(ctx, None, rp, rs, dp, ds, 2, o),
            "null spec, device": lambda: lib.pqa_edge_profiles_device(ctx, None, dev, rpb, fpb, dev, rpb, fpb, 2, o),
            "null reference list": lambda: lib.pqa_edge_profiles(ctx, C.byref(sp), None, rs, dp, ds, 2, o),
            "null captured list": lambda: lib.pqa_edge_profiles(ctx, C.byref(sp), rp, rs, None, ds, 2, o),
            "null reference frame": lambda: lib.pqa_edge_profiles(ctx, C.byref(sp), null_frame, rs, dp, ds, 2, o),
            "null captured frame": lambda: lib.pqa_edge_profiles(ctx, C.byref(sp), rp, rs, null_frame, ds, 2, o),
            "null output": lambda: lib.pqa_edge_profiles(ctx, C.byref(sp), rp, rs, dp, ds, 2, None),
            "null reference clip": lambda: device(r=None),
            "null captured clip": lambda: device(d=None),
            "null output, device": lambda: device(to=None),
            "struct_size": lambda: lib.pqa_edge_profiles(ctx, spec(struct_size=8), rp, rs, dp, ds, 2, o),
            "width 0": lambda: lib.pqa_edge_profiles(ctx, spec(width=0), rp, rs, dp, ds, 2, o),
            "height 0": lambda: lib.pqa_edge_profiles(ctx, spec(height=0), rp, rs, dp, ds, 2, o),
            "width 8193": lambda: lib.pqa_edge_profiles(ctx, spec(width=8193), rp, 8193 * es, dp, 8193 * es, 2, o),
            "height 8193": lambda: device(spc=spec(height=8193)),
            "short reference stride": lambda: lib.pqa_edge_profiles(ctx, C.byref(sp), rp, 16 * es - 1, dp, ds, 2, o),
            "short captured stride": lambda: lib.pqa_edge_profiles(ctx, C.byref(sp), rp, rs, dp, 16 * es - 1, 2, o),
            "negative reference stride": lambda: lib.pqa_edge_profiles(ctx, C.byref(sp), rp, -16 * es, dp, ds, 2, o),
            "negative captured stride": lambda: lib.pqa_edge_profiles(ctx, C.byref(sp), rp, rs, dp, -16 * es, 2, o),
            "short reference pitch": lambda: device(rrp=15 * es),
            "short captured pitch": lambda: device(drp=15 * es),
            "negative reference pitch": lambda: device(rrp=-16 * es),
            "negative captured pitch": lambda: device(drp=-16 * es),
            "negative frame count": lambda: lib.pqa_edge_profiles(ctx, C.byref(sp), rp, rs, dp, ds, -1, o),
            "negative frame count, device": lambda: device(n=-1),
        }
        if es == 2:      # a pitch that is no multiple of the sample size
            calls["odd reference row pitch"] = lambda: device(rrp=33)
            calls["odd captured row pitch"] = lambda: device(drp=33)
            calls["odd reference frame pitch"] = lambda: device(rfp=513)
            calls["odd captured frame pitch"] = lambda: device(dfp=513)
            calls["odd reference stride"] = lambda: lib.pqa_edge_profiles(ctx, C.byref(sp), rp, 33, dp, ds, 2, o)
            calls["odd captured stride"] = lambda: lib.pqa_edge_profiles(ctx, C.byref(sp), rp, rs, dp, 33, 2, o)
        for name, call in calls.items():
            assert call() == N.PQA_EINVAL, name
            assert _equal(eng.edge_profiles(ref, dis), got), name      # a refused call leaves the context usable
        assert not out.any()
        del keep_r, keep_d
        with pytest.raises(ValueError):
            eng.edge_profiles([ref[0], ref[1][:8]], dis)      # planes of two sizes
        with pytest.raises(ValueError):
            eng.edge_profiles(ref, dis[:1])                   # lists of two lengths


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_tails_pitches_and_depths(bpc):
    """50 x 18: a row is no whole number of 16-byte loads; rows padded by 5 samples, base one sample in (the per-sample path);
    the host entry on contiguous frames, on views, and the resident entry agree.  The two clips get DIFFERENT layouts: the load
    width must follow the worse one, whichever clip has it"""
    ref = R.random_frames(3, 18, 50, bpc, seed=10 + bpc, over=True)
    dis = R.random_frames(3, 18, 50, bpc, seed=20 + bpc, over=True)
    want = R.edge_profiles(ref, dis, bpc)
    odd_r, views_r = _padded(ref)                      # rows of 55 samples, base one sample in: the per-sample path
    odd_d, views_d = _padded(dis)
    wide_r, _ = _padded(ref, pad=14, lead=0)           # 64-byte rows at 8 bit, 128-byte rows at 16: the 16-byte loads
    wide_d, _ = _padded(dis, pad=14, lead=0)
    word_r, _ = _padded(ref, pad=6, lead=4)            # 56-sample rows, base 4 samples in: 4-byte but not 16-byte aligned
    word_d, _ = _padded(dis, pad=6, lead=4)
    with _engine(50, 18, bpc) as eng:
        assert _equal(eng.edge_profiles(ref, dis), want)
        assert _equal(eng.edge_profiles(views_r, views_d), want)
        assert _equal(eng.edge_profiles(views_r, dis), want)      # rows of two strides: the binding packs them
        assert _equal(_resident(eng, odd_r, 1, odd_d, 1, 3, (18, 50)), want)
        assert _equal(_resident(eng, wide_r, 0, wide_d, 0, 3, (18, 50)), want)
        assert _equal(_resident(eng, word_r, 4, word_d, 4, 3, (18, 50)), want)
        for (rb, rl), (db, dl) in (((wide_r, 0), (odd_d, 1)), ((odd_r, 1), (wide_d, 0)), ((wide_r, 0), (word_d, 4)),
                                   ((word_r, 4), (wide_d, 0)), ((word_r, 4), (odd_d, 1)), ((odd_r, 1), (word_d, 4))):
            assert _equal(_resident(eng, rb, rl, db, dl, 3, (18, 50)), want), (rb.shape, rl, db.shape, dl)


# one sample on each side of every boundary of the decomposition: stripe, band, a wave's run of rows, a lane's column group
# (16 columns; 16 / 8 / 4 / 2 / 1 samples a load) and load-to-load (64 lanes of a load: 64 V columns, V = 1 ... 16)
SEAM_X = sorted({x for e in (1, 2, 4, 8, 16, 64, 128, 256, 512, STRIPE) for x in (e - 1, e)} | {STRIPE - 16, 3})
SEAM_Y = sorted({y for e in (1, RUN, 2 * RUN, 3 * RUN, BAND) for y in (e - 1, e)})


@pytest.mark.parametrize("bpc,lead", [(8, 0), (8, 1), (8, 4), (10, 0), (10, 1), (10, 2)])
def test_seams_of_the_decomposition(bpc, lead):
    """a width one sample past the column stripe and a height one row past the row band: two stripes and two bands.  Black
    pairs with one bright pixel in R only, D only and both, on each side of each seam: a dropped or doubled difference shows
    in exactly one sum.  lead 0: the 16-byte loads; 4 at 8 bit and 2 at 10: the word loads; otherwise the per-sample path"""
    w, h, top = STRIPE + 1, BAND + 1, (1 << bpc) - 1
    spots = [(y, x) for y in (BAND - 1, BAND) for x in (STRIPE - 1, STRIPE)] * 3     # the corner of stripe and band: all three
    spots += [(SEAM_Y[i % len(SEAM_Y)], x) for i, x in enumerate(SEAM_X)]
    spots += [(y, SEAM_X[(5 * i + 2) % len(SEAM_X)]) for i, y in enumerate(SEAM_Y)]
    spots += [(0, 0), (h - 1, w - 1), (0, w - 1), (h - 1, 0)]
    ref, dis = [], []
    for i, (y, x) in enumerate(spots):
        r, d = np.zeros((h, w), _dt(bpc)), np.zeros((h, w), _dt(bpc))
        if i % 3 != 1:
            r[y, x] = top - (y + x) % 7
        if i % 3 != 0:
            d[y, x] = top - (2 * y + x) % 5
        ref.append(r)
        dis.append(d)
    ref.append(R.random_frames(1, h, w, bpc, seed=60 + bpc)[0])
    dis.append(R.random_frames(1, h, w, bpc, seed=61 + bpc)[0])
    want = R.edge_profiles(ref, dis, bpc)
    for i, (y, x) in enumerate(spots):      # the restatement itself: exactly the four lines the pixel touches, line 0 never
        lines_y, lines_x = [v for v in (y, y + 1) if 1 <= v < h], [v for v in (x, x + 1) if 1 <= v < w]
        for m in ((0,) if i % 3 == 0 else (1,) if i % 3 == 1 else (0, 1, 2)):
            assert np.flatnonzero(want[0][i, :, m]).tolist() == lines_y and np.flatnonzero(want[1][i, :, m]).tolist() == lines_x
        if i % 3 != 2:
            assert not want[0][i, :, 2].any() and not want[1][i, :, 2].any()
    pad = (16 - w % 16) % 16 if lead == 0 else 5 if lead == 1 else 7      # lead 4 / 2: rows of 1032 samples, 4-byte aligned
    rbuf, _ = _padded(ref, pad=pad, lead=lead)
    dbuf, _ = _padded(dis, pad=pad, lead=lead)
    with _engine(64, 64, bpc) as eng:
        assert _equal(eng.edge_profiles(ref, dis), want)
        assert _equal(_resident(eng, rbuf, lead, dbuf, lead, len(ref), (h, w)), want)


@pytest.mark.parametrize("bpc,w,h", [(8, 8192, 3), (8, 3, 8192), (12, 8192, 3), (12, 3, 8192)])
def test_accumulator_limits_on_checkerboards(bpc, w, h):
    """checkerboards of 0 / top: every difference is +-top.  D = R: every line (n top^2, n top^2, +n top^2) with n the samples
    along the line; D the inverted board: a cross term of -n top^2.  A row line of 8192 samples of 4095^2 passes 32 bits in a
    wave's sum after 256 samples, and the signed sum of 8 lanes of 16 is 128 * 4095^2 = 2 146 435 200, 1 048 447 below 2^31.
    At 12 bit also a frame of 0xFFFF samples in the 16-bit container, read as 4095: flat"""
    top = (1 << bpc) - 1
    yy, xx = np.mgrid[0:h, 0:w]
    board = (((yy + xx) & 1) * top).astype(_dt(bpc))
    inv = (top - board).astype(_dt(bpc))
    ref, dis = [board, board], [board, inv]
    if bpc == 12:
        ref.append(np.full((h, w), 0xFFFF, np.uint16))
        dis.append(board)
    with _engine(64, 64, bpc) as eng:
        rows, cols = eng.edge_profiles(ref, dis)
    rs, cs = rows.view(np.int64), cols.view(np.int64)
    for lines, n in ((rs, w), (cs, h)):
        q = n * top * top
        assert not lines[:, 0].any()
        assert (lines[0, 1:] == (q, q, q)).all() and (lines[1, 1:] == (q, q, -q)).all()
        if bpc == 12:
            assert (lines[2, 1:] == (0, q, 0)).all()
    assert _equal((rows, cols), R.edge_profiles(ref, dis, bpc))
    if bpc == 12:
        assert 256 * top * top > 1 << 31 and 128 * top * top < 1 << 31 and 8192 * top * top > 1 << 36


def test_more_frames_than_one_staging_chunk():
    ref, dis = R.random_frames(9, 32, 48, seed=50), R.random_frames(9, 32, 48, seed=51)
    want = R.edge_profiles(ref, dis)
    assert len({want[0][f].tobytes() for f in range(9)}) == 9
    rbuf, _ = _padded(ref, pad=0, lead=0)
    dbuf, _ = _padded(dis, pad=0, lead=0)
    with _engine(48, 32) as eng:
        assert _equal(eng.edge_profiles(ref, dis), want)
        assert _equal(_resident(eng, rbuf, 0, dbuf, 0, 9, (32, 48)), want)
        assert _equal(eng.edge_profiles(ref[:2], dis[:2]), R.edge_profiles(ref[:2], dis[:2]))      # a shorter call after a longer one


@pytest.mark.parametrize("bpc", [8, 10])
def test_a_plane_size_other_than_the_contexts(bpc):
    """a 25 x 9 call and a 100 x 70 call on a 50 x 18 context, and row-sliced views"""
    with _engine(50, 18, bpc) as eng:
        for w, h in ((25, 9), (100, 70)):
            ref, dis = R.random_frames(2, h, w, bpc, seed=70 + w), R.random_frames(2, h, w, bpc, seed=71 + w)
            assert _equal(eng.edge_profiles(ref, dis), R.edge_profiles(ref, dis, bpc)), (w, h)
        ref, dis = R.random_frames(3, 18, 50, bpc, seed=80), R.random_frames(3, 18, 50, bpc, seed=81)
        cut_r, cut_d = [f[3:14] for f in ref], [f[3:14] for f in dis]
        assert not cut_r[0].flags["OWNDATA"] and cut_r[0].shape == (11, 50)
        want = R.edge_profiles(cut_r, cut_d, bpc)
        assert _equal(eng.edge_profiles(cut_r, cut_d), want)
        assert _equal(eng.edge_profiles(cut_r, cut_d, shape=(11, 50)), want)
        with pytest.raises(ValueError):
            eng.edge_profiles(cut_r, cut_d, shape=(18, 50))


def test_independent_of_the_scoring_chain():
    from pqa2_amd import _native as N
    rng = np.random.default_rng(7)
    ref = [rng.integers(0, 256, (48, 64)).astype(np.uint8) for _ in range(6)]
    dis = [np.clip(r.astype(int) + rng.integers(-9, 10, r.shape), 0, 255).astype(np.uint8) for r in ref]
    other_r, other_d = R.random_frames(2, 30, 100, seed=8), R.random_frames(2, 30, 100, seed=9)

    def run(with_call):
        with _engine(64, 48, features=N.FEAT_VMAF | N.FEAT_PSNR | N.FEAT_SSIM, max_batch=4) as eng:
            got = []
            for i in range(6):
                eng.submit(i, [ref[i]], [dis[i]])
                if with_call and i in (0, 2, 4):    # inside a pending batch, and right after one was launched
                    got.append(eng.edge_profiles(ref, dis))
                    got.append(eng.edge_profiles(other_r, other_d))
            return eng.collect(0, 6), got
    plain, _ = run(False)
    mixed, got = run(True)
    assert np.array_equal(plain.view(np.uint64), mixed.view(np.uint64))
    assert len(got) == 6
    assert all(_equal(g, R.edge_profiles(ref, dis)) for g in got[0::2])
    assert all(_equal(g, R.edge_profiles(other_r, other_d)) for g in got[1::2])
