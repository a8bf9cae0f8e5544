"""The line profiles on the MI355X (csrc/line_profiles.hip, pqa_line_profiles / pqa_line_profiles_device): row and column sums
and sums of squares equal the numpy restatement (tests/profile_ref.py) as integers -- smallest calls and argument rules, row
tails / pitches / odd base addresses at 8 / 10 / 12 bit, the seams of the kernel's column stripe and row band, the accumulator
limits on flat frames and the clamp, more frames than a staging chunk, a plane size other than the context's; the calls leave
the scoring chain alone."""
import ctypes as C

import numpy as np
import pytest

from tests import profile_ref as R

pytestmark = pytest.mark.gpu

STRIPE, BAND = 1024, 64      # kProfStripe, kProfBand of csrc/kernels.h: the columns and rows one workgroup reads


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


def _resident(eng, buf, lead, n, shape):
    import torch
    t = torch.from_numpy(buf.view(np.uint8).reshape(-1)).cuda()
    torch.cuda.synchronize()
    return eng.line_profiles_resident(t.data_ptr() + lead * buf.dtype.itemsize, buf.strides[1], buf.strides[0], shape, n)


def _equal(got, want):
    return all(g.dtype == np.uint64 and g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))


def test_the_binding_states_the_kernels_constants():
    import os
    import re
    from pqa2_amd import _native as N
    src = open(os.path.join(os.path.dirname(N.LIB_PATH), "kernels.h")).read()
    assert int(re.search(r"kProfStripe\s*=\s*(\d+)", src).group(1)) == STRIPE == N.PROFILE_STRIPE
    assert int(re.search(r"kProfBand\s*=\s*(\d+)", src).group(1)) == BAND == N.PROFILE_BAND


@pytest.mark.parametrize("bpc", [8, 10])
def test_smallest_calls_and_argument_rules(bpc):
    from pqa2_amd import _native as N
    frames = R.random_frames(bpc, 2, 16, 16, bpc)
    with _engine(16, 16, bpc) as eng:
        got = eng.line_profiles(frames)
        assert got[0].shape == (2, 16, 2) and got[1].shape == (2, 16, 2) and _equal(got, R.line_profiles(frames, bpc))
        for w, h in ((1, 1), (9, 1), (1, 9)):
            small = R.random_frames(3 + w + h, 2, w, h, bpc)
            assert _equal(eng.line_profiles(small), R.line_profiles(small, bpc)), (w, h)
        rows, cols = eng.line_profiles([])
        assert rows.shape == (0, 16, 2) and cols.shape == (0, 16, 2)
        rows, cols = eng.line_profiles_resident(0, 16 * frames[0].itemsize, 256 * frames[0].itemsize, (16, 16), 0)
        assert rows.shape == (0, 16, 2) and cols.shape == (0, 16, 2)

        es = frames[0].itemsize
        sp = eng._profile_spec((16, 16))
        out = np.zeros((2, 32, 2), np.uint64)
        keep, ptrs, stride = eng._luma_list(frames, "profile", (16, 16))
        lib, ctx = eng.lib, eng._ctx

        def spec(**kw):
            s = eng._profile_spec((kw.pop("height", 16), kw.pop("width", 16)))
            for k, v in kw.items():
                setattr(s, k, v)
            return C.byref(s)
        null_frame = (C.c_void_p * 2)(ptrs[0], None)
        dev = 4096      # never dereferenced: every call below is refused before any device call
        calls = {
            "null spec": lambda: lib.pqa_line_profiles(ctx, None, ptrs, stride, 2, out.ctypes.data),
            "null frame list": lambda: lib.pqa_line_profiles(ctx, C.byref(sp), None, stride, 2, out.ctypes.data),
            "null frame": lambda: lib.pqa_line_profiles(ctx, C.byref(sp), null_frame, stride, 2, out.ctypes.data),
            "null output": lambda: lib.pqa_line_profiles(ctx, C.byref(sp), ptrs, stride, 2, None),
            "null clip": lambda: lib.pqa_line_profiles_device(ctx, C.byref(sp), None, 16 * es, 256 * es, 2, out.ctypes.data),
            "null output, device": lambda: lib.pqa_line_profiles_device(ctx, C.byref(sp), dev, 16 * es, 256 * es, 2, None),
            "struct_size": lambda: lib.pqa_line_profiles(ctx, spec(struct_size=8), ptrs, stride, 2, out.ctypes.data),
            "width 0": lambda: lib.pqa_line_profiles(ctx, spec(width=0), ptrs, stride, 2, out.ctypes.data),
            "height 0": lambda: lib.pqa_line_profiles(ctx, spec(height=0), ptrs, stride, 2, out.ctypes.data),
            "width 8193": lambda: lib.pqa_line_profiles(ctx, spec(width=8193), ptrs, 8193 * es, 2, out.ctypes.data),
            "height 8193": lambda: lib.pqa_line_profiles_device(ctx, spec(height=8193), dev, 16 * es, 256 * es, 2, out.ctypes.data),
            "short stride": lambda: lib.pqa_line_profiles(ctx, C.byref(sp), ptrs, 16 * es - 1, 2, out.ctypes.data),
            "negative stride": lambda: lib.pqa_line_profiles(ctx, C.byref(sp), ptrs, -16 * es, 2, out.ctypes.data),
            "short pitch": lambda: lib.pqa_line_profiles_device(ctx, C.byref(sp), dev, 15 * es, 256 * es, 2, out.ctypes.data),
            "negative frame count": lambda: lib.pqa_line_profiles(ctx, C.byref(sp), ptrs, stride, -1, out.ctypes.data),
            "negative frame count, device": lambda: lib.pqa_line_profiles_device(ctx, C.byref(sp), dev, 16 * es, 256 * es, -1, out.ctypes.data),
        }
        if es == 2:      # a pitch that is no multiple of the sample size
            calls["odd row pitch"] = lambda: lib.pqa_line_profiles_device(ctx, C.byref(sp), dev, 33, 512, 2, out.ctypes.data)
            calls["odd frame pitch"] = lambda: lib.pqa_line_profiles_device(ctx, C.byref(sp), dev, 32, 513, 2, out.ctypes.data)
        for name, call in calls.items():
            assert call() == N.PQA_EINVAL, name
            assert _equal(eng.line_profiles(frames), got), name      # a refused call leaves the context usable
        assert not out.any()
        del keep
        with pytest.raises(ValueError):
            eng.line_profiles([frames[0], frames[1][:8]])      # planes of two sizes


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_tails_pitches_and_depths(bpc):
    """50 x 18: a row is no whole number of 16-byte loads; rows padded by 5 samples, base one sample in (the per-sample
    path); the host entry on contiguous frames, on views, and the resident entry agree; one 64-byte-aligned layout with a
    row tail (the 16-byte loads) and one 4-byte-aligned one (the word loads)"""
    frames = R.random_frames(10 + bpc, 3, 50, 18, bpc)
    want = R.line_profiles(frames, bpc)
    buf, views = _padded(frames)
    with _engine(50, 18, bpc) as eng:
        assert _equal(eng.line_profiles(frames), want)
        assert _equal(eng.line_profiles(views), want)
        assert _equal(_resident(eng, buf, 1, 3, (18, 50)), want)
        abuf, _ = _padded(frames, pad=14, lead=0)      # 64-byte rows at 8 bit, 128-byte rows at 16
        assert _equal(_resident(eng, abuf, 0, 3, (18, 50)), want)
        cbuf, _ = _padded(frames, pad=6, lead=4)       # 56-sample rows, base 4 samples in: 4-byte but not 16-byte aligned
        assert _equal(_resident(eng, cbuf, 4, 3, (18, 50)), want)


@pytest.mark.parametrize("bpc,lead", [(8, 0), (8, 1), (10, 0), (10, 2)])
def test_seams_of_stripe_and_band(bpc, lead):
    """a width one sample past the column stripe and a height one row past the row band: two stripes and two bands.  Black
    frames with one bright pixel on each side of each seam: a dropped or doubled line shows in exactly one sum.  lead 0: the
    16-byte loads; otherwise the resident clip starts `lead` samples into its buffer (the per-sample path at 8 bit, the word
    loads at 10)"""
    w, h, top = STRIPE + 1, BAND + 1, (1 << bpc) - 1
    spots = [(BAND - 1, STRIPE - 1), (BAND - 1, STRIPE), (BAND, STRIPE - 1), (BAND, STRIPE), (0, 0), (h - 1, w - 1), (BAND - 1, 0),
             (BAND, 7), (5, STRIPE - 1), (9, STRIPE)]
    frames = []
    for y, x in spots:
        f = np.zeros((h, w), _dt(bpc))
        f[y, x] = top - (y + x) % 7
        frames.append(f)
    frames.append(R.random_frames(60 + bpc, 1, w, h, bpc)[0])
    want = R.line_profiles(frames, bpc)
    for f, (y, x) in zip(range(len(spots)), spots):      # the reference itself: one row and one column are not zero
        assert np.flatnonzero(want[0][f, :, 0]).tolist() == [y] and np.flatnonzero(want[1][f, :, 0]).tolist() == [x]
    buf, views = _padded(frames, pad=(16 - w % 16) % 16 if lead == 0 else 5, lead=lead)
    with _engine(64, 64, bpc) as eng:
        assert _equal(eng.line_profiles(frames), want)
        assert _equal(_resident(eng, buf, lead, len(frames), (h, w)), want)


@pytest.mark.parametrize("bpc,w,h", [(8, 8192, 3), (8, 3, 8192), (12, 8192, 3), (12, 3, 8192)])
def test_accumulator_limits_on_flat_frames(bpc, w, h):
    """flat frames of the maximum: a line of 8192 samples of 4095 sums to 137 371 852 800 > 2^37 in its squares, past 32 bits in
    the column registers after 256 rows and in a wave's row sum after 256 samples; at 12 bit also a frame of 0xFFFF samples
    in the 16-bit container, read as 4095"""
    top = (1 << bpc) - 1
    full = np.full((h, w), top, _dt(bpc))
    frames = [full] + ([np.full((h, w), 0xFFFF, np.uint16)] if bpc == 12 else [])
    with _engine(64, 64, bpc) as eng:
        rows, cols = eng.line_profiles(frames)
    for f in range(len(frames)):
        assert (rows[f, :, 0] == w * top).all() and (rows[f, :, 1] == w * top * top).all()
        assert (cols[f, :, 0] == h * top).all() and (cols[f, :, 1] == h * top * top).all()
    assert _equal((rows, cols), R.line_profiles(frames, bpc))
    if bpc == 12:
        assert 8192 * top * top > 1 << 36


def test_more_frames_than_one_staging_chunk():
    frames = R.random_frames(50, 9, 48, 32)
    want = R.line_profiles(frames)
    assert len({want[0][f].tobytes() for f in range(9)}) == 9
    buf, _ = _padded(frames, pad=0, lead=0)
    with _engine(48, 32) as eng:
        assert _equal(eng.line_profiles(frames), want)
        assert _equal(_resident(eng, buf, 0, 9, (32, 48)), want)
        assert _equal(eng.line_profiles(frames[:2]), R.line_profiles(frames[:2]))      # a shorter call after a longer one


@pytest.mark.parametrize("bpc", [8, 10])
def test_a_plane_size_other_than_the_contexts(bpc):
    """a 25 x 9 call and a 100 x 70 call on a 50 x 18 context, and row-sliced views: the second pass of the solver"""
    with _engine(50, 18, bpc) as eng:
        for w, h in ((25, 9), (100, 70)):
            frames = R.random_frames(70 + w, 2, w, h, bpc)
            assert _equal(eng.line_profiles(frames), R.line_profiles(frames, bpc)), (w, h)
        frames = R.random_frames(80, 3, 50, 18, bpc)
        cut = [f[3:14] for f in frames]
        assert not cut[0].flags["OWNDATA"] and cut[0].shape == (11, 50)
        want = R.line_profiles(cut, bpc)
        assert _equal(eng.line_profiles(cut), want)
        assert np.array_equal(eng.line_profiles(cut, shape=(11, 50))[1], R.cols_of(frames, bpc)(3, 4))
        with pytest.raises(ValueError):
            eng.line_profiles(cut, shape=(18, 50))


def test_independent_of_the_scoring_chain():
    from pqa2_amd import _native as N
    rng = np.random.default_rng(7)
    ref = [rng.integers(0, 256, (48, 64)).astype(np.uint8) for _ in range(6)]
    dis = [np.clip(r.astype(int) + rng.integers(-9, 10, r.shape), 0, 255).astype(np.uint8) for r in ref]
    other = R.random_frames(8, 2, 100, 30)

    def run(with_call):
        with _engine(64, 48, features=N.FEAT_VMAF | N.FEAT_PSNR | N.FEAT_SSIM, max_batch=4) as eng:
            got = []
            for i in range(6):
                eng.submit(i, [ref[i]], [dis[i]])
                if with_call and i in (0, 2, 4):    # inside a pending batch, and right after one was launched
                    got.append(eng.line_profiles(dis))
                    got.append(eng.line_profiles(other))
            return eng.collect(0, 6), got
    plain, _ = run(False)
    mixed, got = run(True)
    assert np.array_equal(plain.view(np.uint64), mixed.view(np.uint64))
    assert len(got) == 6
    assert all(_equal(g, R.line_profiles(dis)) for g in got[0::2]) and all(_equal(g, R.line_profiles(other)) for g in got[1::2])
