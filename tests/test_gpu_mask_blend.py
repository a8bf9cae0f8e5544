"""The mask blend on the MI355X (csrc/mask_blend.hip, pqa_mask_blend / pqa_mask_blend_device) against tests/mask_ref.py:
equality, no tolerance, everywhere.  A lane owns 16 bytes of a row -- 16 samples at 8 bit, 8 otherwise -- and stores them whole
only when they lie inside the row, so the widths are a single sample, end one short of, on and one past a lane's span (15, 16,
17; 31, 33), end inside one (50) and take several lanes and a tail (257); 1030 x 19 passes a wave's 64 lanes in a row (a second
tile of items) and a workgroup's 16 rows (8 at step 0).  The node grids are random with forced runs of 0 and of 256, so the
copied, the filled and the blended items all occur, next to the grids that are all one of them.  On the parent commit there is
no FeatureEngine.mask_blend."""
import ctypes as C

import numpy as np
import pytest

from tests import mask_ref as MR

pytestmark = pytest.mark.gpu

DEPTHS = (8, 10, 12)
STEPS = ((0, 0), (1, 2), (3, 3), (2, 3), (6, 6))
WIDTHS = (1, 15, 16, 17, 31, 33, 50, 257)
HEIGHTS = (1, 2, 9, 19)
SENTINEL = 0xA5


def _dt(bits):
    return np.uint8 if bits == 8 else np.uint16


@pytest.fixture(scope="module")
def engs():
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    made = {b: FeatureEngine(64, 48, bit_depth=b, n_planes=1, features=N.FEAT_PSNR) for b in DEPTHS}   # the size does not matter (plane=None)
    yield made
    for e in made.values():
        e.close()


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


def _lay(planes, pad, lead, spare_rows):
    """(bytes, row pitch, frame pitch) of planes laid out with rows `pad` samples longer than a row, the base `lead` samples
    in and `spare_rows` rows between the frames, the sentinel everywhere else"""
    es = planes[0].dtype.itemsize
    n, (h, w) = len(planes), planes[0].shape
    pitch = (w + pad) * es
    fp = (h + spare_rows) * pitch
    buf = np.full(lead * es + n * fp, SENTINEL, np.uint8)
    for f, p in enumerate(planes):
        rows = buf[lead * es + f * fp:lead * es + f * fp + h * pitch].reshape(h, pitch)
        rows[:, :w * es] = np.ascontiguousarray(p).view(np.uint8).reshape(h, w * es)
    return buf, pitch, fp


def _device(eng, planes, nodes, steps, fill, pad=3, lead=1, in_place=False, spare_rows=1, fill_pad=5, fill_lead=2):
    """through pqa_mask_blend_device.  fill: an integer, or a list of planes, which get a layout of their own.  Returns the
    planes; every destination byte outside the rows' samples must have kept the sentinel, and what is only read its bytes."""
    import torch
    es = planes[0].dtype.itemsize
    n, (h, w) = len(planes), planes[0].shape
    sbuf, pitch, fp = _lay(planes, pad, lead, spare_rows)
    ts = torch.from_numpy(sbuf).cuda()
    td = ts if in_place else torch.full((sbuf.size,), SENTINEL, dtype=torch.uint8, device="cuda")
    kw, tf = {}, None
    if not isinstance(fill, int):
        fbuf, fpitch, ffp = _lay(fill, fill_pad, fill_lead, 0)
        tf = torch.from_numpy(fbuf).cuda()
        kw = dict(fill_ptr=tf.data_ptr() + fill_lead * es, fill_row_pitch=fpitch, fill_frame_pitch=ffp)
    torch.cuda.synchronize()
    eng.mask_blend_resident(nodes, steps, fill if isinstance(fill, int) else 0, (h, w), ts.data_ptr() + lead * es, pitch, fp,
                            td.data_ptr() + lead * es, pitch, fp, n, **kw)
    raw = td.cpu().numpy()
    assert (raw[:lead * es] == SENTINEL).all()
    out = raw[lead * es:].reshape(n, h + spare_rows, pitch)
    assert (out[:, :h, w * es:] == SENTINEL).all() and (out[:, h:, :] == SENTINEL).all(), (w, h, pad, lead)
    if not in_place:     # the source is only read
        assert np.array_equal(ts.cpu().numpy(), sbuf)
    if tf is not None:   # and so is the fill plane
        assert np.array_equal(tf.cpu().numpy(), fbuf)
    return [np.ascontiguousarray(out[f, :h, :w * es]).view(planes[0].dtype).reshape(h, w) for f in range(n)]


def _check_all(eng, bits, planes, nodes, steps, fill, tag):
    """host entry, device entry not in place and in place, against the restatement"""
    want = [MR.blend(p, nodes, *steps, fill if isinstance(fill, int) else fill[f], bits) for f, p in enumerate(planes)]
    for name, got in (("host", eng.mask_blend(planes, nodes, steps, fill, plane=None)),
                      ("device", _device(eng, planes, nodes, steps, fill)),
                      ("in place", _device(eng, planes, nodes, steps, fill, in_place=True)),
                      ("aligned", _device(eng, planes, nodes, steps, fill, pad=(-planes[0].shape[1]) % 16, lead=0, fill_pad=(-planes[0].shape[1]) % 16, fill_lead=0))):
        for f, (g, x) in enumerate(zip(got, want)):
            assert g.dtype == x.dtype and np.array_equal(g, x), (tag, name, f, np.argwhere(g != x)[:4].tolist())
    return want


# ---- the smallest call and the argument rules ------------------------------------------------------------------------------
def test_smallest_call_and_no_frames(engs):
    for bits in DEPTHS:
        eng, top = engs[bits], (1 << bits) - 1
        for a, want in ((0, 5), (256, top), (128, (5 * 128 + top * 128 + 128) >> 8)):
            nodes = np.full((2, 2), a, np.uint16)
            got = eng.mask_blend([np.full((1, 1), 5, _dt(bits))], nodes, (3, 3), top, plane=None)
            assert len(got) == 1 and got[0].shape == (1, 1) and got[0].dtype == _dt(bits) and got[0][0, 0] == want
            assert _device(eng, [np.full((1, 1), 5, _dt(bits))], nodes, (3, 3), top)[0][0, 0] == want
        assert eng.mask_blend([], np.zeros((7, 9), np.uint16), (3, 3), 0, plane=None) == []
        eng.mask_blend_resident(np.zeros((2, 2), np.uint16), (3, 3), 0, (4, 4), 0, 8, 32, 0, 8, 32, 0)   # no frames: nothing is touched
    got = engs[8].mask_blend([np.zeros((48, 64), np.uint8)], np.full((7, 9), 256, np.uint16), (3, 3), 9)   # plane=0: the context's luma size
    assert got[0].shape == (48, 64) and (got[0] == 9).all()
    with pytest.raises(ValueError):
        engs[8].mask_blend([np.zeros((4, 4), np.uint8)], np.zeros((7, 9), np.uint16), (3, 3), 0)
    with pytest.raises(ValueError):   # a grid of the wrong size
        engs[8].mask_blend([np.zeros((4, 4), np.uint8)], np.zeros((3, 2), np.uint16), (3, 3), 0, plane=None)
    with pytest.raises(ValueError):   # fewer fill planes than frames
        engs[8].mask_blend([np.zeros((4, 4), np.uint8)] * 2, np.zeros((2, 2), np.uint16), (3, 3), [np.zeros((4, 4), np.uint8)], plane=None)


@pytest.mark.parametrize("bits", [8, 10])
def test_argument_rules(engs, bits):
    import torch
    from pqa2_amd import _native as N
    eng, es = engs[bits], (1 if bits == 8 else 2)
    w, h = 18, 10
    row = w * es
    buf = torch.zeros(3 << 12, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    q, fl = p + 4096, p + 8192
    nodes = np.zeros(MR.grid_shape(w, h, 3, 3), np.uint16)
    gp = nodes.ctypes.data

    def spec(**kw):
        sp = eng._plane_spec(N.PqaMaskSpec, (h, w), step_log2_x=3, step_log2_y=3, fill=0)
        for k, v in kw.items():
            setattr(sp, k, v)
        return sp

    def refused(rc_call, word):
        with pytest.raises(N.PqaError) as e:
            eng._check(rc_call())
        assert e.value.code == N.PQA_EINVAL and word in str(e.value), str(e.value)

    dev = lambda sp, g=gp, s=p, srp=row, sfp=row * h, f=0, frp=row, ffp=row * h, d=q, drp=row, dfp=row * h, n=1: (
        lambda: eng.lib.pqa_mask_blend_device(eng._ctx, C.byref(sp) if sp is not None else None, g or None, s or None, srp, sfp, f or None,
                                              frp, ffp, d or None, drp, dfp, n))
    refused(dev(None), "null spec")
    refused(dev(spec(struct_size=12)), "struct_size")
    for k in ("width", "height"):
        for v in (0, 8193):
            refused(dev(spec(**{k: v})), "size")
    for k in ("step_log2_x", "step_log2_y"):
        refused(dev(spec(**{k: 7})), "steps")
    refused(dev(spec(fill=1 << bits)), "fill")
    refused(dev(spec(fill=1 << bits), f=fl), "fill")
    refused(dev(spec(), n=-1), "negative")
    refused(dev(spec(), g=0), "null node")
    refused(dev(spec(), s=0), "null")
    refused(dev(spec(), d=0), "null")
    refused(dev(spec(), srp=row - es), "source pitch")
    refused(dev(spec(), drp=row - es), "destination pitch")
    refused(dev(spec(), f=fl, frp=row - es), "fill pitch")
    refused(dev(spec(), f=q), "fill plane")
    for at, v in ((0, 257), (nodes.size - 1, 257), (5, 65535)):
        bad = nodes.copy()
        bad.reshape(-1)[at] = v
        refused(dev(spec(), g=bad.ctypes.data), "above 256")
        with pytest.raises(N.PqaError, match="above 256"):
            eng.mask_blend([np.zeros((h, w), _dt(bits))], bad, (3, 3), 0, plane=None)
    with pytest.raises(N.PqaError, match="uint16"):
        eng.mask_blend([np.zeros((h, w), _dt(bits))], nodes.astype(np.int64) + 65536, (3, 3), 0, plane=None)
    if es == 2:      # an odd device base or pitch at 16 bit
        refused(dev(spec(), srp=row + 1), "sample size")
        refused(dev(spec(), drp=row + 1), "sample size")
        refused(dev(spec(), sfp=row * h + 1), "sample size")
        refused(dev(spec(), dfp=row * h + 1), "sample size")
        refused(dev(spec(), s=p + 1), "sample size")
        refused(dev(spec(), d=q + 1), "sample size")
        refused(dev(spec(), f=fl + 1), "sample size")
        refused(dev(spec(), f=fl, frp=row + 1), "sample size")
        refused(dev(spec(), f=fl, ffp=row * h + 1), "sample size")
    # the host entry: a null list, a null frame, short rows, a destination that is its fill plane
    a, o, fp_ = np.zeros((h, w), _dt(bits)), np.zeros((h, w), _dt(bits)), np.zeros((h, w), _dt(bits))
    ptr = lambda arr: (C.c_void_p * 1)(arr.ctypes.data)
    sptr, dptr, fptr, null = ptr(a), ptr(o), ptr(fp_), (C.c_void_p * 1)(None)
    host = lambda sp, g=gp, s=sptr, ss=row, f=None, fs=row, d=dptr, ds=row, n=1: (
        lambda: eng.lib.pqa_mask_blend(eng._ctx, C.byref(sp), g or None, s, ss, f, fs, d, ds, n))
    refused(host(spec(), s=None), "null")
    refused(host(spec(), d=None), "null")
    refused(host(spec(), s=null), "null")
    refused(host(spec(), d=null), "null")
    refused(host(spec(), f=null), "null")
    refused(host(spec(), g=0), "null node")
    refused(host(spec(), ss=row - 1), "stride")
    refused(host(spec(), ds=row - 1), "stride")
    refused(host(spec(), f=fptr, fs=row - 1), "stride")
    refused(host(spec(), f=dptr), "fill plane")
    refused(host(spec(), n=-2), "negative")
    refused(host(spec(width=0)), "size")
    refused(host(spec(step_log2_x=9)), "steps")
    # nothing was written, and both entries work afterwards: a refused call leaves the context usable
    assert not o.any() and not buf.cpu().numpy().any()
    assert eng.lib.pqa_mask_blend_device(eng._ctx, C.byref(spec()), gp, None, row, row * h, None, 0, 0, None, row, row * h, 0) == 0
    full = np.full_like(nodes, 256)
    eng._check(host(spec(fill=7), g=full.ctypes.data)())
    assert (o == 7).all()
    eng._check(dev(spec())())


# ---- tails, pitches and depths -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", DEPTHS)
def test_widths_and_heights(engs, bits):
    """every width by every height, the steps taken in turn, constant fill and fill plane in turn"""
    eng, top = engs[bits], (1 << bits) - 1
    k = 0
    for w in WIDTHS:
        for h in HEIGHTS:
            steps = STEPS[k % len(STEPS)]
            rng = np.random.default_rng(1000 * w + h)
            nodes = MR.random_grid(rng, w, h, *steps)
            planes = _noise(w * 31 + h, bits, (h, w))
            fill = (0, top, 1 << (bits - 1))[k % 3] if k % 2 else _noise(w * 37 + h, bits, (h, w))
            _check_all(eng, bits, planes, nodes, steps, fill, (w, h, steps))
            k += 1


@pytest.mark.parametrize("steps", STEPS)
def test_steps_on_and_off_the_grid(engs, steps):
    """sizes that are multiples of the step, one past a multiple (the last node column and row are used), and neither"""
    Gx, Gy = 1 << steps[0], 1 << steps[1]
    for bits in DEPTHS:
        for w, h in ((2 * Gx + 1, 2 * Gy + 1), (3 * Gx, 2 * Gy), (max(2 * Gx - 3, 1), Gy + 2), (50, 19)):
            rng = np.random.default_rng(w * 100 + h + bits)
            nodes = MR.random_grid(rng, w, h, *steps)
            nodes[-1, :] = rng.integers(1, 257, nodes.shape[1])     # the last row and column count
            nodes[:, -1] = rng.integers(1, 257, nodes.shape[0])
            planes = _noise(w + h, bits, (h, w), n=1)
            _check_all(engs[bits], bits, planes, nodes, steps, (1 << bits) - 1, (bits, w, h, steps))
            _check_all(engs[bits], bits, planes, nodes, steps, _noise(w + h + 1, bits, (h, w), n=1), (bits, w, h, steps, "plane"))


@pytest.mark.parametrize("bits", DEPTHS)
def test_wide_plane_crosses_a_wave_and_a_workgroup(engs, bits):
    w, h = 1030, 19
    planes, fills = _noise(5, bits, (h, w)), _noise(6, bits, (h, w))
    for steps in ((3, 3), (0, 0), (2, 3)):
        nodes = MR.random_grid(np.random.default_rng(bits + steps[0]), w, h, *steps)
        _check_all(engs[bits], bits, planes, nodes, steps, fills, (bits, steps))
        _check_all(engs[bits], bits, planes, nodes, steps, 3, (bits, steps, "const"))


@pytest.mark.parametrize("bits", DEPTHS)
def test_uniform_grids_and_single_nodes(engs, bits):
    """a grid all 0 is the identity, one all 256 the fill, and a single node in a corner reaches its one cell"""
    eng, top = engs[bits], (1 << bits) - 1
    w, h, steps = 50, 19, (3, 2)
    shape = MR.grid_shape(w, h, *steps)
    planes, fills = _noise(8, bits, (h, w)), _noise(9, bits, (h, w))
    for fill in (0, top, fills):
        got = _check_all(eng, bits, planes, np.zeros(shape, np.uint16), steps, fill, "zeros")
        assert all(np.array_equal(g, p) for g, p in zip(got, planes))
        got = _check_all(eng, bits, planes, np.full(shape, 256, np.uint16), steps, fill, "full")
        assert all((g == fill).all() if isinstance(fill, int) else np.array_equal(g, fill[f]) for f, g in enumerate(got))
        for j, i in ((0, 0), (0, shape[1] - 1), (shape[0] - 1, 0), (shape[0] - 1, shape[1] - 1)):
            for v in (1, 200, 256):
                nodes = np.zeros(shape, np.uint16)
                nodes[j, i] = v
                _check_all(eng, bits, planes, nodes, steps, fill, ("corner", j, i, v))


def test_samples_above_the_depth(engs):
    """u16: where alpha > 0 a sample above top reads as top, source and fill alike; where alpha = 0 it is copied as it is"""
    for bits in (10, 12):
        w, h, steps = 40, 12, (2, 2)
        rng = np.random.default_rng(bits)
        planes = [rng.integers(0, 65536, (h, w)).astype(np.uint16)]
        fills = [rng.integers(0, 65536, (h, w)).astype(np.uint16)]
        nodes = MR.random_grid(rng, w, h, *steps)
        nodes[:, :3] = 0
        nodes[:, -3:] = 256
        got = _check_all(engs[bits], bits, planes, nodes, steps, fills, bits)
        a = MR.alpha(nodes, w, h, *steps)
        assert np.array_equal(got[0][a == 0], planes[0][a == 0]) and (got[0][a > 0] <= (1 << bits) - 1).all()


@pytest.mark.parametrize("bits", [8, 10])
def test_in_place_touches_the_bounds_only(engs, bits):
    """a few non-zero nodes inside a plane: in place everything outside the mask's bounds is the source still, not in place it
    is the source's copy; the bounds start inside an item, a cell and a tile of rows"""
    eng = engs[bits]
    w, h, steps = 257, 50, (3, 3)
    nodes = np.zeros(MR.grid_shape(w, h, *steps), np.uint16)
    nodes[2:5, 6:11] = np.random.default_rng(1).integers(1, 257, (3, 5))
    nodes[3, 8] = 256
    x0, y0, x1, y1 = MR.bounds(nodes, w, h, *steps)
    assert (x0, y0, x1, y1) == (41, 9, 88, 40)
    planes, fills = _noise(11, bits, (h, w), n=3), _noise(12, bits, (h, w), n=3)
    for fill in (1, fills):
        for in_place in (True, False):
            got = _device(eng, planes, nodes, steps, fill, in_place=in_place, pad=7, lead=0)
            for f, (g, p) in enumerate(zip(got, planes)):
                assert np.array_equal(g, MR.blend(p, nodes, *steps, fill if isinstance(fill, int) else fill[f], bits))
                outside = np.ones((h, w), bool)
                outside[y0:y1, x0:x1] = False
                assert np.array_equal(g[outside], p[outside]) and not np.array_equal(g, p)
    # a node grid whose non-zero nodes weigh on no sample: in place nothing is launched
    edge = np.zeros(MR.grid_shape(17, 9, 3, 3), np.uint16)      # the last node column lies at x = 24, behind the node at x = 16 = w - 1
    edge[:, -1] = 256
    assert MR.bounds(edge, 17, 9, 3, 3) is None
    small = _noise(13, bits, (9, 17), n=1)
    assert np.array_equal(_device(eng, small, edge, (3, 3), 0, in_place=True)[0], small[0])


@pytest.mark.parametrize("bits", [8, 10])
def test_nine_host_frames_cross_the_chunk(engs, bits):
    w, h, steps = 70, 21, (3, 3)
    planes, fills = _noise(21, bits, (h, w), n=9), _noise(22, bits, (h, w), n=9)
    nodes = MR.random_grid(np.random.default_rng(2), w, h, *steps)
    for fill in (4, fills):
        want = [MR.blend(p, nodes, *steps, fill if isinstance(fill, int) else fill[f], bits) for f, p in enumerate(planes)]
        keep = [p.copy() for p in planes]
        got = engs[bits].mask_blend(planes, nodes, steps, fill, plane=None)
        assert len(got) == 9 and all(np.array_equal(g, x) for g, x in zip(got, want))
        assert all(np.array_equal(p, k) for p, k in zip(planes, keep))
    # rows of a view: a stride that is no pitch of the staging
    buf = np.zeros((2, h, w + 5), _dt(bits))
    buf[:, :, 2:w + 2] = np.stack(planes[:2])
    got = engs[bits].mask_blend([buf[f, :, 2:w + 2] for f in range(2)], nodes, steps, 4, plane=None)
    assert all(np.array_equal(g, MR.blend(p, nodes, *steps, 4, bits)) for g, p in zip(got, planes))
