"""The premises of the overlay mask, on the CPU: what tests/mask_ref.py (the restatement the GPU tests compare against) must
have for the blend to be what include/pqa_vmaf.h promises, and the two grid builders of pqa2_amd/distortion.py against their
restatement."""
import numpy as np
import pytest

from tests import mask_ref as MR

DEPTHS = (8, 10, 12)
STEPS = ((0, 0), (1, 2), (3, 3), (2, 3), (6, 6))


def _dt(bits):
    return np.uint8 if bits == 8 else np.uint16


# ---- alpha and the blend -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", DEPTHS)
def test_zero_is_the_identity_and_full_is_the_fill(bits):
    top = (1 << bits) - 1
    w, h = 37, 21
    rng = np.random.default_rng(bits)
    src = rng.integers(0, top + 1, (h, w)).astype(_dt(bits))
    src[0, :4] = (0, top, 1, top - 1)
    plane = rng.integers(0, top + 1, (h, w)).astype(_dt(bits))
    plane[0, :4] = (top, 0, top, 0)
    for steps in STEPS:
        shape = MR.grid_shape(w, h, *steps)
        for fill in (0, top, 1 << (bits - 1), plane):
            assert np.array_equal(MR.blend(src, np.zeros(shape, np.uint16), *steps, fill, bits), src)
            full = MR.blend(src, np.full(shape, 256, np.uint16), *steps, fill, bits)
            assert np.array_equal(full, np.broadcast_to(np.asarray(fill, _dt(bits)), (h, w)))
        # every result lies between the source and the fill, at the sample extremes too
        nodes = MR.random_grid(rng, w, h, *steps)
        for fill in (0, top, plane):
            out = MR.blend(src, nodes, *steps, fill, bits).astype(np.int64)
            lo, hi = np.minimum(src, fill).astype(np.int64), np.maximum(src, fill).astype(np.int64)
            assert (out >= lo).all() and (out <= hi).all()


@pytest.mark.parametrize("steps", STEPS)
def test_alpha_lies_between_its_four_nodes(steps):
    w, h = (3 << steps[0]) + 1, (2 << steps[1]) + 3
    A = MR.random_grid(np.random.default_rng(sum(steps)), w, h, *steps).astype(np.int64)
    a = MR.alpha(A, w, h, *steps)
    y, x = np.mgrid[0:h, 0:w]
    i, j = x >> steps[0], y >> steps[1]
    four = np.stack([A[j, i], A[j, i + 1], A[j + 1, i], A[j + 1, i + 1]])
    assert (a >= four.min(axis=0)).all() and (a <= four.max(axis=0)).all() and a.min() >= 0 and a.max() <= 256


@pytest.mark.parametrize("steps", STEPS)
def test_alpha_is_continuous_across_cells(steps):
    """on a node column (fx = 0) alpha is the vertical interpolation of that column alone, whichever cell the sample is counted
    to; on a node (fx = fy = 0) it is the node"""
    sx, sy = steps
    Gx, Gy = 1 << sx, 1 << sy
    w, h = 3 * Gx + 1, 3 * Gy + 1
    A = MR.random_grid(np.random.default_rng(7 + sx), w, h, sx, sy).astype(np.int64)
    a = MR.alpha(A, w, h, sx, sy)
    for x in range(0, w, Gx):
        for y in range(h):
            j, fy = y >> sy, y & (Gy - 1)
            assert a[y, x] == (A[j, x >> sx] * (Gy - fy) * Gx + A[j + 1, x >> sx] * fy * Gx + ((Gx * Gy) >> 1)) >> (sx + sy)
    assert np.array_equal(a[::Gy, ::Gx], A[:a[::Gy, ::Gx].shape[0], :a[::Gy, ::Gx].shape[1]])
    # a step across a cell border moves alpha no further than a step inside a cell can: the slope is bounded by the nodes
    if Gx > 1:
        assert np.abs(np.diff(a, axis=1)).max() <= -(-256 // Gx) + 1


# ---- the builders ------------------------------------------------------------------------------------------------------------
CASES = (   # width, height, tile, node, feather, grow
    (320, 180, 16, 8, 16, 1), (100, 70, 16, 4, 16, 0), (65, 33, 32, 8, 0, 1), (64, 64, 16, 16, 48, 2), (47, 29, 8, 8, 24, 1),
    (90, 50, 16, 8, 8, 0))


@pytest.mark.parametrize("case", CASES)
def test_overlay_mask_against_the_restatement(case):
    from pqa2_amd import distortion as D
    w, h, tile, node, feather, grow = case
    ty, tx = -(-h // tile), -(-w // tile)
    rng = np.random.default_rng(w + h)
    for density in (0.0, 0.08, 0.5, 1.0):
        t = rng.random((ty, tx)) < density
        if density == 0.08:
            t[-1, -1] = True      # a partial last tile, where the plane is no multiple of the tile
        m = D.overlay_mask(t, w, h, tile, grow=grow, feather=feather, node=node)
        s = m["step_log2"]
        assert 1 << s == node and m["nodes"].dtype == np.uint16
        assert np.array_equal(m["nodes"], MR.overlay_nodes(t, w, h, tile, grow, feather, node))
        a = MR.alpha(m["nodes"], w, h, s, s)
        grown = MR._grown(t, grow)
        px = np.kron(grown, np.ones((tile, tile), bool))[:h, :w]
        assert (a[px] == 256).all()                                    # every sample of a masked tile
        reach = max(feather, node) if grown.any() else 0               # alpha = 0 beyond the feather (a hard edge ramps inside one node step)
        far = ~np.kron(MR._grown(grown, -(-reach // tile)), np.ones((tile, tile), bool))[:h, :w]
        yy, xx = np.nonzero(px)
        if len(yy):
            ys, xs = np.nonzero(a)
            assert ys.min() > yy.min() - reach and ys.max() <= yy.max() + reach and xs.min() > xx.min() - reach and xs.max() <= xx.max() + reach
        assert not a[far].any()
        assert m["share"] == np.count_nonzero(a) / (w * h)
        assert m["bounds"] == MR.bounds(m["nodes"], w, h, s, s)
        if m["bounds"]:
            x0, y0, x1, y1 = m["bounds"]
            outside = np.ones((h, w), bool)
            outside[y0:y1, x0:x1] = False
            assert not a[outside].any()
        else:
            assert not grown.any() and m["share"] == 0 and m["boxes"] == []
        covered = np.zeros((h, w), bool)
        for x0, y0, x1, y1 in m["boxes"]:
            assert 0 <= x0 < x1 <= w and 0 <= y0 < y1 <= h and px[y0:y1, x0:x1].any()
            covered[y0:y1, x0:x1] = True
        assert covered[px].all()                                       # the boxes hold every masked tile


def test_mask_touching_every_edge():
    from pqa2_amd import distortion as D
    w, h, tile = 50, 35, 16      # partial last tiles both ways
    t = np.ones((3, 4), bool)
    m = D.overlay_mask(t, w, h, tile, grow=1, feather=16, node=8)
    assert (m["nodes"] == 256).all() and m["share"] == 1.0 and m["bounds"] == [0, 0, w, h] and m["boxes"] == [[0, 0, w, h]]
    ring = np.ones((3, 4), bool)
    ring[1, 1:3] = False
    m = D.overlay_mask(ring, w, h, tile, grow=0, feather=0, node=8)
    a = MR.alpha(m["nodes"], w, h, 3, 3)
    assert (a[0] == 256).all() and (a[-1] == 256).all() and (a[:, 0] == 256).all() and (a[:, -1] == 256).all()
    assert a[24, 24] == 0 and a[24, 40] == 0 and m["bounds"] == [0, 0, w, h]


def test_chroma_grids_agree_with_the_luma_grid():
    """a chroma sample under the shared grid at step_log2 - shift sees the alpha of the luma sample it sits on"""
    from pqa2_amd import distortion as D
    for w, h in ((320, 180), (75, 41)):
        t = np.zeros((-(-h // 16), -(-w // 16)), bool)
        t[1, 2] = t[-1, -1] = True
        for hs, vs in ((1, 1), (1, 0), (0, 0)):
            m = D.overlay_mask(t, w, h, 16, chroma_shift=(hs, vs))
            s = m["step_log2"]
            cw, ch = (w + (1 << hs) - 1) >> hs, (h + (1 << vs) - 1) >> vs
            assert m["nodes"].shape == MR.grid_shape(cw, ch, s - hs, s - vs)
            luma, chroma = MR.alpha(m["nodes"], w, h, s, s), MR.alpha(m["nodes"], cw, ch, s - hs, s - vs)
            assert np.array_equal(chroma[:luma[::1 << vs, ::1 << hs].shape[0], :luma[::1 << vs, ::1 << hs].shape[1]], luma[::1 << vs, ::1 << hs])
    with pytest.raises(ValueError, match="chroma"):
        D.overlay_mask(np.zeros((2, 2), bool), 4, 4, 2, node=1, feather=0, chroma_shift=(1, 1))
    with pytest.raises(ValueError, match="chroma"):
        D.overlay_mask_from_boxes([[0, 0, 2, 2]], 4, 4, node=1, feather=0, chroma_shift=(0, 1))


def test_builder_argument_errors():
    from pqa2_amd import distortion as D
    t = np.zeros((2, 2), bool)
    for kw in (dict(node=3), dict(node=128), dict(node=0), dict(feather=12), dict(feather=-8), dict(grow=-1)):
        with pytest.raises(ValueError):
            D.overlay_mask(t, 32, 32, 16, **kw)
    with pytest.raises(ValueError, match="multiple"):
        D.overlay_mask(np.zeros((3, 3), bool), 32, 32, 12, node=8)
    with pytest.raises(ValueError, match="disagree"):
        D.overlay_mask(np.zeros((3, 2), bool), 32, 32, 16)
    for box in ([0, 0, 0, 4], [4, 4, 2, 8], [0, 0, 40, 8], [-1, 0, 8, 8], [0, 0, 8]):
        with pytest.raises(ValueError):
            D.overlay_mask_from_boxes([box], 32, 32)


def test_boxes_snap_outward():
    from pqa2_amd import distortion as D
    w, h = 320, 180
    m = D.overlay_mask_from_boxes([list(MR.LOGO_BOX), [0, 0, 1, 1], [313, 170, 320, 180]], w, h)
    ref, snapped = MR.box_nodes([MR.LOGO_BOX, (0, 0, 1, 1), (313, 170, 320, 180)], w, h)
    assert np.array_equal(m["nodes"], ref)
    assert m["boxes"] == snapped == [[216, 120, 288, 160], [0, 0, 8, 8], [312, 168, 320, 180]]
    a = MR.alpha(m["nodes"], w, h, 3, 3)
    for x0, y0, x1, y1 in m["boxes"]:
        assert (a[y0:y1, x0:x1] == 256).all()
    assert m["share"] == np.count_nonzero(a) / (w * h) and m["bounds"] == MR.bounds(m["nodes"], w, h, 3, 3)
    already = D.overlay_mask_from_boxes([[192, 96, 304, 176]], w, h)
    assert already["boxes"] == [[192, 96, 304, 176]]
    hard = D.overlay_mask_from_boxes([[192, 96, 304, 176]], w, h, feather=0)
    assert set(np.unique(hard["nodes"])) == {0, 256} and hard["share"] < already["share"]
