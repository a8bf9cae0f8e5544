"""Sub-pixel and scale registration without a GPU: the exact-fraction solver on hand-made moment tables, the Q16 window algebra,
the numpy restatement of the moments against its Python-int form, and align.register driven by the restatements
(tests/flow_ref.py, tests/resample_ref.py) on synthesised captures whose geometry is known."""
from fractions import Fraction

import numpy as np
import pytest

from pqa2_amd import align as AL
from tests import flow_ref as F
from tests import spatial_align_ref as S


def _table(width, height, tile, u, v, weight=lambda i, j: 1000 + 37 * i + 11 * j):
    """the moments of a picture whose every tile sees the displacement (u(px), v(py)) exactly: dt = -(gx u + gy v) with
    uncorrelated gradients, so sum gx dt = -u sum gx^2 and sum gy dt = -v sum gy^2"""
    cxs, cys = AL._tile_centres(width, tile), AL._tile_centres(height, tile)
    M = np.zeros((len(cys), len(cxs), 6), np.int64)
    for j, py in enumerate(cys):
        for i, px in enumerate(cxs):
            if px is None or py is None:
                continue
            g = weight(i, j) * 128        # keeps u * g integral for the u below (tile centres are half integers)
            gxt, gyt = -u(px) * g, -v(py) * 2 * g
            assert gxt.denominator == 1 and gyt.denominator == 1
            M[j, i] = (g, 0, 2 * g, int(gxt), int(gyt), 0)
    return M


def test_solver_recovers_a_pure_shift_and_a_pure_scale_exactly():
    shift = _table(96, 64, 16, lambda p: Fraction(3, 8), lambda p: Fraction(-5, 8))
    assert AL.solve_geometry(shift, 96, 64, 16) == (Fraction(3, 8), 0, Fraction(-5, 8), 0)
    scale = _table(96, 64, 16, lambda p: p * Fraction(1, 64), lambda p: p * Fraction(-1, 32))
    assert AL.solve_geometry(scale, 96, 64, 16) == (0, Fraction(1, 64), 0, Fraction(-1, 32))
    both = _table(100, 70, 8, lambda p: Fraction(1, 4) + p * Fraction(1, 32), lambda p: Fraction(-1, 2) + p * Fraction(1, 64))
    assert AL.solve_geometry(both, 100, 70, 8) == (Fraction(1, 4), Fraction(1, 32), Fraction(-1, 2), Fraction(1, 64))
    # the tile centres are those of the COUNTED pixels: the first tile of a 96-wide plane at T = 16 counts x = 1 ... 15
    assert AL._tile_centres(96, 16)[0] == Fraction(1 + 15 + 1, 2) - 48 and AL._tile_centres(96, 16)[-1] == Fraction(80 + 94 + 1, 2) - 48
    assert AL._tile_centres(65, 8)[-1] is None       # x = 64 is the last column: not counted


def test_solver_refuses_a_singular_table():
    assert AL.solve_geometry(np.zeros((4, 6, 6), np.int64), 96, 64, 16) is None                      # a flat picture
    one_col = _table(96, 64, 16, lambda p: Fraction(1, 2), lambda p: Fraction(0), weight=lambda i, j: 1000 if i == 2 else 0)
    assert AL.solve_geometry(one_col, 96, 64, 16) is None        # gradient in one tile column: no scale can be told
    one_row = _table(96, 64, 16, lambda p: Fraction(1, 2), lambda p: Fraction(0), weight=lambda i, j: 1000 if j == 1 else 0)
    assert AL.solve_geometry(one_row, 96, 64, 16) is None
    with pytest.raises(ValueError):
        AL.solve_geometry(np.zeros((4, 5, 6), np.int64), 96, 64, 16)


def test_window_algebra_is_exact_in_q16():
    for n, x0, w in ((192, -51793, 12735328), (128, -6707, 8322014), (1920, 0, 1920 * 65536), (35, 12345, 35 * 65536 - 777)):
        d, s = AL.window_geometry(x0, w, n)
        assert AL.geometry_window(d, s, n) == (x0, w)                       # window -> map -> window
        for a, e in ((Fraction(3, 7), Fraction(1, 90)), (Fraction(-5, 3), Fraction(-1, 33))):
            d1, s1 = AL.compose_geometry(d, s, a, e)
            assert (d1, s1) == (d + s * a, s * (1 + e))
            d2, s2 = AL.compose_geometry(d1, s1, -a / (1 + e), 1 / (1 + e) - 1)      # the inverse increment
            assert (d2, s2) == (d, s) and AL.geometry_window(d2, s2, n) == (x0, w)
    assert AL.geometry_window(0, 1, 640) == (0, 640 * 65536)
    assert AL.geometry_window(Fraction(1, 2), 1, 640) == (32768, 640 * 65536)
    assert AL.geometry_window(0, Fraction(101, 100), 100) == (-32768, 101 * 65536)   # 1 % larger: half a sample out on each side
    assert AL.register_levels(192, 128, 16, 1) == [(1, 16), (0, 16)]
    assert AL.register_levels(192, 128, 32, None) == [(2, 8), (1, 16), (0, 32)]
    assert AL.register_levels(1920, 1080, 32, None) == [(4, 16), (3, 32), (2, 32), (1, 32), (0, 32)]   # 120 x 67 at l = 4
    assert AL.register_levels(40, 40, 32, None) == [(0, 8)]


@pytest.mark.parametrize("bits,tile,w,h", [(8, 8, 19, 11), (10, 16, 35, 18), (12, 64, 67, 66)])
def test_restatement_equals_its_python_int_form(bits, tile, w, h):
    rng = np.random.default_rng(bits)
    dt = np.uint8 if bits == 8 else np.uint16
    ref, dis = (rng.integers(0, 1 << bits, (h, w)).astype(dt) for _ in range(2))
    assert F.moments([ref], [dis], tile, bits)[0].tolist() == F.moments_exact(ref, dis, tile, bits)


def test_restatement_at_the_accumulator_bounds():
    """a vertical step edge between 0 and 4095 in both planes under a constant difference of +-4095: gx = 8 * 4095 = 32 760
    beside the edge where dt = 16 * 4095 = 65 520, so gx^2, gx dt and dt^2 reach their bounds at the same pixels; 0xffff in
    the container reads as 4095"""
    top = 4095
    ref = np.zeros((64, 64), np.uint16)
    dis = np.full((64, 64), 0xffff, np.uint16)
    M = F.moments([ref], [dis], 64, 12)[0, 0, 0]
    assert M.tolist() == [0, 0, 0, 0, 0, 62 * 62 * (16 * top) ** 2] and F.moments_exact(ref, dis, 64, 12)[0][0] == M.tolist()
    edge = np.zeros((64, 64), np.uint16)
    edge[:, 32:] = top
    gx, gy, dtv = F._fields(edge, edge, 12)
    assert gx.max() == 8 * top and gy.max() == 0 and dtv.max() == 0


GEOMETRIES = {"first": (192, 128, (0.37, -0.61, 1.012, 0.992)), "second": (320, 192, (1.4, -0.8, 1.03, 1.03))}


def _pair(name, frames=2, noise=3):
    w, h, g = GEOMETRIES[name]
    ref = [f[0] for f in S.natural_planes(41, frames, w, h)]
    return ref, [F.capture(r, *g, noise=noise, seed=100 + i) for i, r in enumerate(ref)], g


@pytest.mark.parametrize("name,bar_px,bar_scale", [("first", (0.0050, 0.0008), (2.2e-4, 1.2e-4)), ("second", (0.0130, 0.0054), (5.4e-4, 4.7e-4))])
def test_register_recovers_a_known_geometry(name, bar_px, bar_scale):
    """Content natural_planes(41), two frames; capture: a Lanczos warp plus uniform noise of +-3; tile 16, one pyramid level,
    bicubic warps.  Measured with these restatements (errors in dx, dy / sx, sy):
        first  (192 x 128; 0.37, -0.61, 1.012, 0.992): 0.00254, 0.00041 px / 1.1e-4, 6e-5;   3 increments, converged
        second (320 x 192; 1.4, -0.8, 1.03, 1.03):     0.00654, 0.00274 px / 2.7e-4, 2.4e-4; 3 increments, converged
    The bars are twice those, rounded down."""
    ref, dis, g = _pair(name)
    out = AL.register(*F.restatements(8), ref, dis, filter="bicubic", tile=16, levels=1)
    err = [abs(out[k] - v) for k, v in zip(("dx", "dy", "sx", "sy"), g)]
    print(name, out, err)
    assert out["converged"] and out["levels"] == 1 and 1 <= out["iterations"] <= 2 * 5
    assert err[0] <= bar_px[0] and err[1] <= bar_px[1] and err[2] <= bar_scale[0] and err[3] <= bar_scale[1]
    assert out["mse_after"] < out["mse_before"] / 10 and AL.geometry_applied(out)
    w, h = GEOMETRIES[name][:2]
    dx, sx = AL.window_geometry(out["x0_q16"], out["w_q16"], w)
    dy, sy = AL.window_geometry(out["y0_q16"], out["h_q16"], h)
    assert [float(v) for v in (dx, dy, sx, sy)] == [out[k] for k in ("dx", "dy", "sx", "sy")]


@pytest.mark.parametrize("noise", [0, 3])
def test_identical_pair_is_left_alone(noise):
    """the identical pair, clean and with uniform noise of +-3: nothing to apply at the default register_min_px = 1/16
    (measured drift with these restatements: none -- no increment reaches the 1/64 px stop)"""
    ref, _, _ = _pair("first")
    rng = np.random.default_rng(7)
    dis = [np.clip(r.astype(int) + rng.integers(-noise, noise + 1, r.shape), 0, 255).astype(np.uint8) for r in ref]
    out = AL.register(*F.restatements(8), ref, dis, filter="bicubic", tile=16, levels=1)
    assert out["converged"] and out["corner_px"] < 1 / 16 and not AL.geometry_applied(out)
    assert abs(out["dx"]) < 0.016 and abs(out["dy"]) < 0.016 and abs(out["sx"] - 1) < 5e-4 and abs(out["sy"] - 1) < 5e-4


def test_flat_pair_does_not_converge():
    flat = [np.full((64, 96), 90, np.uint8)] * 2
    out = AL.register(*F.restatements(8), flat, flat, filter="bicubic", tile=16, levels=None)
    assert not out["converged"] and not AL.geometry_applied(out) and out["iterations"] == 0
    assert (out["x0_q16"], out["y0_q16"], out["w_q16"], out["h_q16"]) == (0, 0, 96 * 65536, 64 * 65536)


def test_crop_margins():
    from pqa2_amd.pipeline import registration_crop
    ident = {"x0_q16": 0, "y0_q16": 0, "w_q16": 192 * 65536, "h_q16": 128 * 65536}
    assert registration_crop(ident, 192, 128, 1, 1) == [0, 0, 0, 0]
    x0, ww = AL.geometry_window(Fraction(3, 2), 1, 192)          # displaced right by 1.5: the last two columns read past the edge
    y0, wh = AL.geometry_window(Fraction(-1, 2), 1, 128)
    g = {"x0_q16": x0, "y0_q16": y0, "w_q16": ww, "h_q16": wh}
    assert registration_crop(g, 192, 128) == [0, 1, 2, 0] and registration_crop(g, 192, 128, 1, 1) == [0, 2, 2, 0]
    x0, ww = AL.geometry_window(0, Fraction(102, 100), 200)      # 2 % larger: two samples out on each side at the edges
    g = {"x0_q16": x0, "y0_q16": 0, "w_q16": ww, "h_q16": 128 * 65536}
    assert registration_crop(g, 200, 128) == [2, 0, 2, 0]
