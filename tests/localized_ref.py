"""Localized-content frames for the VIF / ADM / motion parity tests: a flat background with one small textured patch.

Whole-frame parity (test_gpu_parity.py) divides an error by the whole feature value, so an error that lives on a seam
of a kernel (a tile's halo column, the first lane of a stripe, the row where one march segment hands over to the next,
the mirrored last column) is diluted by the rest of the frame.  Here the only texture is a PATCH x PATCH block on a frame
that is flat at mid grey, where every sample centres to exactly zero:

  * on the flat frame the oracles give VIF num = den = the pixel count of the scale, ADM num = den and motion 0, exactly;
  * so `contribution = oracle64(patch frame) - oracle64(flat frame)` is what the patch's neighbourhood adds to a feature
    (for motion: the value itself), and errors are measured against THAT, not against the whole value;
  * moving the patch by a multiple of STEP = 16 pixels (a whole sample at the coarsest scale, 2^3, times the decimation
    phase of the next filter) leaves all 17 oracle features unchanged to 1e-14 while the patch's support stays away
    from the frame border and the ADM crop border -- interior placements share one oracle evaluation.

No GPU imports: tests/test_localized_ref.py pins these facts on the CPU, tests/test_gpu_localized.py uses them.
"""
from __future__ import annotations

import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np

REL_TOL = 5e-5        # the whole-frame bar of test_gpu_parity.py, here applied to the contribution
REL32_FACTOR = 8.0    # ... or 8 x the f32 oracle's own distance from f64 (tests/fuzz_parity.py's rule)
REL32_MAX = 2e-5      # premise: the f32 oracle stays this close to f64, contribution-normalised
FLOOR = 0.01          # normalisation floor (edge placements: a patch outside the ADM crop contributes exactly 0)
PATCH = 32            # patch side in pixels
SUPPORT = 40          # pixels around the patch its filters reach (VIF: 8 + 2*4 + 4*2 + 8*1 = 32 at scale 3)
STEP = 16             # placement step: every seam of every scale is straddled with >= 8 pixels on each side
OUTER = 0.12          # a patch whose support touches the outer 12 % in the swept direction gets its own oracle run
NOISE = 12            # dis = ref + U[-NOISE, NOISE] inside the patch
SEEDS = (8, 32)       # patch content of frames 2k and 2k+1 of every placement.  Chosen among seeds 1..40 from the f64 oracle
                      # alone: a 32 x 32 patch is 4 x 4 samples at scale 3, and what survives three low-pass filters depends on
                      # the draw -- with these two every feature gains >= 1.4 % of its flat value at 2064 x 128 (8 / 10 / 12
                      # bit), so no interior placement needs the floor (tests/test_localized_ref.py asserts it)

N_FEAT = 17
FEATURES = ([f"vif_num_s{s}" for s in range(4)] + [f"vif_den_s{s}" for s in range(4)] +
            [f"adm_num_s{s}" for s in range(4)] + [f"adm_den_s{s}" for s in range(4)] + ["motion"])

WIDE = (2064, 128)    # multiples of 4 and >= 128: takes the ADM pyramid kernel
TALL = (128, 1056)
ODD_WIDE = (2063, 127)
ODD_TALL = (131, 1057)


def sample_dtype(bpc: int):
    return np.uint8 if bpc <= 8 else np.uint16


def flat_value(bpc: int) -> int:
    return 128 << (bpc - 8)


def flat_frame(w: int, h: int, bpc: int) -> np.ndarray:
    return np.full((h, w), flat_value(bpc), sample_dtype(bpc))


@functools.lru_cache(maxsize=None)
def patch_content(seed: int, bpc: int, enhance: bool = False):
    """(ref, dis) PATCH x PATCH blocks: ref uniform noise over the whole range, dis = ref + U[-NOISE, NOISE] clipped.
    enhance: dis := 2 ref - dis clipped (a sharpened copy, so that an enhancement gain limit of 1.0 bites)."""
    rng = np.random.default_rng(seed)
    peak = (1 << bpc) - 1
    ref = rng.integers(0, peak + 1, (PATCH, PATCH))
    dis = np.clip(ref + rng.integers(-NOISE, NOISE + 1, (PATCH, PATCH)), 0, peak)
    if enhance:
        dis = np.clip(2 * ref - dis, 0, peak)
    dt = sample_dtype(bpc)
    ref, dis = ref.astype(dt), dis.astype(dt)
    ref.setflags(write=False)
    dis.setflags(write=False)
    return ref, dis


def patch_frame(w: int, h: int, x: int, y: int, seed: int, bpc: int, enhance: bool = False):
    """(ref, dis) frames: flat background, the seeded patch with its top-left corner at (x, y), clipped by the frame."""
    assert 0 <= x < w and 0 <= y < h
    pr, pd = patch_content(seed, bpc, enhance)
    ref, dis = flat_frame(w, h, bpc), flat_frame(w, h, bpc)
    pw, ph = min(PATCH, w - x), min(PATCH, h - y)
    ref[y:y + ph, x:x + pw] = pr[:ph, :pw]
    dis[y:y + ph, x:x + pw] = pd[:ph, :pw]
    return ref, dis


def placement_clip(w: int, h: int, places, bpc: int, enhance: bool = False):
    """(refs, diss): placement k occupies frames 2k and 2k+1 -- same position, the two seeded contents, so frame 2k+1
    carries the pair's motion."""
    refs, diss = [], []
    for (x, y) in places:
        for seed in SEEDS:
            r, d = patch_frame(w, h, x, y, seed, bpc, enhance)
            refs.append(r)
            diss.append(d)
    return refs, diss


# ---- placement lists ---------------------------------------------------------------------------------------------------
def wide_places():
    return [(x, 48) for x in range(0, WIDE[0] - PATCH + 1, STEP)]       # x = 0 ... 2032


def tall_places():
    return [(48, y) for y in range(0, TALL[1] - PATCH + 1, STEP)]       # y = 0 ... 1024


def corner_places(w: int, h: int):
    """All four corners and the middle of each edge.  At the right / bottom edge the patch is flush with the last column /
    row, one pixel short of it, and clipped by it (8 of its 32 columns / rows outside; with 12 outside the f32 oracle itself
    is 2.4e-5 from f64 on VIF scale 1 in the bottom right corner at 12 bit, beyond REL32_MAX)."""
    xm, ym = (w - PATCH) // 2, (h - PATCH) // 2
    far_x, far_y = [w - PATCH, w - PATCH - 1, w - PATCH + 8], [h - PATCH, h - PATCH - 1, h - PATCH + 8]
    out = [(0, 0), (xm, 0), (0, ym)]
    for fx, fy in zip(far_x, far_y):
        out += [(fx, 0), (0, fy), (fx, fy), (xm, fy), (fx, ym)]
    return out


def is_interior(pos: int, extent: int) -> bool:
    """The patch support [pos - SUPPORT, pos + PATCH + SUPPORT) stays clear of the outer 12 % of the swept extent (the frame
    border and the 10 % ADM crop border with them)."""
    return pos - SUPPORT >= OUTER * extent and pos + PATCH + SUPPORT <= (1.0 - OUTER) * extent


def interior_mask(w: int, h: int, places, axis: int):
    """axis 0: swept in x; 1: swept in y; None: no placement is interior (corner sets)."""
    if axis is None:
        return [False] * len(places)
    return [is_interior(p[axis], (w, h)[axis]) for p in places]


SWEEPS = {
    # name: (geometry, placements, swept axis)
    "wide": (WIDE, wide_places, 0),
    "tall": (TALL, tall_places, 1),
    "corners_wide": (ODD_WIDE, lambda: corner_places(*ODD_WIDE), None),
    "corners_tall": (ODD_TALL, lambda: corner_places(*ODD_TALL), None),
}


def sweep(name: str):
    (w, h), places, axis = SWEEPS[name]
    return w, h, places(), axis


# ---- oracle values -------------------------------------------------------------------------------------------------------
def pair_features(orc, w, h, x, y, bpc, enhance=False, **kw) -> np.ndarray:
    """[2, 17] oracle records of one placement's two frames (frame 0: motion 0, frame 1: the pair's motion)."""
    a = patch_frame(w, h, x, y, SEEDS[0], bpc, enhance)
    b = patch_frame(w, h, x, y, SEEDS[1], bpc, enhance)
    return orc.clip_features([a[0], b[0]], [a[1], b[1]], bpc, **kw)


def flat_features(orc, w, h, bpc, **kw) -> np.ndarray:
    """[17] oracle record of the flat frame (second of two, so that motion is a real difference: 0)."""
    f = flat_frame(w, h, bpc)
    return orc.clip_features([f, f], [f, f], bpc, **kw)[1]


def flat_expected(w: int, h: int) -> np.ndarray:
    """The VIF part of the flat record in closed form: num = den = pixels of the scale (each scale halves, rounding down)."""
    px = [float((w >> s) * (h >> s)) for s in range(4)]
    return np.array(px + px)


class Expected:
    """Oracle values of a placement list: exp64 / exp32 [n, 2, 17], the flat record, and the bar of every value.

    Placements that are not interior are evaluated one by one; the interior ones share the evaluation of the middle
    interior placement (translation by multiples of STEP, pinned by tests/test_localized_ref.py)."""

    def __init__(self, o64, o32, w, h, places, axis, bpc, enhance=False, threads=8, **kw):
        self.w, self.h, self.places, self.bpc = w, h, list(places), bpc
        self.interior = np.array(interior_mask(w, h, self.places, axis), bool)
        inner = np.flatnonzero(self.interior)
        todo = [int(k) for k in np.flatnonzero(~self.interior)]
        self.anchor = int(inner[len(inner) // 2]) if len(inner) else None
        if self.anchor is not None:
            todo.append(self.anchor)

        def one(k):
            x, y = self.places[k]
            return k, pair_features(o64, w, h, x, y, bpc, enhance, **kw), pair_features(o32, w, h, x, y, bpc, enhance, **kw)

        n = len(self.places)
        self.exp64, self.exp32 = np.zeros((n, 2, N_FEAT)), np.zeros((n, 2, N_FEAT))
        with ThreadPoolExecutor(max_workers=threads) as ex:
            for k, e64, e32 in ex.map(one, todo):
                self.exp64[k], self.exp32[k] = e64, e32
        if self.anchor is not None:
            self.exp64[self.interior] = self.exp64[self.anchor]
            self.exp32[self.interior] = self.exp32[self.anchor]
        self.flat = flat_features(o64, w, h, bpc, **kw)
        self.contribution = contribution(self.exp64, self.flat)
        self.norm = normaliser(self.exp64, self.flat)
        # the f32 oracle's own contribution-normalised distance from f64, per placement (worst value of the pair)
        self.rel32 = (np.abs(self.exp32 - self.exp64) / self.norm)[..., _checked()].reshape(n, -1).max(axis=1)
        self.bar = np.maximum(REL_TOL, REL32_FACTOR * self.rel32)[:, None, None] * self.norm

    def floor_used(self) -> np.ndarray:
        """[n, 2, 17] bool: the value's normaliser is the 0.01 floor, not its contribution."""
        return np.abs(self.contribution) < FLOOR * np.abs(self.exp64)


def _checked() -> np.ndarray:
    """Boolean [2, 17] mask of the values of a pair that carry information: all 16 spatial features of both frames and the
    motion of frame 1 (frame 0's motion belongs to the previous placement)."""
    m = np.ones((2, N_FEAT), bool)
    m[0, 16] = False
    return m


CHECKED = _checked()


def contribution(exp64: np.ndarray, flat: np.ndarray) -> np.ndarray:
    """What the patch adds to every feature: oracle64(patch frame) - oracle64(flat frame); motion: the value itself."""
    c = exp64 - flat
    c[..., 16] = exp64[..., 16]
    return c


def normaliser(exp64: np.ndarray, flat: np.ndarray) -> np.ndarray:
    """max(|contribution|, 0.01 |oracle64|), and 1 where both are 0 (frame 0's motion: never compared)."""
    nrm = np.maximum(np.abs(contribution(exp64, flat)), FLOOR * np.abs(exp64))
    return np.where(nrm == 0.0, 1.0, nrm)
