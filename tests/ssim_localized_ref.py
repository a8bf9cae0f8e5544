"""Localized-content frames for the float_ssim / float_ms_ssim parity tests (csrc/ssim_family.hip): a flat background
with one strongly distorted 64 x 64 patch, after tests/localized_ref.py.

The whole-frame test (test_gpu_ssim_family.py::test_matches_the_restatement) holds a mean that is close to 1 to an
absolute 1e-5 on textured frames; an error on a seam of a kernel -- a map tile's halo column, the row where one thread's
8 output rows end, a decimation-only tile of the scale-0 launch, the folded last column of an odd pyramid level, the last
box of a width that is no multiple of the box factor -- is diluted by every other window of the frame.  Here ref = dis =
mid grey outside the patch, where the restatement gives l = c = s = 1 exactly (f64 and f32), so

  * `deficit = ref64(patch frame) - 1` is what the patch's neighbourhood takes from a mean, and errors are measured
    against THAT: norm = max(|deficit|, FLOOR x |deficit of the sweep's anchor placement|) per slot;
  * the bar is |gpu - ref64| <= max(REL_TOL, REL32_FACTOR x rel32) x norm + ULP32, rel32 being the f32 restatement's own
    |ref32 - ref64| / norm for that placement and slot (tests/fuzz_parity.py's rule) and ULP32 = 2^-23 one f32 ulp at 1.0:
    the kernels emit f32 map values near 1 and form C * rcp(C) on flat windows, so a mean of them may differ from 1 by
    that much with nothing wrong.  Nothing in the bar comes from the code under test;
  * moving the patch by a multiple of STEP = 16 pixels (one sample of scale 4) leaves all 20 slots unchanged to 1e-14 while
    its support stays clear of the invalid border of scale 4, so interior placements share one restatement evaluation.

The patch carries energy in every octave (block patterns of side 1, 2, 4, 8, 16: still a 4 x 4 high-contrast blob at
scale 4) and dis is strongly distorted (luminance offset, halved contrast, independent noise): with a mild distortion the
deficits are 1e-5 ... 1e-8 of the mean and f32 rounding swamps them.

Checked slots: float_ssim and its l, c, s means (ext[0:4]), the per-scale l, c, s means (ext[5:20]) and, by the same rule
on ms - 1, the product ext[4].  No (slot, scale) pair is dropped: the patch's luminance offset of 32 grey levels gives the
l means deficits of 2e-4 ... 7e-4, and the f32 restatement stays within SSF_REL32_MAX of f64 on them as on c and s.

Tile constants restated from pqa2_amd/csrc/kernels.h (kSsfTileW, kSsfTileH) and ssim_family.hip (DTH, TW): the CPU test
asserts the tile counts the sweep table claims.

No GPU imports.
"""
from __future__ import annotations

import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from tests import localized_ref as L
from tests import ssim_family_ref as R
from tests.localized_ref import flat_frame, flat_value, sample_dtype  # noqa: F401  (shared with the VIF / ADM / motion tests)

REL_TOL = L.REL_TOL              # 5e-5: localized_ref's bar, applied to the deficit
REL32_FACTOR = L.REL32_FACTOR    # 8 x the f32 restatement's own distance from f64
FLOOR = L.FLOOR                  # 0.01: normalisation floor for placements clipped into the invalid border
ULP32 = 2.0 ** -23               # one f32 ulp at 1.0
PATCH = 64
STEP = 16                        # one sample of scale 4
BORDER = 5 * 16                  # invalid border of the scale-4 map in pixels
SUPPORT = 5 * 16 + 4 * (1 + 2 + 4 + 8) + 4   # scale-4 window radius + the four 9-tap filters, rounded up to 144
THREADS = 16                     # restatement evaluations in flight (numpy releases the GIL)

MAP_TW, MAP_TH = 64, 32          # kSsfTileW x kSsfTileH: one workgroup's block of the SSIM map (kernels.h)
DOWN_TW, DOWN_TH = 64, 16        # ssf_down_kernel's output tile (TW x DTH in ssim_family.hip)
FUSED_TW, FUSED_TH = MAP_TW // 2, MAP_TH // 2   # outputs of the decimation fused into the scale-0 map launch, per tile

N_SLOT = 20
SLOTS = (["float_ssim", "float_ssim_l", "float_ssim_c", "float_ssim_s", "float_ms_ssim"] +
         [f"ms_{q}_s{j}" for q in "lcs" for j in range(5)])
FS_SLOTS = (0, 1, 2, 3)

# Premise (asserted by tests/test_ssim_localized_ref.py): over the interior placements of every sweep and every slot the
# f32 restatement stays this close to f64, deficit-normalised.  Twice the worst value measured with the restatements on
# the CPU (first, middle and last interior placement of wide, tall, box2_wide and box2_tall, 8 / 10 / 12 bit): 3.02e-6,
# set by ms_l_s4 of box2_wide at 10 bit, placement (816, 160); c and s: 2.46e-6 (ms_c_s4, tall, 12 bit), float_ssim 6e-8.
SSF_REL32_MAX = 6.1e-6

# Patch content of frames 2k and 2k + 1 of every placement.  Chosen among seeds 1..40 from the f64 restatement alone: the
# two whose smallest |deficit| over all 20 slots, at the middle of the wide and of the tall frame (8 bit), is largest
# (6.2e-4 and 5.6e-4) -- what survives four low-pass filters depends on the draw.
SEEDS = (33, 39)


# ---- content ---------------------------------------------------------------------------------------------------------
def _octaves(rng) -> np.ndarray:
    """Sum of random block patterns, block sides 1, 2, 4, 8, 16, each uniform in [-1, 1): energy in every octave."""
    out = np.zeros((PATCH, PATCH))
    for b in (1, 2, 4, 8, 16):
        out += np.kron(rng.uniform(-1.0, 1.0, (PATCH // b, PATCH // b)), np.ones((b, b)))
    return out


@functools.lru_cache(maxsize=None)
def patch_content(seed: int, bpc: int):
    """(ref, dis) PATCH x PATCH blocks in 8-bit units times 2^(bpc - 8): ref = 128 + 40 octaves, dis = 96 + 0.5 (ref - 128)
    + 20 independent octaves, both rounded and clipped."""
    rng = np.random.default_rng(seed)
    unit, peak = float(1 << (bpc - 8)), (1 << bpc) - 1
    r = 128.0 + 40.0 * _octaves(rng)
    d = 96.0 + 0.5 * (r - 128.0) + 20.0 * _octaves(rng)
    dt = sample_dtype(bpc)
    ref = np.clip(np.rint(r * unit), 0, peak).astype(dt)
    dis = np.clip(np.rint(d * unit), 0, peak).astype(dt)
    ref.setflags(write=False)
    dis.setflags(write=False)
    return ref, dis


def patch_frame(w: int, h: int, x: int, y: int, seed: int, bpc: int):
    """(ref, dis) frames: flat mid grey, the seeded patch with its top-left corner at (x, y), clipped by the frame."""
    assert 0 <= x < w and 0 <= y < h
    pr, pd = patch_content(seed, bpc)
    ref, dis = flat_frame(w, h, bpc), flat_frame(w, h, bpc)
    pw, ph = min(PATCH, w - x), min(PATCH, h - y)
    ref[y:y + ph, x:x + pw] = pr[:ph, :pw]
    dis[y:y + ph, x:x + pw] = pd[:ph, :pw]
    return ref, dis


def placement_clip(w: int, h: int, places, bpc: int):
    """(refs, diss): placement k occupies frames 2k and 2k + 1 -- the same position, the two seeded contents."""
    refs, diss = [], []
    for (x, y) in places:
        for seed in SEEDS:
            r, d = patch_frame(w, h, x, y, seed, bpc)
            refs.append(r)
            diss.append(d)
    return refs, diss


# ---- sweeps ----------------------------------------------------------------------------------------------------------
WIDE, TALL = (2064, 176), (176, 2064)
ODD_WIDE, ODD_TALL = (2049, 193), (193, 2049)   # 32 k + 1: odd at every one of the five levels (2049, 1025, 513, 257, 129)
UNION = (200, 208)
BOX_TALL, BOX_WIDE = (400, 1104), (1104, 400)


def _mid(extent: int) -> int:
    return (extent - PATCH) // 2 // STEP * STEP


def line_places(w: int, h: int, axis: int):
    """Every STEP along `axis` (the last placement flush with or short of the far edge), centred in the other."""
    if axis == 0:
        return [(x, _mid(h)) for x in range(0, w - PATCH + 1, STEP)]
    return [(_mid(w), y) for y in range(0, h - PATCH + 1, STEP)]


def corner_places(w: int, h: int):
    """The centre (the anchor), then all four corners and the middle of each edge; at the right / bottom edge the patch is
    flush with the last column / row, one pixel short of it, and clipped by it (8 of its 64 columns / rows outside)."""
    xm, ym = (w - PATCH) // 2, (h - PATCH) // 2
    far_x, far_y = [w - PATCH, w - PATCH - 1, w - PATCH + 8], [h - PATCH, h - PATCH - 1, h - PATCH + 8]
    out = [(xm, ym), (0, 0), (xm, 0), (0, ym)]
    for fx, fy in zip(far_x, far_y):
        out += [(fx, 0), (0, fy), (fx, fy), (xm, fy), (fx, ym)]
    return out


def grid_places(w: int, h: int):
    """Every STEP in both directions, the centre-most placement (the anchor) first."""
    out = [(x, y) for y in range(0, h - PATCH + 1, STEP) for x in range(0, w - PATCH + 1, STEP)]
    c = min(out, key=lambda p: abs(p[0] - _mid(w)) + abs(p[1] - _mid(h)))
    return [c] + [p for p in out if p != c]


def is_interior(pos: int, extent: int) -> bool:
    """The patch's support stays inside the valid region of the scale-4 map in the swept direction."""
    return pos - SUPPORT >= BORDER and pos + PATCH + SUPPORT <= extent - BORDER


def interior_mask(w: int, h: int, places, axis):
    """axis 0: swept in x; 1: swept in y; None: no placement is interior (corner and grid sets)."""
    if axis is None:
        return [False] * len(places)
    return [is_interior(p[axis], (w, h)[axis]) for p in places]


SWEEPS = {
    # name: (geometry, placements, swept axis)
    "wide": (WIDE, lambda: line_places(*WIDE, 0), 0),
    "tall": (TALL, lambda: line_places(*TALL, 1), 1),
    "corners_wide": (ODD_WIDE, lambda: corner_places(*ODD_WIDE), None),
    "corners_tall": (ODD_TALL, lambda: corner_places(*ODD_TALL), None),
    "union_x": (UNION, lambda: grid_places(*UNION), None),
    "box2_tall": (BOX_TALL, lambda: line_places(*BOX_TALL, 1), 1),
    "box2_wide": (BOX_WIDE, lambda: line_places(*BOX_WIDE, 0), 0),
}


def sweep(name: str):
    (w, h), places, axis = SWEEPS[name]
    return w, h, places(), axis


# ---- tile counts (what the sweep table claims; asserted on the CPU) ----------------------------------------------------
def _cdiv(a: int, b: int) -> int:
    return -(-a // b)


def map_tiles(w: int, h: int):
    """(columns, rows) of 64 x 32 map tiles of a w x h plane."""
    return _cdiv(w - 10, MAP_TW), _cdiv(h - 10, MAP_TH)


def down_tiles(w: int, h: int):
    """(columns, rows) of 64 x 16 output tiles of ssf_down_kernel on a w x h input."""
    return _cdiv(_cdiv(w, 2), DOWN_TW), _cdiv(_cdiv(h, 2), DOWN_TH)


def fused_tiles(w: int, h: int):
    """(columns, rows) of the 32 x 16 output tiles of the decimation fused into the scale-0 launch."""
    return _cdiv(_cdiv(w, 2), FUSED_TW), _cdiv(_cdiv(h, 2), FUSED_TH)


def decimation_only(w: int, h: int):
    """(columns, rows) of the scale-0 launch that only decimate: the union of both tilings minus the map's tiles."""
    (mx, my), (fx, fy) = map_tiles(w, h), fused_tiles(w, h)
    return max(0, fx - mx), max(0, fy - my)


# ---- restatement values ------------------------------------------------------------------------------------------------
def record(ref, dis, bpc: int, dtype=np.float64, ms: bool = True) -> np.ndarray:
    """The 20 slots; ms=False: float_ssim alone, the MS-SSIM slots NaN (box-factor cases on large frames)."""
    return R.ext_record(ref, dis, bpc, want_ms_ssim=ms, dtype=dtype)[:N_SLOT]


def pair_records(w, h, x, y, bpc, dtype=np.float64, ms: bool = True) -> np.ndarray:
    """[2, 20] restatement records of one placement's two frames."""
    return np.stack([record(*patch_frame(w, h, x, y, seed, bpc), bpc, dtype, ms) for seed in SEEDS])


class Expected:
    """Restatement values of a placement list: exp64 / exp32 [n, 2, 20], deficit, norm, rel32 and bar per value.

    Placements that are not interior are evaluated one by one; the interior ones share the evaluation of the middle
    interior placement (translation by multiples of STEP, pinned by tests/test_ssim_localized_ref.py).  The anchor (whose
    deficit carries the floor) is that middle interior placement, or the first placement of a set without interior --
    corner_places and grid_places put the centre there.  Slots that were not evaluated (ms=False) are NaN throughout."""

    def __init__(self, w, h, places, axis, bpc, threads=THREADS, ms=True):
        self.w, self.h, self.places, self.bpc = w, h, list(places), bpc
        self.interior = np.array(interior_mask(w, h, self.places, axis), bool)
        inner = np.flatnonzero(self.interior)
        todo = [int(k) for k in np.flatnonzero(~self.interior)]
        self.anchor = int(inner[len(inner) // 2]) if len(inner) else 0
        if len(inner):
            todo.append(self.anchor)

        def one(k):
            x, y = self.places[k]
            return k, pair_records(w, h, x, y, bpc, ms=ms), pair_records(w, h, x, y, bpc, np.float32, ms)

        n = len(self.places)
        self.exp64, self.exp32 = np.zeros((n, 2, N_SLOT)), np.zeros((n, 2, N_SLOT))
        with ThreadPoolExecutor(max_workers=min(threads, THREADS)) as ex:
            for k, e64, e32 in ex.map(one, todo):
                self.exp64[k], self.exp32[k] = e64, e32
        if len(inner):
            self.exp64[self.interior] = self.exp64[self.anchor]
            self.exp32[self.interior] = self.exp32[self.anchor]
        self.deficit = self.exp64 - 1.0
        self.anchor_deficit = self.deficit[self.anchor]                                                     # [2, 20]
        self.norm = normaliser(self.deficit, self.anchor_deficit)
        self.rel32 = np.abs(self.exp32 - self.exp64) / self.norm                                            # [n, 2, 20]
        self.bar = np.maximum(REL_TOL, REL32_FACTOR * self.rel32) * self.norm + ULP32

    def floor_used(self) -> np.ndarray:
        """[n, 2, 20] bool: the value's normaliser is the floor, not its own deficit."""
        return np.abs(self.deficit) < FLOOR * np.abs(self.anchor_deficit)


def normaliser(deficit: np.ndarray, anchor_deficit: np.ndarray) -> np.ndarray:
    """max(|deficit|, FLOOR |anchor's deficit|) per slot and frame of the pair."""
    return np.maximum(np.abs(deficit), FLOOR * np.abs(anchor_deficit))


# ---- part 0: what the whole-frame bar can see ---------------------------------------------------------------------------
def column_detection_threshold(ref, dis, bpc: int, tol: float) -> dict:
    """For every mean the whole-frame test holds to an absolute `tol`: the smallest relative change eps of ALL windows of
    one map column (v -> v (1 + eps), the column where that is most visible) that moves the mean by `tol`.
    eps = tol x windows / max over columns of sum |v|.  Keys: the slot names."""
    out = {}

    def put(name, m):
        out[name] = tol * m.size / float(np.abs(m).sum(axis=0).max())

    f = R.decimation_factor(ref.shape[1], ref.shape[0])
    x, y = R.box_decimate(R.to_float(ref, bpc), f), R.box_decimate(R.to_float(dis, bpc), f)
    l, c, s = R.lcs_maps(x, y, True)
    for name, m in zip(SLOTS[:4], (l * c * s, l, c, s)):
        put(name, m)
    x, y = R.to_float(ref, bpc), R.to_float(dis, bpc)
    for j in range(R.MS_SCALES):
        for q, m in zip("lcs", R.lcs_maps(x, y, True)):
            put(f"ms_{q}_s{j}", m)
        if j + 1 < R.MS_SCALES:
            x, y = R.lpf97_decimate(x), R.lpf97_decimate(y)
    return out
