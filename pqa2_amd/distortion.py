"""Distortion map: where inside the frame two clips differ.  Pure Python and numpy, no GPU: the solver behind
score_files(distortion_map=T).  The measurement is FeatureEngine.tile_moments (pqa_tile_moments, csrc/tile_moments.hip):
per tile of T x T pixels the exact uint64 sums M[..., 0..5] = sum r, sum d, sum r^2, sum d^2, sum r d, sum |d - r| of the
reference r and the captured d.  From them: tile_metrics (MSE, MAD, PSNR, block SSIM of every tile), frame_summary (the worst
tile of a frame and how concentrated its error is), find_defects (localised, short-lived damage as events with a box) and
persistent_regions (tiles that are hot through the whole clip: a burnt-in logo, clock or timecode, and the clip PSNR without
them).  Every decision is taken on integers -- Python ints, or int64 where the bound is shown; floating point appears only in
the reported figures, after one division."""
from fractions import Fraction

import numpy as np

SUM_R, SUM_D, SUM_RR, SUM_DD, SUM_RD, SUM_AD = range(6)


def _top(bit_depth: int) -> int:
    return (1 << int(bit_depth)) - 1


def _ratio(v, limit: int = 1 << 16) -> Fraction:
    """a threshold given as int, float or Fraction as the simplest fraction near it (0.9 -> 9/10, not the float's binary
    neighbour): the rules below compare integers"""
    return Fraction(v).limit_denominator(limit)


def psnr_cap(bit_depth: int) -> float:
    """the cap the project applies to psnr_y: libvmaf's 6 b + 12 dB (60 dB at 8 bit, 72 dB at 10 bit)"""
    return 6.0 * bit_depth + 12.0


def _psnr(sse, pixels, bit_depth: int) -> np.ndarray:
    """PSNR in dB of arrays of SSE and pixel counts (one division each), capped"""
    top = float(_top(bit_depth))
    mse = np.asarray(sse, np.float64) / np.asarray(pixels, np.float64)
    with np.errstate(divide="ignore"):
        db = np.where(mse > 0, 10.0 * np.log10(top * top / np.where(mse > 0, mse, 1.0)), np.inf)
    return np.minimum(db, psnr_cap(bit_depth))


def tile_counts(width: int, height: int, tile: int) -> np.ndarray:
    """int64 [ty, tx]: the pixels of every tile of a width x height plane; edge tiles hold the pixels that exist"""
    if tile < 1 or width < 1 or height < 1:
        raise ValueError("tile_counts needs a positive size and tile")
    cw = np.minimum(tile, width - np.arange(-(-width // tile), dtype=np.int64) * tile)
    ch = np.minimum(tile, height - np.arange(-(-height // tile), dtype=np.int64) * tile)
    return ch[:, None] * cw[None, :]


def tile_sse(M: np.ndarray) -> np.ndarray:
    """uint64 [..., ty, tx]: the squared error of every tile, sum r^2 - 2 sum r d + sum d^2 (never negative; below 2^37 for a
    64-tile at 12 bit)"""
    M = np.asarray(M)
    if M.dtype != np.uint64 or M.shape[-1] != 6:
        raise ValueError("tile moments are uint64 [..., 6]")
    return M[..., SUM_RR] + M[..., SUM_DD] - np.uint64(2) * M[..., SUM_RD]


def tile_metrics(M: np.ndarray, width: int, height: int, tile: int, bit_depth: int, frames: int = 1) -> dict:
    """{mse, mad, psnr, ssim}: float64 arrays of the shape of M without its last axis ([n, ty, tx]).  `frames`: the frame
    pairs summed into M (1: per-frame moments; the clip-summed moments of n frames: n), which multiplies the pixel counts.
    psnr is capped at psnr_cap(bit_depth).  ssim is the block form
        ((2 ur ud + C1)(2 srd + C2)) / ((ur^2 + ud^2 + C1)(sr^2 + sd^2 + C2)),  C1 = (0.01 top)^2, C2 = (0.03 top)^2,
    with biased variances, evaluated as
        ((10^4 2 Sr Sd + t)(10^4 2 (n Srd - Sr Sd) + 9 t)) / ((10^4 (Sr^2 + Sd^2) + t)(10^4 (n Srr - Sr^2 + n Sdd - Sd^2) + 9 t)),
    t = top^2 n^2: all four factors are exact integers, and float64 sees them only for two products and one division.
    int64 holds them for per-frame moments: n <= 2^12, Sr <= 2^12 * 4095 < 2^24, so 2 Sr Sd, Sr^2 + Sd^2, 2 n Srd and
    n Srr + n Sdd stay below 2^49, 10^4 times that below 5.63e18, t <= 4095^2 * 2^24 < 2^48, 9 t < 2.54e18, the sum below
    8.2e18 < 2^63.  Clip-summed moments (frames > 1) are wider and go through Python ints."""
    M = np.asarray(M)
    S = tile_sse(M)
    n = tile_counts(width, height, tile) * int(frames)
    if M.shape[-3:-1] != n.shape:
        raise ValueError(f"moments of a {M.shape[-2]} x {M.shape[-3]} grid, but the plane has {n.shape[1]} x {n.shape[0]} tiles")
    top = _top(bit_depth)
    wide = frames > 1 or bit_depth > 12 or tile > 64
    I = M.astype(object) if wide else M.astype(np.int64)
    nn = n.astype(object) if wide else n
    sr, sd = I[..., SUM_R], I[..., SUM_D]
    t = top * top * nn * nn
    p1 = 10000 * (2 * sr * sd) + t
    p2 = 10000 * (2 * (nn * I[..., SUM_RD] - sr * sd)) + 9 * t
    q1 = 10000 * (sr * sr + sd * sd) + t
    q2 = 10000 * (nn * I[..., SUM_RR] - sr * sr + nn * I[..., SUM_DD] - sd * sd) + 9 * t
    if wide:      # one correctly rounded division of two exact integers
        ssim = np.frompyfunc(lambda a, b: float(Fraction(int(a), int(b))), 2, 1)(p1 * p2, q1 * q2).astype(np.float64)
    else:
        ssim = (p1.astype(np.float64) * p2.astype(np.float64)) / (q1.astype(np.float64) * q2.astype(np.float64))
    nf = n.astype(np.float64)
    return {"mse": S.astype(np.float64) / nf, "mad": M[..., SUM_AD].astype(np.float64) / nf,
            "psnr": _psnr(S, nf, bit_depth), "ssim": ssim}


def _as_sse(M) -> np.ndarray:
    M = np.asarray(M)
    return tile_sse(M) if M.ndim == 4 else M


def frame_summary(M, width: int, height: int, tile: int, bit_depth: int) -> dict:
    """Per frame of M ([n, ty, tx, 6] moments, or [n, ty, tx] tile SSE): {tile_psnr_min [n], tile_psnr_min_at [n, 2] (tile
    column i and row j of the first such tile), concentration [n]}.  concentration is the share of the frame's SSE held by
    its ceil(N / 16) tiles of largest SSE (N tiles): 1/16 or a little more for an error spread evenly, near 1 for one broken
    region; 0 for identical frames.  The sums are exact in uint64 (a tile's SSE is below 2^37, a plane of 8192 x 8192 has
    at most 2^20 tiles); one division."""
    S = _as_sse(M)
    if S.ndim != 3 or S.dtype != np.uint64:
        raise ValueError("frame_summary needs [n, ty, tx, 6] moments or [n, ty, tx] uint64 SSE")
    counts = tile_counts(width, height, tile)
    if S.shape[1:] != counts.shape:
        raise ValueError("tile grid and plane size disagree")
    n, ty, tx = S.shape
    psnr = _psnr(S, counts.astype(np.float64), bit_depth).reshape(n, -1)
    at = psnr.argmin(axis=1) if n else np.zeros(0, np.int64)
    k = -(-(ty * tx) // 16)
    flat = np.sort(S.reshape(n, -1), axis=1)[:, ::-1]
    total, head = flat.sum(axis=1, dtype=np.uint64), flat[:, :k].sum(axis=1, dtype=np.uint64)
    conc = np.array([int(head[f]) / int(total[f]) if total[f] else 0.0 for f in range(n)], np.float64)
    return {"tile_psnr_min": psnr[np.arange(n), at] if n else np.zeros(0), "concentration": conc,
            "tile_psnr_min_at": np.stack([at % tx, at // tx], axis=1).astype(np.int64)}


def _floor_thresholds(counts: np.ndarray, per_pixel: Fraction) -> np.ndarray:
    """int64 [ty, tx]: floor(per_pixel * n) of every tile -- an integer S exceeds the real bound exactly when it exceeds its
    floor.  A grid has at most four distinct counts."""
    out = np.zeros(counts.shape, np.int64)
    for c in np.unique(counts):
        out[counts == c] = int(per_pixel * int(c) // 1)
    return out


def hot_tiles(S, counts, *, factor=16, min_mse=4.0, tile: int, bit_depth: int = 8) -> np.ndarray:
    """bool [n, ty, tx]: tile (i, j) is hot in frame f when BOTH hold, in integers,
        S > min_mse (top / 255)^2 n            -- its MSE exceeds min_mse in 8-bit code values squared, and
        S T^2 > factor S_med n                 -- its MSE exceeds `factor` times the frame's typical tile MSE,
    n the tile's pixels, S_med the lower median of the SSE of the frame's full tiles (those of T^2 pixels; of all tiles when
    the plane has no full tile).  Both bounds are taken as floor(bound): S is an integer."""
    S = np.asarray(S)
    counts = np.asarray(counts, np.int64)
    if S.ndim != 3 or S.dtype != np.uint64 or S.shape[1:] != counts.shape:
        raise ValueError("hot_tiles needs uint64 SSE [n, ty, tx] and the counts [ty, tx] of the same grid")
    top = _top(bit_depth)
    fac, floor_mse = _ratio(factor), _ratio(min_mse)
    if fac < 0 or floor_mse < 0:
        raise ValueError("factor and min_mse must not be negative")
    Si = S.astype(np.int64)      # below 2^37
    absolute = _floor_thresholds(counts, floor_mse * top * top / (255 * 255))
    full = counts == tile * tile
    pick = full if full.any() else np.ones_like(full)
    hot = np.zeros(S.shape, bool)
    for f in range(S.shape[0]):
        vals = np.sort(Si[f][pick])
        med = int(vals[(len(vals) - 1) // 2])
        relative = _floor_thresholds(counts, fac * med / (tile * tile))
        hot[f] = (Si[f] > absolute) & (Si[f] > relative)
    return hot


def _components(mask: np.ndarray):
    """the 4-neighbour components of a bool [ty, tx] mask as lists of (j, i), in raster order of their first tile"""
    ty, tx = mask.shape
    seen = np.zeros_like(mask)
    out = []
    for j0, i0 in zip(*np.nonzero(mask)):
        if seen[j0, i0]:
            continue
        seen[j0, i0] = True
        comp, stack = [], [(int(j0), int(i0))]
        while stack:
            j, i = stack.pop()
            comp.append((j, i))
            for jj, ii in ((j - 1, i), (j + 1, i), (j, i - 1), (j, i + 1)):
                if 0 <= jj < ty and 0 <= ii < tx and mask[jj, ii] and not seen[jj, ii]:
                    seen[jj, ii] = True
                    stack.append((jj, ii))
        out.append(sorted(comp))
    return out


def plane_size(counts, tile: int):
    """(width, height) of the plane a grid of counts belongs to.  A grid of one tile does not say how its pixels are arranged
    (it is taken as a single row of them): pass the size to the callers below instead."""
    counts = np.asarray(counts, np.int64)
    ty, tx = counts.shape
    if tx > 1:      # tile (0, 0) is `tile` wide: its count gives the height of the first row of tiles
        w_last = int(counts[0, -1]) // (int(counts[0, 0]) // tile)
    elif ty > 1:    # ... or `tile` high: its count gives the width of the only column
        w_last = int(counts[0, 0]) // tile
    else:
        w_last = int(counts[0, 0])
    return (tx - 1) * tile + w_last, (ty - 1) * tile + int(counts[-1, -1]) // w_last


def _box(tiles, tile: int, width: int, height: int):
    js, is_ = [t[0] for t in tiles], [t[1] for t in tiles]
    return [min(is_) * tile, min(js) * tile, min((max(is_) + 1) * tile, width), min((max(js) + 1) * tile, height)]


def find_defects(S, counts, *, factor=16, min_mse=4.0, tile: int, bit_depth: int = 8, width: int | None = None,
                 height: int | None = None, hot: np.ndarray | None = None) -> list:
    """The localised defects of a clip from its tile SSE S[f, j, i] (uint64) and the tile pixel counts [ty, tx].  The hot
    tiles of a frame (hot_tiles: the `factor` and `min_mse` rules; or the mask given as `hot`) are joined into 4-neighbour
    components; components of consecutive frames that share a tile form one event.  Returns the events, ordered by first
    frame and position, as dicts:
      first, last   the first and last frame of the event
      frames        the frames in which it has a component
      peak_frame    the frame in which the MSE over the event's tiles is largest (the first of them), peak_mse: that MSE
      box           [x0, y0, x1, y1] in pixels (x1, y1 exclusive): the union of its tiles over the event, clipped to the plane
      share         the SSE of its tiles over the SSE of the whole frame, at the peak frame
    `width`, `height`: the plane's size, for the clip of the box (default: derived from the counts)."""
    S = np.asarray(S)
    counts = np.asarray(counts, np.int64)
    if hot is None:
        hot = hot_tiles(S, counts, factor=factor, min_mse=min_mse, tile=tile, bit_depth=bit_depth)
    if width is None or height is None:
        width, height = plane_size(counts, tile)
    parent = []

    def find(e):
        while parent[e] != e:
            parent[e] = parent[parent[e]]
            e = parent[e]
        return e
    parts = []      # (event id, frame, tiles) of every component
    prev = {}       # tile -> event id, of the frame before
    for f in range(S.shape[0]):
        cur = {}
        for comp in (_components(hot[f]) if hot[f].any() else []):
            touching = sorted({find(prev[t]) for t in comp if t in prev})
            if touching:
                e = touching[0]
                for other in touching[1:]:
                    parent[other] = e
            else:
                e = len(parent)
                parent.append(e)
            parts.append((e, f, comp))
            for t in comp:
                cur[t] = e
        prev = cur
    events = {}
    for e, f, comp in parts:
        events.setdefault(find(e), {}).setdefault(f, []).extend(comp)
    out = []
    for per_frame in events.values():
        tiles = sorted({t for comp in per_frame.values() for t in comp})
        peak = None
        for f in sorted(per_frame):
            sse = sum(int(S[f, j, i]) for j, i in per_frame[f])
            pix = sum(int(counts[j, i]) for j, i in per_frame[f])
            if peak is None or sse * peak[2] > peak[1] * pix:      # a larger MSE, compared cross-multiplied
                peak = (f, sse, pix)
        total = int(S[peak[0]].sum(dtype=np.uint64))      # below 2^57: exact
        out.append({"first": min(per_frame), "last": max(per_frame), "frames": len(per_frame), "peak_frame": peak[0],
                    "peak_mse": peak[1] / peak[2], "box": _box(tiles, tile, width, height),
                    "share": peak[1] / total if total else 0.0})
    return sorted(out, key=lambda ev: (ev["first"], ev["box"][1], ev["box"][0]))


def persistent_tiles(hot, share=0.9) -> np.ndarray:
    """bool [ty, tx]: the tiles that are hot in at least `share` of the n frames of hot [n, ty, tx] (and in one at least),
    compared in integers"""
    hot = np.asarray(hot, bool)
    r = _ratio(share, 1000)
    times = hot.sum(axis=0).astype(np.int64)
    return (times * r.denominator >= r.numerator * hot.shape[0]) & (times > 0)


def persistent_regions(hot, S, counts, *, share=0.9, tile: int, bit_depth: int = 8, width: int | None = None,
                       height: int | None = None) -> dict:
    """Overlay candidates: the tiles that are hot (hot_tiles) in at least `share` of the frames -- a channel logo, a clock or
    a timecode burnt into the capture lowers every score of every frame, and stays.  Returns {regions, tiles, psnr_all,
    psnr_excluding}: `regions` the 4-neighbour components of those tiles as {box: [x0, y0, x1, y1], tiles, frames_hot_min};
    `psnr_all` the PSNR of the plane over the whole clip (total SSE over total pixels, capped like psnr_y), `psnr_excluding`
    the same with the SSE and the pixels of those tiles taken out -- exact, because SSE is additive (None when every tile is
    excluded)."""
    hot = np.asarray(hot, bool)
    S = np.asarray(S)
    counts = np.asarray(counts, np.int64)
    if hot.shape != S.shape or S.shape[1:] != counts.shape:
        raise ValueError("persistent_regions needs hot and S of one shape [n, ty, tx] and counts [ty, tx]")
    if width is None or height is None:
        width, height = plane_size(counts, tile)
    n = S.shape[0]
    times = hot.sum(axis=0).astype(np.int64)
    mask = persistent_tiles(hot, share)
    per_tile = S.sum(axis=0, dtype=np.uint64)      # a tile over the clip: below 2^37 n, exact; the plane's total need not fit
    sse_all = sum(int(v) for v in per_tile.ravel())
    pix_all = int(counts.sum()) * n
    sse_in = sum(int(v) for v in per_tile[mask])
    pix_in = int(counts[mask].sum()) * n
    regions = [{"box": _box(comp, tile, width, height), "tiles": len(comp),
                "frames_hot_min": int(min(times[j, i] for j, i in comp))} for comp in _components(mask)]
    return {"regions": regions, "tiles": int(mask.sum()),
            "psnr_all": float(_psnr(sse_all, pix_all, bit_depth)) if pix_all else None,
            "psnr_excluding": float(_psnr(sse_all - sse_in, pix_all - pix_in, bit_depth)) if pix_all > pix_in else None}


def heatmap_pgm(mean_psnr) -> bytes:
    """A binary P5 image, one pixel per tile, of a [ty, tx] map of PSNR values: clamp(round(255 (50 - psnr) / 30), 0, 255) --
    black at 50 dB and above, white at 20 dB and below.  The formula defines the picture; it is not a measurement."""
    p = np.asarray(mean_psnr, np.float64)
    if p.ndim != 2:
        raise ValueError("heatmap_pgm needs a [ty, tx] map")
    v = np.clip(np.rint(255.0 * (50.0 - p) / 30.0), 0, 255).astype(np.uint8)
    return b"P5\n%d %d\n255\n" % (p.shape[1], p.shape[0]) + v.tobytes()


def analyse_plane(S, M_sum, width: int, height: int, tile: int, bit_depth: int, *, factor=16, min_mse=4.0,
                  share=0.9) -> dict:
    """What score_files reports for one plane of a clip: S uint64 [n, ty, tx] (the tile SSE of every frame) and M_sum uint64
    [ty, tx, 6] (the moments summed over the clip).  Returns {grid, defects, persistent, psnr_all, psnr_excluding,
    concentration_mean, tile_psnr_min_mean, worst_frame, columns, mean_psnr}; `columns` (the per-frame arrays of
    frame_summary) and `mean_psnr` (the PSNR of every tile over the clip, [ty, tx]) are for the caller, not for JSON."""
    counts = tile_counts(width, height, tile)
    n = S.shape[0]
    hot = hot_tiles(S, counts, factor=factor, min_mse=min_mse, tile=tile, bit_depth=bit_depth)
    defects = find_defects(S, counts, tile=tile, bit_depth=bit_depth, width=width, height=height, hot=hot)
    pers = persistent_regions(hot, S, counts, share=share, tile=tile, bit_depth=bit_depth, width=width, height=height)
    cols = frame_summary(S, width, height, tile, bit_depth)
    worst = int(np.argmin(cols["tile_psnr_min"])) if n else None
    mean_psnr = _psnr(tile_sse(M_sum), counts.astype(np.float64) * max(n, 1), bit_depth)
    return {"grid": [int(counts.shape[1]), int(counts.shape[0])], "defects": defects, "persistent": pers["regions"],
            "psnr_all": pers["psnr_all"], "psnr_excluding": pers["psnr_excluding"],
            "concentration_mean": float(cols["concentration"].mean()) if n else 0.0,
            "tile_psnr_min_mean": float(cols["tile_psnr_min"].mean()) if n else 0.0,
            "worst_frame": None if worst is None else {"frame": worst, "tile_psnr_min": float(cols["tile_psnr_min"][worst]),
                                                       "tile": [int(v) for v in cols["tile_psnr_min_at"][worst]]},
            "columns": cols, "mean_psnr": mean_psnr}


# ---- overlay masking: the node grid FeatureEngine.mask_blend takes (pqa_mask_blend, csrc/mask_blend.hip) ----------------------
# A grid of nodes 0 ... 256, `node` = 1 << step_log2 luma samples apart each way, ((size + node - 1) >> step_log2) + 1 of them
# along an axis; alpha at a sample is their bilinear interpolation (mask_alpha).  Chroma planes take the same grid at step_log2
# minus their shift: a chroma sample then sees the alpha of the luma sample it sits on.

MASK_FULL = 256


def _step_log2(node: int, chroma_shift=(0, 0)) -> int:
    node = int(node)
    if node < 1 or node > 64 or node & (node - 1):
        raise ValueError(f"node must be a power of two from 1 to 64, not {node}")
    s = node.bit_length() - 1
    for sh in chroma_shift:
        if int(sh) < 0 or s - int(sh) < 0:
            raise ValueError(f"nodes {node} samples apart cannot serve a chroma plane subsampled by {1 << int(sh)}")
    return s


def mask_alpha(nodes, width: int, height: int, step_log2_x: int, step_log2_y: int) -> np.ndarray:
    """int64 [height, width]: alpha 0 ... 256 of every sample of a plane under a node grid, as include/pqa_vmaf.h defines it"""
    A = np.asarray(nodes).astype(np.int64)
    sx, sy = int(step_log2_x), int(step_log2_y)
    gx, gy = 1 << sx, 1 << sy
    if A.shape != (((height + gy - 1) >> sy) + 1, ((width + gx - 1) >> sx) + 1):
        raise ValueError("node grid and plane size disagree")
    x, y = np.arange(width, dtype=np.int64), np.arange(height, dtype=np.int64)
    i, fx, j, fy = x >> sx, x & (gx - 1), y >> sy, y & (gy - 1)
    E0 = A[j] * (gy - fy)[:, None] + A[j + 1] * fy[:, None]      # [height, nodes along x]
    return (E0[:, i] * (gx - fx) + E0[:, i + 1] * fx + ((gx * gy) >> 1)) >> (sx + sy)


def grow_tiles(mask: np.ndarray, times: int) -> np.ndarray:
    """a bool map grown `times` times by its 8-neighbourhood"""
    m = np.asarray(mask, bool).copy()
    for _ in range(int(times)):
        p = np.pad(m, 1)
        m = np.zeros_like(m)
        for dj in range(3):
            for di in range(3):
                m |= p[dj:dj + m.shape[0], di:di + m.shape[1]]
    return m


def _mask_result(inside: np.ndarray, boxes, width: int, height: int, node: int, feather: int, step: int) -> dict:
    """the feathered grid around the nodes `inside`, and what the builders report about it"""
    feather = int(feather)
    if feather < 0 or feather % node:
        raise ValueError(f"feather {feather} is no multiple of the node step {node}")
    K = feather // node
    nodes = np.where(inside, MASK_FULL, 0).astype(np.uint16)
    reach = inside
    for s in range(1, K):      # Chebyshev distance s from the inside set
        wider = grow_tiles(reach, 1)
        nodes[wider & ~reach] = MASK_FULL - (MASK_FULL * s) // K
        reach = wider
    bounds = None
    js, is_ = np.nonzero(nodes)
    if len(js):      # node i weighs on the samples strictly between nodes i - 1 and i + 1
        bounds = [max(0, ((int(is_.min()) - 1) << step) + 1), max(0, ((int(js.min()) - 1) << step) + 1),
                  min(width, (int(is_.max()) + 1) << step), min(height, (int(js.max()) + 1) << step)]
        if bounds[0] >= bounds[2] or bounds[1] >= bounds[3]:
            bounds = None
    covered = int(np.count_nonzero(mask_alpha(nodes, width, height, step, step))) if bounds else 0
    return {"nodes": nodes, "step_log2": step, "boxes": boxes, "bounds": bounds, "share": covered / (width * height)}


def overlay_mask(tiles, width: int, height: int, tile: int, *, grow: int = 1, feather: int = 16, node: int = 8,
                 chroma_shift=(0, 0)) -> dict:
    """The node grid that masks the tiles `tiles` (bool [ty, tx] over tiles of `tile` x `tile` luma samples, e.g.
    persistent_tiles) out of a width x height picture, in integers.  The tiles are grown `grow` times by their 8-neighbourhood.
    A node is inside when its position (node gx, node gy) lies in the closed square [i tile, (i + 1) tile] x [j tile, (j + 1)
    tile] of a masked tile (i, j) -- a partial last tile counts with its full square -- so every sample of a masked tile has
    alpha = 256 exactly; `tile` must be a multiple of `node`.  Nodes at Chebyshev distance s node steps from the inside set,
    1 <= s < feather / node, hold 256 - (256 s) // (feather / node), all others 0; feather is a multiple of node, 0 (or node)
    is a hard edge.  chroma_shift: the (horizontal, vertical) subsampling the grid has to serve at step_log2 - shift.
    Returns {nodes uint16 [gy, gx], step_log2, boxes, bounds, share}: boxes the 4-neighbour components of the grown tiles as
    [x0, y0, x1, y1] in pixels, bounds the rectangle of the samples a non-zero node weighs on (None: there is none), share
    the exact fraction of samples with alpha > 0."""
    tile, width, height = int(tile), int(width), int(height)
    step = _step_log2(node, chroma_shift)
    if tile < 1 or tile % node:
        raise ValueError(f"tile {tile} is no multiple of the node step {node}")
    t = np.asarray(tiles, bool)
    if width < 1 or height < 1 or t.shape != (-(-height // tile), -(-width // tile)):
        raise ValueError("tile map and plane size disagree")
    if int(grow) < 0:
        raise ValueError("grow must not be negative")
    t = grow_tiles(t, grow)
    gy, gx = ((height + node - 1) >> step) + 1, ((width + node - 1) >> step) + 1
    inside = np.zeros((gy, gx), bool)
    r = tile // node
    for j, i in zip(*np.nonzero(t)):
        inside[j * r:(j + 1) * r + 1, i * r:(i + 1) * r + 1] = True      # slices past the grid's edge end there
    boxes = [_box(comp, tile, width, height) for comp in _components(t)]
    return _mask_result(inside, boxes, width, height, node, feather, step)


def overlay_mask_from_boxes(boxes, width: int, height: int, *, feather: int = 16, node: int = 8, chroma_shift=(0, 0)) -> dict:
    """The same grid from boxes [x0, y0, x1, y1] in luma pixels (x1, y1 exclusive) the user names.  A box is snapped outward
    to multiples of `node` and of the chroma step and its nodes are the inside set; nothing is grown.  `boxes` comes back
    snapped and clipped to the picture."""
    width, height = int(width), int(height)
    step = _step_log2(node, chroma_shift)
    if width < 1 or height < 1:
        raise ValueError("the picture has no samples")
    gy, gx = ((height + node - 1) >> step) + 1, ((width + node - 1) >> step) + 1
    inside = np.zeros((gy, gx), bool)
    out = []
    for b in boxes:
        if len(b) != 4:
            raise ValueError(f"a box is [x0, y0, x1, y1], not {list(b)}")
        x0, y0, x1, y1 = (int(v) for v in b)
        if not (0 <= x0 < x1 <= width and 0 <= y0 < y1 <= height):
            raise ValueError(f"box {[x0, y0, x1, y1]} is empty or leaves the {width}x{height} picture")
        gxs = [max(node, 1 << int(chroma_shift[0])), max(node, 1 << int(chroma_shift[1]))]
        x0, y0 = x0 // gxs[0] * gxs[0], y0 // gxs[1] * gxs[1]
        x1, y1 = -(-x1 // gxs[0]) * gxs[0], -(-y1 // gxs[1]) * gxs[1]
        inside[y0 >> step:(y1 >> step) + 1, x0 >> step:(x1 >> step) + 1] = True
        out.append([x0, y0, min(x1, width), min(y1, height)])
    return _mask_result(inside, out, width, height, node, feather, step)
