"""Temporal, spatial and level alignment on the host.  Spatial (best_shift, below the temporal part): from the shifted-window luma
SSE (FeatureEngine.shift_sse, pqa_shift_sse) to the whole-pixel displacement of the captured picture.  Levels (best_levels,
level_lut, at the end of this file): from the per-level transfer table (FeatureEngine.level_stats, pqa_level_stats) to the gain
and offset of the captured samples, the named range conversion they amount to and the table that undoes it; a transfer curve
(best_curve, curve_lut, behind them): the monotone curve of the same table and its inverse, for FeatureEngine.table_apply.  Colour (best_colour,
colour_correction, at the very end): from the cross-plane moments (FeatureEngine.colour_moments, pqa_colour_moments) to the 3 x 4 map of
the captured planes, the named matrix conversion it amounts to and the Q14 matrix that undoes it.  Active picture (active_picture, common_window, after the colour part): from the row and column profiles
(FeatureEngine.line_profiles, pqa_line_profiles) to the black bars of each clip and the rectangle both share.  Temporal: from the banded cross-frame SSE matrix (FeatureEngine.cross_sse, pqa_cross_sse) to a
constant frame offset and a per-frame map with repeated and dropped frames.

    D[i][c] = sum over luma pixels of (ref_i - dis_{i+k})^2,  k = k_lo + c;  UINT64_MAX where i + k is no captured frame

Sign convention: k > 0 means the capture is late -- captured frame i + k shows reference frame i.  Everything here is
Python-int / int64 arithmetic on exact integers, so a result does not depend on the machine, the rank or the run.

This replaces the reference's hand-tuned `frame_offset` spin box (app/bookend_alignment.py) and the "SSIM" / "Combined"
alignment methods its options tab offers and nothing implements."""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

SENTINEL = (1 << 64) - 1
# What one repeated or dropped frame costs in frame_map, as a mean squared error at 8 bit (scaled by 4^(bit_depth - 8)):
# leaving the straight path must pay for itself by more than an MSE of 25 (a PSNR of about 34 dB) on one frame.  A real
# repeat or drop saves the whole difference between two different pictures on EVERY later frame, orders of magnitude more
# on moving content; noise between two captures of the same picture stays well below.  An option value, not a constant of
# the method.
DEFAULT_PENALTY_MSE = 25.0


def _key(k: int):
    """the tie order of offsets: the smaller |k| first, then the negative one"""
    return (abs(k), k)


def _band(D, k_lo):
    D = np.asarray(D)
    if D.ndim != 2 or D.shape[1] < 1:
        raise ValueError("D must be [n_ref, span]")
    span = D.shape[1]
    if k_lo is None:
        if span % 2 == 0:
            raise ValueError("k_lo is needed for a band with an even number of offsets")
        k_lo = -(span // 2)
    return D, int(k_lo), span


def best_offset(D, n_pixels: int, min_overlap: int | None = None, *, k_lo: int | None = None, n_dis: int | None = None):
    """(k, mse_at_k, confidence) of the constant offset with the smallest mean of D over its valid rows.

    D is [n_ref, span] (k_lo defaults to the symmetric band -(span // 2)).  Only offsets with at least `min_overlap` valid
    rows compete; the default is half of the shorter clip (n_dis defaults to the number of captured frames D can see).
    Ties go to the smaller |k|, then to the negative k.  The means are compared as exact fractions.  `confidence` is the
    second-smallest mean divided by the smallest (inf at a smallest of 0, or when one offset qualifies and it is 0; 1.0
    when one offset qualifies and it is not).  ValueError when no offset qualifies."""
    D, k_lo, span = _band(D, k_lo)
    n_ref = D.shape[0]
    valid = D != np.uint64(SENTINEL)
    if n_dis is None:   # the captured frames the band shows to exist
        rows, cols = np.nonzero(valid)
        n_dis = int((rows + cols).max()) + k_lo + 1 if len(rows) else 0
    if min_overlap is None:
        min_overlap = max(1, min(n_ref, n_dis) // 2)
    cands = []
    for c in range(span):
        rows = np.flatnonzero(valid[:, c])
        if len(rows) < max(1, int(min_overlap)):
            continue
        total = sum(int(v) for v in D[rows, c])
        cands.append((total, len(rows), k_lo + c))
    if not cands:
        raise ValueError(f"no offset in {k_lo} ... {k_lo + span - 1} has {min_overlap} overlapping frames")

    def less(a, b):   # mean a < mean b, exactly; ties by the offset's key
        la, lb = a[0] * b[1], b[0] * a[1]
        return la < lb or (la == lb and _key(a[2]) < _key(b[2]))
    best = cands[0]
    for cnd in cands[1:]:
        if less(cnd, best):
            best = cnd
    rest = [cnd for cnd in cands if cnd is not best]
    mse = best[0] / (best[1] * float(n_pixels))
    if best[0] == 0:
        conf = float("inf")
    elif not rest:
        conf = 1.0
    else:
        second = rest[0]
        for cnd in rest[1:]:
            if less(cnd, second):
                second = cnd
        conf = (second[0] * best[1]) / (second[1] * best[0])
    return best[2], mse, conf


def default_penalty(n_pixels: int, bit_depth: int = 8, penalty_mse: float | None = None) -> int:
    """the integer cost of one repeated or dropped frame: penalty_mse * n_pixels, rounded once"""
    if penalty_mse is None:
        penalty_mse = DEFAULT_PENALTY_MSE * 4.0 ** (int(bit_depth) - 8)
    return int(round(float(penalty_mse) * int(n_pixels)))


def frame_map(D, n_dis: int, penalty_mse: float | None = None, n_pixels: int = 1, *, k_lo: int | None = None,
              bit_depth: int = 8, first: int = 0, last: int | None = None):
    """The cheapest path of offsets k_j over the captured frames j = first ... last - 1 (default: all n_dis of them).

    State k_j costs D[j - k_j][k_j - k_lo] (the reference frame j - k_j must exist).  Steps: k_j = k_{j-1} (both clips
    advance, free), k_j = k_{j-1} + 1 (the capture repeats a frame: the reference index stays), k_j = k_{j-1} - d (d
    reference frames were dropped); a step costs P = round(penalty_mse * n_pixels) per repeated or dropped frame.
    `penalty_mse` defaults to DEFAULT_PENALTY_MSE * 4^(bit_depth - 8).  All sums are Python ints.

    Tie rule: among paths of equal total cost the one whose offsets, read from the LAST captured frame backwards, come
    first in the order (smaller |k|, then negative k) wins.

    Returns (ref_index, repeated, dropped): ref_index[j - first] is the reference frame captured frame j shows, `repeated`
    the captured frame numbers that repeat their predecessor, `dropped` the reference frame numbers no captured frame
    shows because the path jumped over them.  ValueError when a captured frame has no valid state."""
    D, k_lo, span = _band(D, k_lo)
    n_ref = D.shape[0]
    last = int(n_dis) if last is None else int(last)
    first = int(first)
    if not (0 <= first <= last <= n_dis):
        raise ValueError("bad captured frame range")
    P = default_penalty(n_pixels, bit_depth, penalty_mse)
    ks = list(range(k_lo, k_lo + span))

    def cost(j, k):
        i = j - k
        if i < 0 or i >= n_ref:
            return None
        v = int(D[i, k - k_lo])
        return None if v == SENTINEL else v
    V, back = [], []   # V[t][s]: cheapest path to state s at frame first + t (None: unreachable)
    for t, j in enumerate(range(first, last)):
        row, brow = [None] * span, [None] * span
        for s, k in enumerate(ks):
            cj = cost(j, k)
            if cj is None:
                continue
            if t == 0:
                row[s] = cj
                continue
            best = None
            for sp, kp in enumerate(ks):
                vp = V[t - 1][sp]
                if vp is None:
                    continue
                if k == kp:
                    step = 0
                elif k == kp + 1:
                    step = P
                elif k < kp:
                    step = (kp - k) * P
                else:
                    continue
                cand = (vp + step, _key(kp), sp)
                if best is None or cand[:2] < best[:2]:
                    best = cand
            if best is not None:
                row[s] = best[0] + cj
                brow[s] = best[2]
        if all(v is None for v in row):
            raise ValueError(f"captured frame {j} has no valid state in the band {k_lo} ... {k_lo + span - 1}")
        V.append(row)
        back.append(brow)
    if not V:
        return [], [], []
    s = min((s for s in range(span) if V[-1][s] is not None), key=lambda s: (V[-1][s], _key(ks[s])))
    path = [0] * len(V)
    for t in range(len(V) - 1, -1, -1):
        path[t] = ks[s]
        if t > 0:
            s = back[t][s]
    ref_index = [first + t - k for t, k in enumerate(path)]
    repeated, dropped = [], []
    for t in range(1, len(path)):
        if path[t] == path[t - 1] + 1:
            repeated.append(first + t)
        elif path[t] < path[t - 1]:
            dropped.extend(range(ref_index[t - 1] + 1, ref_index[t]))
    return ref_index, repeated, dropped


def path_cost(D, ks_path, n_pixels: int = 1, penalty_mse: float | None = None, *, k_lo: int | None = None,
              bit_depth: int = 8, first: int = 0):
    """The total cost frame_map assigns to the offsets `ks_path` of captured frames first ..., or None when the path is not
    legal (a state without a reference frame, a step that is not allowed).  What frame_map minimises, stated once more."""
    D, k_lo, span = _band(D, k_lo)
    P = default_penalty(n_pixels, bit_depth, penalty_mse)
    total = 0
    for t, k in enumerate(ks_path):
        i = first + t - k
        if not (k_lo <= k < k_lo + span) or i < 0 or i >= D.shape[0] or int(D[i, k - k_lo]) == SENTINEL:
            return None
        total += int(D[i, k - k_lo])
        if t > 0:
            kp = ks_path[t - 1]
            if k == kp + 1:
                total += P
            elif k < kp:
                total += (kp - k) * P
            elif k != kp:
                return None
    return total


def align(D, n_ref: int, n_dis: int, n_pixels: int, *, k_lo: int, fps: float = 0.0, bit_depth: int = 8,
          penalty_mse: float | None = None, min_overlap: int | None = None) -> dict:
    """best_offset and frame_map of one matrix as the `alignment` object of a result: {offset_frames, offset_seconds, mse,
    confidence, repeated, dropped, searched}.  The frame map runs over the captured frames that have a reference frame
    under the offset found, widened by nothing: frames in front of the reference's first picture are the offset itself."""
    D, k_lo, span = _band(D, k_lo)
    k, mse, conf = best_offset(D, n_pixels, min_overlap, k_lo=k_lo, n_dis=n_dis)
    j0, j1 = max(0, k), min(n_dis, D.shape[0] + k)
    try:
        _, repeated, dropped = frame_map(D, n_dis, penalty_mse, n_pixels, k_lo=k_lo, bit_depth=bit_depth, first=j0, last=j1)
    except ValueError:
        repeated, dropped = [], []
    return {"offset_frames": int(k), "offset_seconds": (k / fps if fps else 0.0), "mse": float(mse),
            "confidence": float(conf), "repeated": [int(j) for j in repeated], "dropped": [int(i) for i in dropped],
            "searched": [int(k_lo), int(k_lo + span - 1)]}


# ---- spatial alignment -----------------------------------------------------------------------------------------------------
def _shift_key(p: int, dx: int, dy: int):
    """the tie order of shifts: the smaller error, then the shorter shift, then the smaller |dy|, then dy, then dx"""
    return (p, dx * dx + dy * dy, abs(dy), dy, dx)


def _argmin_shift(P, R: int):
    return min(((dx, dy) for dy in range(-R, R + 1) for dx in range(-R, R + 1)),
               key=lambda s: _shift_key(P[s[1] + R][s[0] + R], s[0], s[1]))


def _parabola(lo: int, mid: int, hi: int):
    """vertex of the parabola through (-1, lo), (0, mid), (1, hi), relative to 0; None when it has no minimum"""
    den = lo - 2 * mid + hi
    return (lo - hi) / (2.0 * den) if den > 0 else None


def best_shift(S, radius: int, n_pixels: int = 1) -> dict:
    """The whole-pixel displacement (dx, dy) of the captured picture from S[n_frames][2R + 1][2R + 1] (pqa_shift_sse):
    S[f][j][i] is the squared error of frame pair f with the capture read at (x + i - R, y + j - R), so dx > 0 means the
    captured picture sits to the right of the reference's, dy > 0 below it.

    The frames are pooled, P = sum over f of S[f] in Python ints, and the minimum is taken with the tie key (P, dx^2 + dy^2,
    |dy|, dy, dx).  Returns {dx, dy, mse, confidence, agreement, at_edge, subpixel_dx, subpixel_dy, searched}:
    mse = P / (n_frames * n_pixels), n_pixels = (W - 2R)(H - 2R), the pixels one entry of S sums;
    confidence = (the smallest P outside the 3 x 3 neighbourhood of the minimum) / (P at the minimum): inf when the minimum
    is 0 and that one is not, 1.0 when both are 0 or the search has no entry outside the neighbourhood;
    agreement = the share of the frames whose own minimum under the same key is (dx, dy);
    at_edge = |dx| == R or |dy| == R: a minimum on the border of the search is not a minimum;
    subpixel_dx / subpixel_dy = the vertex of the three-point parabola through P along each axis, relative to the minimum
    (-0.5 ... 0.5; informational: a steady +-0.5 hints at scaling, which a shift does not correct), None when at_edge or
    when the three points have no minimum;  searched = R."""
    S = np.asarray(S)
    R = int(radius)
    if R < 0 or S.ndim != 3 or S.shape[0] < 1 or S.shape[1:] != (2 * R + 1, 2 * R + 1):
        raise ValueError("S must be [n_frames >= 1, 2R + 1, 2R + 1]")
    n = S.shape[0]
    frames = [[[int(v) for v in row] for row in S[f]] for f in range(n)]
    P = [[sum(frames[f][j][i] for f in range(n)) for i in range(2 * R + 1)] for j in range(2 * R + 1)]
    dx, dy = _argmin_shift(P, R)
    best = P[dy + R][dx + R]
    outside = [P[j][i] for j in range(2 * R + 1) for i in range(2 * R + 1) if abs(j - R - dy) > 1 or abs(i - R - dx) > 1]
    if not outside:
        conf = 1.0
    elif best == 0:
        conf = float("inf") if min(outside) > 0 else 1.0
    else:
        conf = min(outside) / best
    at_edge = abs(dx) == R or abs(dy) == R
    sub_x = sub_y = None
    if not at_edge:
        sub_x = _parabola(P[dy + R][dx + R - 1], best, P[dy + R][dx + R + 1])
        sub_y = _parabola(P[dy + R - 1][dx + R], best, P[dy + R + 1][dx + R])
    return {"dx": int(dx), "dy": int(dy), "mse": best / (float(n) * float(n_pixels)), "confidence": float(conf),
            "agreement": sum(1 for f in range(n) if _argmin_shift(frames[f], R) == (dx, dy)) / float(n),
            "at_edge": bool(at_edge), "subpixel_dx": sub_x, "subpixel_dy": sub_y, "searched": R}


# ---- level alignment -------------------------------------------------------------------------------------------------------
LEVEL_MAPS = ("identity", "limited_to_full", "full_to_limited")


def named_level_map(name: str, bit_depth: int, chroma: bool = False):
    """(a, b) of the fixed map dis = a * ref + b, as Fractions, s = 2^(bit_depth - 8):
    identity a = 1, b = 0;  limited_to_full luma a = 255/219, b = -16 s * 255/219, chroma a = 255/224 about 128 s;
    full_to_limited luma a = 219/255, b = 16 s, chroma a = 224/255 about 128 s."""
    s = 1 << (int(bit_depth) - 8)
    if name == "identity":
        return Fraction(1), Fraction(0)
    if name not in LEVEL_MAPS:
        raise ValueError(f"unknown level map {name!r}")
    if chroma:
        a = Fraction(255, 224) if name == "limited_to_full" else Fraction(224, 255)
        return a, 128 * s * (1 - a)
    if name == "limited_to_full":
        return Fraction(255, 219), Fraction(-16 * s * 255, 219)
    return Fraction(219, 255), Fraction(16 * s)


def _fit(levels, T0, T1):
    """least-squares (a, b) of dis = a * ref + b over `levels` from the counts and sums; None when no slope can be formed"""
    n = sum(T0[v] for v in levels)
    sr = sum(v * T0[v] for v in levels)
    sd = sum(T1[v] for v in levels)
    srr = sum(v * v * T0[v] for v in levels)
    srd = sum(v * T1[v] for v in levels)
    den = n * srr - sr * sr
    if n == 0 or den == 0:
        return None
    a = Fraction(n * srd - sr * sd, den)
    return a, (Fraction(sd) - a * sr) / n


def _map_sse(a, b, top, T0, T1, T2):
    """sum over the pixels of (dis - clamp(a * ref + b, 0, top))^2, exact: what is left when the capture chain applied the
    map and clipped to its range"""
    sse = Fraction(0)
    for v, c in enumerate(T0):
        if c:
            p = min(max(a * v + b, 0), top)
            sse += T2[v] - 2 * p * T1[v] + p * p * c
    return sse


def _levels_exact(T, bit_depth: int, chroma: bool, min_improvement: float, snap: float):
    """(the best_levels() result, what best_curve() goes on with in exact numbers: the pooled columns T0 / T1 / T2, n_pix, the
    fitted gain, the MSE of the chosen map and of the identity)"""
    T = np.asarray(T)
    L = 1 << int(bit_depth)
    if T.ndim != 3 or T.shape[0] < 1 or T.shape[1:] != (L, 3):
        raise ValueError("T must be [n_frames >= 1, 2^bit_depth, 3]")
    top = L - 1
    T0, T1, T2 = ([sum(int(x) for x in T[:, v, k]) for v in range(L)] for k in range(3))
    n_pix = sum(T0)
    if n_pix == 0:
        raise ValueError("T counts no pixel")
    populated = [v for v in range(L) if T0[v]]

    def mse(a, b):
        return _map_sse(a, b, top, T0, T1, T2) / n_pix
    named = {k: mse(*named_level_map(k, bit_depth, chroma)) for k in LEVEL_MAPS}
    curve = sum(Fraction(T2[v]) - Fraction(T1[v] * T1[v], T0[v]) for v in populated) / n_pix
    fit = _fit(populated, T0, T1) if len(populated) >= 2 else None
    degenerate = fit is None
    used = populated
    if degenerate:
        a, b = Fraction(1), Fraction(0)
    else:
        a, b = fit
        inside = [v for v in populated if 1 <= a * v + b <= top - 1]
        refit = _fit(inside, T0, T1) if len(inside) >= 2 else None
        if refit is not None:
            (a, b), used = refit, inside
    mse_affine = mse(a, b)
    kind = "identity" if degenerate else min(LEVEL_MAPS, key=lambda k: named[k])     # min keeps the first of equals
    chosen = named[kind]
    if not degenerate and chosen > Fraction(snap) * mse_affine:
        kind, chosen = "affine", mse_affine
    ma, mb = (a, b) if kind == "affine" else named_level_map(kind, bit_depth, chroma)
    out = {"gain": float(a), "offset": float(b), "kind": kind,
           "mismatch": bool(not degenerate and named["identity"] > Fraction(min_improvement) * chosen),
           "mse_identity": float(named["identity"]), "mse_affine": float(mse_affine), "mse_curve": float(curve),
           "named": {k: float(x) for k, x in named.items()}, "map_gain": float(ma), "map_offset": float(mb),
           "levels_used": len(used), "frames": int(T.shape[0]), "degenerate": bool(degenerate)}
    return out, {"T0": T0, "T1": T1, "T2": T2, "n_pix": n_pix, "gain": a, "chosen": chosen, "identity": named["identity"]}


def best_levels(T, bit_depth: int, *, chroma: bool = False, min_improvement: float = 2.0, snap: float = 1.25) -> dict:
    """The level mapping of a captured plane from T[n_frames][L][3] (pqa_level_stats; L = 2^bit_depth): T[f][v] = (count, sum
    of dis, sum of dis^2) over the pixels whose reference sample is v.  The frames are pooled; everything below is Python
    ints and Fractions, converted to float only in the result.  top = L - 1.

    gain, offset: the least-squares a, b of dis = a * ref + b from the joint moments, refitted once over only those populated
    reference levels whose predicted captured value a * v + b lies in [1, top - 1], so that clipping at 0 or top does not
    bias the fit (the first fit is kept when fewer than two such levels remain).  levels_used = the levels of the final fit.
    The MSE of a map (a, b) is taken against clamp(a * v + b, 0, top).  mse_identity; mse_affine (the fitted map);
    mse_curve = sum_v (T2 - T1^2 / T0) / N, the residual about the conditional mean: the floor any per-level correction
    could reach.  named = {identity, limited_to_full, full_to_limited: MSE under named_level_map()}.
    kind = the named map with the smallest MSE (ties: the order above), or "affine" when that MSE exceeds snap * mse_affine.
    mismatch = mse_identity > min_improvement * (MSE of the chosen map).  map_gain / map_offset = the chosen map's a, b (the
    named map's own values, or the fitted ones): what correction_lut() undoes.
    degenerate = fewer than two reference levels are populated: no fit is made, gain = 1, offset = 0, kind = "identity",
    mismatch false.  frames = n_frames."""
    return _levels_exact(T, bit_depth, chroma, min_improvement, snap)[0]


def level_lut(gain, offset, bit_depth: int) -> np.ndarray:
    """The inverse of dis = gain * ref + offset as an integer table over the captured levels:
    lut[d] = clamp(floor((d - offset) / gain + 1/2), 0, top), top = 2^bit_depth - 1, computed in Fractions (a float argument
    is taken at its exact binary value; pass named_level_map()'s Fractions for a named map).  uint8 at 8 bit, else uint16."""
    a, b = Fraction(gain), Fraction(offset)
    if a <= 0:
        raise ValueError("level_lut needs a positive gain")
    top = (1 << int(bit_depth)) - 1
    half = Fraction(1, 2)
    lut = [min(max(((d - b) / a + half).__floor__(), 0), top) for d in range(top + 1)]
    return np.asarray(lut, np.uint8 if bit_depth <= 8 else np.uint16)


def correction_lut(levels: dict, bit_depth: int, chroma: bool = False) -> np.ndarray:
    """level_lut() of the map a best_levels() result chose: a named kind with its exact a and b, "affine" with the fit"""
    if levels["kind"] in LEVEL_MAPS:
        return level_lut(*named_level_map(levels["kind"], bit_depth, chroma), bit_depth)
    return level_lut(levels["gain"], levels["offset"], bit_depth)


# ---- transfer-curve alignment ------------------------------------------------------------------------------------------------
# A gamma leg, a contrast enhancer or a black stretch is no gain and offset: the forward table T of pqa_level_stats is turned
# into a monotone curve g (captured level as a function of the reference level) and its inverse as an integer table, which
# FeatureEngine.table_apply puts the captured planes through.  The forward direction is deliberate: E[dis | ref = v] is unbiased
# under dis = g(ref) + noise, whereas E[ref | dis] shrinks towards the mean under coding noise and would "correct" a clip whose
# levels are fine.
def table_sse(T) -> int:
    """sum over the frames and levels of T2 - 2 v T1 + v^2 T0, a Python int: the squared error of the pairs T was made from"""
    T = np.asarray(T)
    return sum(int(T[f, v, 2]) - 2 * v * int(T[f, v, 1]) + v * v * int(T[f, v, 0]) for f in range(T.shape[0]) for v in range(T.shape[1]))


def isotonic(values, weights) -> list:
    """The weighted isotonic regression (non-decreasing) of `values`, as Fractions: pool adjacent violators.  A block is pooled
    with its predecessor only while its mean is strictly below the predecessor's, so equal means stay blocks of their own."""
    blocks = []   # [sum of weight * value, sum of weight, members]
    for x, w in zip(values, weights):
        w = Fraction(w)
        if w <= 0:
            raise ValueError("isotonic needs positive weights")
        blocks.append([Fraction(x) * w, w, 1])
        while len(blocks) > 1 and blocks[-1][0] * blocks[-2][1] < blocks[-2][0] * blocks[-1][1]:
            s, w1, n = blocks.pop()
            blocks[-1][0] += s
            blocks[-1][1] += w1
            blocks[-1][2] += n
    out = []
    for s, w, n in blocks:
        out += [s / w] * n
    return out


def _curve(T0, T1, top: int, min_count: int):
    """(knots, g over every level 0 ... top as Fractions) of the pooled columns T0 / T1, or None when no curve can be formed:
    fewer than two knots, or a g that is constant over them"""
    knots = [v for v in range(top + 1) if T0[v] >= max(1, int(min_count))]
    if len(knots) < 2:
        return None
    gk = isotonic([Fraction(T1[v], T0[v]) for v in knots], [T0[v] for v in knots])
    if gk[0] == gk[-1]:
        return None
    g = [None] * (top + 1)
    for v in range(knots[0]):                        # slope 1 outside the knots, clamped to the range
        g[v] = max(Fraction(0), gk[0] - (knots[0] - v))
    for v in range(knots[-1] + 1, top + 1):
        g[v] = min(Fraction(top), gk[-1] + (v - knots[-1]))
    for (v0, g0), (v1, g1) in zip(zip(knots, gk), zip(knots[1:], gk[1:])):
        step = (g1 - g0) / (v1 - v0)
        for v in range(v0, v1):
            g[v] = g0 + step * (v - v0)
    g[knots[-1]] = gk[-1]
    return knots, g


def _pooled(T, bit_depth: int):
    T = np.asarray(T)
    L = 1 << int(bit_depth)
    if T.ndim != 3 or T.shape[0] < 1 or T.shape[1:] != (L, 3):
        raise ValueError("T must be [n_frames >= 1, 2^bit_depth, 3]")
    return ([sum(int(x) for x in T[:, v, k]) for v in range(L)] for k in range(3))


def _curve_gamma(knots, g, T0, lo: int, hi: int):
    """the T0-weighted least-squares slope of ln g against ln v, both normalised to (lo, hi), over the knots strictly inside on
    both axes; a float, or None when fewer than two such knots exist"""
    pts = []
    for v in knots:
        x, y = (v - lo) / (hi - lo), float((g[v] - lo) / (hi - lo))
        if 0 < x < 1 and 0 < y < 1:
            pts.append((math.log(x), math.log(y), float(T0[v])))
    n = sum(w for _, _, w in pts)
    if len(pts) < 2:
        return None
    mx, my = sum(w * x for x, _, w in pts) / n, sum(w * y for _, y, w in pts) / n
    sxx = sum(w * (x - mx) ** 2 for x, _, w in pts)
    return None if sxx <= 0 else sum(w * (x - mx) * (y - my) for x, y, w in pts) / sxx


def best_curve(T, bit_depth: int, *, chroma: bool = False, full_range: bool = True, min_count: int = 16, curve_snap: float = 1.1,
               curve_min_gain: float = 0.5, min_improvement: float = 2.0, snap: float = 1.25) -> dict:
    """best_levels() of T[n_frames][L][3] (pqa_level_stats, pooled over the frames), and on top of it the monotone transfer
    curve g of the captured levels on the reference's.  Exact ints and Fractions up to the floats of the result.

    Knots are the reference levels v with T0[v] >= min_count; g at the knots is the T0-weighted isotonic regression
    (isotonic(): non-decreasing) of the conditional means T1 / T0; between knots g is linear, below the first and above the
    last it continues with slope 1, clamped to [0, top].  curve_degenerate = no curve is formed: fewer than two knots, a g
    that is constant, a best_levels() result that is degenerate, or a fitted gain that is not positive (the capture does not
    follow the reference at all: independent pictures).  knots = the number of knots.
    mse_monotone = sum_v (T2 - 2 g T1 + g^2 T0) / N: it lies between mse_curve (the floor) and mse_affine wherever every
    populated level is a knot.  None when curve_degenerate.
    kind becomes "curve" when the MSE of the map best_levels() chose exceeds curve_snap * mse_monotone AND exceeds mse_monotone
    by at least curve_min_gain * 4^(bit_depth - 8); the second condition keeps noise-free affine clips, whose only residual is
    rounding (about 1/12), out of "curve".  mismatch is then mse_identity > min_improvement * mse_monotone.  Otherwise the
    best_levels() result stands as it is.
    gamma: a float, reported only -- the T0-weighted least-squares slope of ln g against ln v over the interior knots, both
    normalised to (0, top), or to (16 s, 235 s) with full_range=False, s = 2^(bit_depth - 8) as in named_level_map; None for
    a chroma plane, when curve_degenerate, or with fewer than two interior knots."""
    out, ex = _levels_exact(T, bit_depth, chroma, min_improvement, snap)
    T0, T1, T2, n_pix = ex["T0"], ex["T1"], ex["T2"], ex["n_pix"]
    top = (1 << int(bit_depth)) - 1
    cv = None if out["degenerate"] or ex["gain"] <= 0 else _curve(T0, T1, top, min_count)
    out.update(mse_monotone=None, knots=0, gamma=None, curve_degenerate=cv is None)
    if cv is None:
        return out
    knots, g = cv
    mono = sum(T2[v] - 2 * g[v] * T1[v] + g[v] * g[v] * T0[v] for v in range(top + 1) if T0[v]) / n_pix
    s = 1 << (int(bit_depth) - 8)
    lo, hi = (0, top) if full_range else (16 * s, 235 * s)
    out.update(mse_monotone=float(mono), knots=len(knots), gamma=None if chroma else _curve_gamma(knots, g, T0, lo, hi))
    if ex["chosen"] > Fraction(curve_snap) * mono and ex["chosen"] - mono >= Fraction(curve_min_gain) * s * s:
        out.update(kind="curve", mismatch=bool(ex["identity"] > Fraction(min_improvement) * mono))
    return out


def curve_lut(T, bit_depth: int, min_count: int = 16) -> np.ndarray:
    """The inverse of best_curve()'s g as an integer table over the captured levels d = 0 ... top (uint8 at 8 bit, else uint16):
    what FeatureEngine.table_apply puts a captured plane through.  For every d:
      1. the v whose g(v) is nearest d -- the candidates are the last v with g(v) <= d (v = 0 when there is none) and its
         successor; the lower one wins a tie;
      2. that v widened to the whole run of levels with the same g (a plateau: clipped or crushed levels);
      3. the entry is the T0-weighted mean of the run, rounded half up, or the run's midpoint (rounded half up) when the run
         holds no pixel.
    Non-decreasing by construction.  ValueError when no curve can be formed (best_curve(): curve_degenerate)."""
    T0, T1, _ = _pooled(T, bit_depth)
    top = (1 << int(bit_depth)) - 1
    cv = _curve(T0, T1, top, min_count)
    if cv is None:
        raise ValueError("curve_lut: no curve can be formed from this table")
    g = cv[1]
    run_of, entry = [0] * (top + 1), []     # level -> index of its run; run -> its entry
    v = 0
    while v <= top:
        e = v
        while e < top and g[e + 1] == g[v]:
            e += 1
        n = sum(T0[v:e + 1])
        num, den = (sum(u * T0[u] for u in range(v, e + 1)), n) if n else (v + e, 2)
        entry.append((2 * num + den) // (2 * den))
        for u in range(v, e + 1):
            run_of[u] = len(entry) - 1
        v = e + 1
    lut, v = [], 0
    for d in range(top + 1):
        while v < top and g[v + 1] <= d:    # the last v with g(v) <= d; g is non-decreasing, and so is v in d
            v += 1
        pick = v + 1 if v < top and g[v] <= d and g[v + 1] - d < d - g[v] else v
        lut.append(entry[run_of[pick]])
    assert all(a <= b for a, b in zip(lut, lut[1:])), "curve_lut: the table must be non-decreasing"
    return np.asarray(lut, np.uint8 if bit_depth <= 8 else np.uint16)


# ---- sub-pixel and scale registration ------------------------------------------------------------------------------------------
# The map of one axis of n samples, in edge coordinates X = x + 1/2:  X_dis = n/2 + s (X_ref - n/2) + d.  d > 0: the captured
# picture is displaced to the right (down), as in best_shift; s > 1: it is larger.  The captured clip resampled onto the
# reference grid is a same-size pqa_resample call with the source window x0 = d + n (1 - s) / 2, w = n s.  The state of the
# iteration is that window as Q16 integers, nothing else: every step below is a function of integers.
Q16 = 65536
REGISTER_STOP_PX = Fraction(1, 64)   # an increment that moves no frame corner this far ends the iteration at a level


def _round_q16(v: Fraction) -> int:
    return (Fraction(v) * Q16 + Fraction(1, 2)).__floor__()


def geometry_window(d, s, n: int):
    """(x0_q16, w_q16) of the map (d, s) of an axis of n samples: x0 = d + n (1 - s) / 2 and w = n s, each rounded to Q16
    (half up); d and s are taken as exact Fractions"""
    d, s = Fraction(d), Fraction(s)
    return _round_q16(d + n * (1 - s) / 2), _round_q16(n * s)


def window_geometry(x0_q16: int, w_q16: int, n: int):
    """(d, s) as Fractions of the window (x0_q16, w_q16) of an axis of n samples: the inverse of geometry_window, exact"""
    s = Fraction(int(w_q16), Q16 * n)
    return Fraction(int(x0_q16), Q16) - n * (1 - s) / 2, s


def compose_geometry(d, s, a, e):
    """(d + s a, s (1 + e)): the map (d, s) after the increment u = a + e p was measured on the clip resampled through it
    (p: the distance from the frame centre); Fractions, not quantised"""
    d, s, a, e = Fraction(d), Fraction(s), Fraction(a), Fraction(e)
    return d + s * a, s * (1 + e)


def _solve_fractions(A, b):
    """x of A x = b by Gaussian elimination in Fractions; None when A is singular"""
    n = len(b)
    rows = [[Fraction(v) for v in A[i]] + [Fraction(b[i])] for i in range(n)]
    for c in range(n):
        piv = next((r for r in range(c, n) if rows[r][c] != 0), None)
        if piv is None:
            return None
        rows[c], rows[piv] = rows[piv], rows[c]
        for r in range(n):
            if r != c and rows[r][c] != 0:
                k = rows[r][c] / rows[c][c]
                rows[r] = [x - k * y for x, y in zip(rows[r], rows[c])]
    return [rows[i][n] / rows[i][i] for i in range(n)]


def _tile_centres(n: int, tile: int):
    """per tile of an axis of n samples: the centre of its counted pixels (1 ... n - 2) relative to the frame centre, in edge
    coordinates -- (lo + hi + 1) / 2 - n / 2 --, or None when it counts no pixel"""
    out = []
    for i in range(-(-n // tile)):
        lo, hi = max(1, i * tile), min(n - 2, (i + 1) * tile - 1)
        out.append(Fraction(lo + hi + 1 - n, 2) if lo <= hi else None)
    return out


def solve_geometry(M, width: int, height: int, tile: int):
    """The increment (a_x, e_x, a_y, e_y), as Fractions, from the tile moments M[ty][tx][6] = sum gx^2, gx gy, gy^2, gx dt,
    gy dt, dt^2 (pqa_flow_moments, summed over the frames): the remaining displacement of the captured picture is modelled
    as u = a_x + e_x px, v = a_y + e_y py at the tile centre (px, py), relative to the frame centre, and
    sum over tiles and pixels of (dt + gx u + gy v)^2 is minimised -- a 4 x 4 system in Fractions.  gx, gy and dt all carry
    the factor 16 of their stencils, so the result is in pixels.  None when the system is singular: fewer than two tile
    columns or rows that carry gradient, or a flat picture."""
    M = np.asarray(M)
    cxs, cys = _tile_centres(int(width), int(tile)), _tile_centres(int(height), int(tile))
    if M.shape != (len(cys), len(cxs), 6):
        raise ValueError(f"M must be [{len(cys)}, {len(cxs)}, 6] for {width}x{height} at tile {tile}")
    A = [[Fraction(0)] * 4 for _ in range(4)]
    b = [Fraction(0)] * 4
    for j, py in enumerate(cys):
        for i, px in enumerate(cxs):
            if px is None or py is None:
                continue
            gxx, gxy, gyy, gxt, gyt = (int(v) for v in M[j, i, :5])
            basis = ((1, px), (1, py))           # u = basis[0] . (a_x, e_x), v = basis[1] . (a_y, e_y)
            G = ((gxx, gxy), (gxy, gyy))
            for p in range(2):
                for q in range(2):
                    for m in range(2):
                        for k in range(2):
                            A[2 * p + m][2 * q + k] += G[p][q] * basis[p][m] * basis[q][k]
                for m in range(2):
                    b[2 * p + m] += (gxt, gyt)[p] * basis[p][m]
    sol = _solve_fractions(A, [-v for v in b])
    return None if sol is None else tuple(sol)


def _corner_sq(ax, ex, ay, ey, w, h):
    """the largest squared displacement u^2 + v^2 over the four frame corners of u = ax + ex px, v = ay + ey py"""
    return max((ax + sx * ex * w / 2) ** 2 + (ay + sy * ey * h / 2) ** 2 for sx in (-1, 1) for sy in (-1, 1))


def register_levels(width: int, height: int, tile: int, levels=None):
    """[(level l, tile at l)] from the coarsest level to 0.  levels = None: the largest l <= 4 at which the (width >> l) x
    (height >> l) plane still holds 4 whole tiles each way, the tile halved down to 8 where that takes; an int: that l."""
    def tile_at(l):
        t = int(tile)
        while t > 8 and ((width >> l) // t < 4 or (height >> l) // t < 4):
            t //= 2
        return t
    if levels is None:
        levels = next((l for l in range(4, 0, -1) if (width >> l) // tile_at(l) >= 4 and (height >> l) // tile_at(l) >= 4), 0)
    if not 0 <= int(levels) <= 4:
        raise ValueError("levels must be None or 0 ... 4")
    return [(l, tile_at(l)) for l in range(int(levels), -1, -1)]


def geometry_applied(geometry: dict, min_px: float = 1.0 / 16) -> bool:
    """whether a register() result is worth undoing: it converged, it moves a frame corner by min_px at least, and the last
    full-resolution pass left less error than the first"""
    return bool(geometry["converged"] and geometry["corner_px"] >= min_px and geometry["mse_after"] < geometry["mse_before"])


def register(moments, resample, ref, dis, *, filter: str = "bicubic", tile: int = 32, levels=None, max_iters: int = 5,
             trace=None) -> dict:
    """Sub-pixel shift and scale of the captured luma planes `dis` against `ref` (two lists of 2-D arrays of one size),
    coarse to fine.  The two callables do the device work -- moments(ref_planes, dis_planes, tile) -> [n, ty, tx, 6] int64
    (FeatureEngine.flow_moments) and resample(planes, (height, width), filter, window) -> planes (FeatureEngine.resample) --
    so the same driver runs on the engine and on the numpy restatement (tests/flow_ref.py), with the same integers.

    Pyramid level l is both clips resized whole-plane to (W >> l, H >> l) with "bilinear" (register_levels picks the levels and
    the tile of each).  At a level, the capture is resampled with `filter` through the window of the current map, the moments
    of all frames are summed and solve_geometry gives an increment; it is composed (compose_geometry) and the map
    re-quantised to its Q16 window (geometry_window) until an increment moves no frame corner by 1/64 pixel, or `max_iters`
    increments were applied.  From level l to l - 1 the shift doubles and the scale stays.  A level whose system is singular
    is left as it came; at level 0 that ends the run with converged = False, as does a map outside 1/2 < s < 2,
    |d| < n / 4.  The first pass of all is one at full resolution on the clips as they are: mse_before.

    Returns {dx, dy, sx, sy (floats of the exact Fractions of the final window), x0_q16, y0_q16, w_q16, h_q16 (the same-size
    pqa_resample window of the luma plane), corner_px (the largest displacement of a frame corner under the map),
    mse_before, mse_after (sum dt^2 / 256 per counted pixel of the first and of the last full-resolution pass), iterations
    (increments applied, all levels), levels (the coarsest level), tile, converged}.  `trace` (a list) receives (level,
    (x0_q16, y0_q16, w_q16, h_q16), M) of every pass."""
    ref, dis = list(ref), list(dis)
    if not ref or len(ref) != len(dis):
        raise ValueError("register needs as many captured as reference planes, and one at least")
    H, W = np.shape(ref[0])
    plan = register_levels(W, H, tile, levels)

    def measure(r, d, t, level, win):
        M = np.asarray(moments(r, d, t)).sum(axis=0)
        if trace is not None:
            trace.append((level, win, M.copy()))
        return M

    def mse(M):
        return int(M[:, :, 5].sum()) / (256.0 * len(ref) * (W - 2) * (H - 2))
    full = (0, 0, W * Q16, H * Q16)
    mse_before = mse_after = mse(measure(ref, dis, plan[-1][1], 0, full))
    size = (W >> plan[0][0], H >> plan[0][0])
    win = (0, 0, size[0] * Q16, size[1] * Q16)      # (x0_q16, y0_q16, w_q16, h_q16) at the size of the current level
    iterations, converged, failed = 0, False, False
    for level, t in plan:
        w, h = W >> level, H >> level
        if (w, h) != size:            # one level finer: the shift scales with the plane, the scale factor stays
            (dx, sx), (dy, sy) = window_geometry(win[0], win[2], size[0]), window_geometry(win[1], win[3], size[1])
            (x0, ww), (y0, wh) = geometry_window(dx * 2, sx, w), geometry_window(dy * 2, sy, h)
            win, size = (x0, y0, ww, wh), (w, h)
        if level:
            r_l, d_l = resample(ref, (h, w), "bilinear", None), resample(dis, (h, w), "bilinear", None)
        else:
            r_l, d_l = ref, dis
        converged = False
        for it in range(max_iters + 1):
            fwin = tuple(v / float(Q16) for v in win)
            warped = d_l if win == (0, 0, w * Q16, h * Q16) else resample(d_l, (h, w), filter, fwin)
            M = measure(r_l, warped, t, level, win)
            if level == 0:
                mse_after = mse(M)
            inc = solve_geometry(M, w, h, t)
            if inc is None:
                failed = level == 0
                break
            if _corner_sq(*inc, w, h) < REGISTER_STOP_PX ** 2:
                converged = True
                break
            if it == max_iters:
                break
            (dx, sx), (dy, sy) = window_geometry(win[0], win[2], w), window_geometry(win[1], win[3], h)
            dx, sx = compose_geometry(dx, sx, inc[0], inc[1])
            dy, sy = compose_geometry(dy, sy, inc[2], inc[3])
            if not (Fraction(1, 2) < sx < 2 and Fraction(1, 2) < sy < 2 and abs(dx) * 4 < w and abs(dy) * 4 < h):
                failed = True
                break
            (x0, ww), (y0, wh) = geometry_window(dx, sx, w), geometry_window(dy, sy, h)
            win = (x0, y0, ww, wh)
            iterations += 1
        if failed:
            break
    if failed:
        converged = False
    if size != (W, H):      # the run ended above level 0: report the map at full resolution
        win, size = full, (W, H)
    (dx, sx), (dy, sy) = window_geometry(win[0], win[2], W), window_geometry(win[1], win[3], H)
    corner = max(((sx - 1) * gx * W / 2 + dx) ** 2 + ((sy - 1) * gy * H / 2 + dy) ** 2 for gx in (-1, 1) for gy in (-1, 1))
    return {"dx": float(dx), "dy": float(dy), "sx": float(sx), "sy": float(sy), "x0_q16": int(win[0]), "y0_q16": int(win[1]),
            "w_q16": int(win[2]), "h_q16": int(win[3]), "corner_px": float(corner) ** 0.5, "mse_before": float(mse_before),
            "mse_after": float(mse_after), "iterations": int(iterations), "levels": int(plan[0][0]), "tile": int(tile),
            "converged": bool(converged)}


# ---- colour-matrix alignment -------------------------------------------------------------------------------------------------
# A capture chain that decodes Y'CbCr with one matrix and encodes with another couples the planes:
# (Yd, Ud, Vd) = A (Yr, Ur, Vr) + b.  The measurement is the Gram matrix of z = (1, SYr, Ur, Vr, SYd, Ud, Vd) over the chroma
# grid (FeatureEngine.colour_moments, pqa_colour_moments; SY: the sum of the s = 2^(hshift + vshift) luma samples under a chroma
# sample).  Everything below is in PER-SAMPLE units: a luma component is the block mean SY / s, so the factors of s are divided
# out of the sums here, exactly.
COLOUR_STANDARDS = {"bt601": (Fraction(299, 1000), Fraction(114, 1000)), "bt709": (Fraction(2126, 10000), Fraction(722, 10000)),
                    "bt2020": (Fraction(2627, 10000), Fraction(593, 10000))}
COLOUR_MAPS = ("identity",) + tuple(f"{x}_to_{y}" for x in COLOUR_STANDARDS for y in COLOUR_STANDARDS if x != y)
COLOUR_Q = 14                                             # pqa_colour_apply's matrix is Q14
COLOUR_MAX_GAIN, COLOUR_MAX_OFFSET = 1 << 16, 1 << 28     # its entries lie strictly inside (-limit, limit)


def _encode_matrix(kr: Fraction, kb: Fraction):
    """E: R'G'B' -> (Y', Cb, Cr), Y' in 0 ... 1 and Cb, Cr in -1/2 ... 1/2, for the luma weights (Kr, Kb)"""
    kg = 1 - kr - kb
    y = [kr, kg, kb]
    cb = [(int(i == 2) - y[i]) / (2 * (1 - kb)) for i in range(3)]
    cr = [(int(i == 0) - y[i]) / (2 * (1 - kr)) for i in range(3)]
    return [y, cb, cr]


def _invert3(A):
    """the inverse of a 3 x 3 matrix of Fractions, or None when it is singular"""
    cols = [_solve_fractions(A, [int(i == j) for i in range(3)]) for j in range(3)]
    if any(c is None for c in cols):
        return None
    return [[cols[j][i] for j in range(3)] for i in range(3)]


def _matmul3(A, B):
    return [[sum(A[i][k] * B[k][j] for k in range(3)) for j in range(3)] for i in range(3)]


def _code_ranges(bit_depth: int, full_range: bool):
    """(offsets, spans) of (Y, Cb, Cr) in code values"""
    f = 1 << (int(bit_depth) - 8)
    if full_range:
        top = (1 << int(bit_depth)) - 1
        return [Fraction(0), Fraction(128 * f), Fraction(128 * f)], [Fraction(top)] * 3
    return [Fraction(16 * f), Fraction(128 * f), Fraction(128 * f)], [Fraction(219 * f), Fraction(224 * f), Fraction(224 * f)]


def named_colour_map(name: str, bit_depth: int, full_range: bool = False):
    """(A, b) of the fixed map dis = A ref + b over (Y, U, V) in code values, as Fractions (A: 3 x 3 nested lists, b: 3):
    "identity", or "X_to_Y" for X != Y in bt601 / bt709 / bt2020 -- material whose samples mean standard X, decoded as X and
    encoded again as Y: E_Y E_X^-1 with E built from (Kr, Kb) (COLOUR_STANDARDS).  Limited range: luma spans 219 f from 16 f and
    chroma 224 f about 128 f, f = 2^(bit_depth - 8); full range: both span 2^bit_depth - 1, luma from 0, chroma about 128 f."""
    ident = [[Fraction(int(i == j)) for j in range(3)] for i in range(3)]
    if name == "identity":
        return ident, [Fraction(0)] * 3
    if name not in COLOUR_MAPS:
        raise ValueError(f"unknown colour map {name!r}")
    x, y = name.split("_to_")
    M = _matmul3(_encode_matrix(*COLOUR_STANDARDS[y]), _invert3(_encode_matrix(*COLOUR_STANDARDS[x])))
    off, span = _code_ranges(bit_depth, full_range)
    A = [[span[i] * M[i][j] / span[j] for j in range(3)] for i in range(3)]
    b = [off[i] - sum(A[i][j] * off[j] for j in range(3)) for i in range(3)]
    return A, b


def _colour_gram(G, s: int):
    """the pooled 7 x 7 Gram matrix in per-sample units (Fractions) of G[n_frames][28]"""
    G = np.asarray(G)
    if G.ndim != 2 or G.shape[0] < 1 or G.shape[1] != 28:
        raise ValueError("G must be [n_frames >= 1, 28]")
    pooled = [sum(int(x) for x in G[:, e]) for e in range(28)]
    scale = [1, s, 1, 1, s, 1, 1]
    S = [[Fraction(0)] * 7 for _ in range(7)]
    e = 0
    for i in range(7):
        for j in range(i, 7):
            S[i][j] = S[j][i] = Fraction(pooled[e], scale[i] * scale[j])
            e += 1
    return S


def _colour_sse(S, k: int, coef):
    """sum over the samples of (z_k - coef . (1, Yr, Ur, Vr))^2 from the Gram matrix alone"""
    return S[k][k] - 2 * sum(coef[i] * S[i][k] for i in range(4)) + sum(coef[i] * coef[j] * S[i][j] for i in range(4) for j in range(4))


def best_colour(G, bit_depth: int, hshift: int, vshift: int, *, full_range: bool = False, min_improvement: float = 2.0,
                snap: float = 1.25, total_samples: int | None = None) -> dict:
    """The colour map of a captured clip from G[n_frames][28] (pqa_colour_moments: the upper triangle of the sum of z z^T, z =
    (1, SYr, Ur, Vr, SYd, Ud, Vd), over the unmasked chroma samples).  The frames are pooled; everything below is Python ints
    and Fractions, converted to float only in the result.  s = 2^(hshift + vshift); every luma quantity is the BLOCK MEAN
    SY / s, so a luma MSE here is the error of the block mean: the block-sum residual divided by s^2.

    matrix / offset: the least-squares fit of each captured component on (1, Yr, Ur, Vr) from the normal equations.  The MSE of a
    map is formed per plane from the Gram matrix alone, without clipping (the measurement masks clipped samples instead:
    pqa_colour_moments' lo / hi) and pooled with the plane sizes as weights, (s Y + U + V) / (s + 2): mse_identity,
    mse_matrix (the fit), mse_diagonal (each component fitted on 1 and its own plane only: what level alignment could
    reach), named = {identity, X_to_Y ...: under named_colour_map()}; the per-plane triples are under `planes`.
    kind = the named map with the smallest pooled MSE (ties: the order of COLOUR_MAPS), or "matrix" when that MSE exceeds
    snap * mse_matrix.  cross_plane = mse_diagonal > snap * mse_matrix: when false, level alignment is the right tool.
    mismatch = mse_identity > min_improvement * (pooled MSE of the chosen map).  map_matrix / map_offset: the chosen map's A
    and b (the named map's own values, or the fit): what colour_correction() undoes.
    degenerate = the 4 x 4 system is singular (a flat or monochrome-looking clip) or fewer than 4 samples survived the mask:
    identity, no mismatch.  samples = the samples that entered; samples_masked_share = 1 - samples / total_samples (None
    when total_samples is not given); frames = n_frames."""
    s = 1 << (int(hshift) + int(vshift))
    S = _colour_gram(G, s)
    n = S[0][0]
    weights = [Fraction(s, s + 2), Fraction(1, s + 2), Fraction(1, s + 2)]

    def pooled(triple):
        return sum(w * m for w, m in zip(weights, triple))

    def map_mse(A, b):
        return [_colour_sse(S, 4 + k, [b[k]] + list(A[k])) / n for k in range(3)]
    ident = named_colour_map("identity", bit_depth, full_range)
    fit = None
    if n >= 4:
        rows = [_solve_fractions([S[i][:4] for i in range(4)], [S[i][4 + k] for i in range(4)]) for k in range(3)]
        if all(r is not None for r in rows):
            fit = ([list(r[1:]) for r in rows], [r[0] for r in rows])
    masked = None if total_samples is None else (float(1 - n / int(total_samples)) if total_samples else 0.0)
    base = {"frames": int(np.asarray(G).shape[0]), "samples": int(n), "samples_masked_share": masked}
    if fit is None:
        zero = [0.0, 0.0, 0.0]
        flat = {k: float(x) for k, x in zip(("mse_identity", "mse_matrix", "mse_diagonal"), (0, 0, 0))}
        return dict(base, kind="identity", mismatch=False, cross_plane=False, degenerate=True, named={}, **flat,
                    matrix=[[float(v) for v in r] for r in ident[0]], offset=zero, map_matrix=[[float(v) for v in r] for r in ident[0]],
                    map_offset=zero, planes={"mse_identity": zero, "mse_matrix": zero, "mse_diagonal": zero, "named": {}})
    A, b = fit
    diag = []
    for k in range(3):   # component k on (1, its own plane)
        i = 1 + k
        sol = _solve_fractions([[S[0][0], S[0][i]], [S[i][0], S[i][i]]], [S[0][4 + k], S[i][4 + k]])
        coef = [Fraction(0)] * 4
        if sol is None:      # its own plane is flat: the mean is all that can be fitted
            coef[0] = S[0][4 + k] / n
        else:
            coef[0], coef[i] = sol
        diag.append(_colour_sse(S, 4 + k, coef) / n)
    named_planes = {name: map_mse(*named_colour_map(name, bit_depth, full_range)) for name in COLOUR_MAPS}
    named = {name: pooled(t) for name, t in named_planes.items()}
    fit_planes = map_mse(A, b)
    mse_matrix, mse_diagonal = pooled(fit_planes), pooled(diag)
    kind = min(COLOUR_MAPS, key=lambda name: named[name])   # min keeps the first of equals
    chosen = named[kind]
    if chosen > Fraction(snap) * mse_matrix:
        kind, chosen = "matrix", mse_matrix
    mA, mb = (A, b) if kind == "matrix" else named_colour_map(kind, bit_depth, full_range)

    def floats(M):
        return [[float(v) for v in r] for r in M]
    return dict(base, kind=kind, mismatch=bool(named["identity"] > Fraction(min_improvement) * chosen),
                cross_plane=bool(mse_diagonal > Fraction(snap) * mse_matrix), degenerate=False,
                mse_identity=float(named["identity"]), mse_matrix=float(mse_matrix), mse_diagonal=float(mse_diagonal),
                named={k: float(v) for k, v in named.items()}, matrix=floats(A), offset=[float(v) for v in b],
                map_matrix=floats(mA), map_offset=[float(v) for v in mb],
                planes={"mse_identity": [float(v) for v in named_planes["identity"]], "mse_matrix": [float(v) for v in fit_planes],
                        "mse_diagonal": [float(v) for v in diag],
                        "named": {k: [float(v) for v in t] for k, t in named_planes.items()}})


def colour_matrix_q14(A, b):
    """int32[12] of the map (A, b) as pqa_colour_apply takes it -- rows (offset, gains of Y, U, V), each entry times 2^14
    rounded half up, once -- or None when an entry leaves the ABI's range (|offset| < 2^28, |gain| < 2^16)"""
    half = Fraction(1, 2)
    out = []
    for i in range(3):
        row = [(Fraction(b[i]) * (1 << COLOUR_Q) + half).__floor__()] + [(Fraction(A[i][j]) * (1 << COLOUR_Q) + half).__floor__() for j in range(3)]
        if abs(row[0]) >= COLOUR_MAX_OFFSET or any(abs(v) >= COLOUR_MAX_GAIN for v in row[1:]):
            return None
        out += row
    return np.asarray(out, np.int32)


def colour_correction(result: dict, bit_depth: int, full_range: bool = False):
    """The Q14 int32[12] matrix (colour_matrix_q14) of the INVERSE of the map a best_colour() result chose: ref = A^-1 (dis - b).
    A named kind inverts the named map's own Fractions, "matrix" the fit (its floats at their exact binary values).  The
    inverse is formed exactly and rounded once.  None when the matrix is singular or the inverse leaves the ABI's range."""
    if result["kind"] in COLOUR_MAPS:
        A, b = named_colour_map(result["kind"], bit_depth, full_range)
    else:
        A = [[Fraction(v) for v in r] for r in result["map_matrix"]]
        b = [Fraction(v) for v in result["map_offset"]]
    inv = _invert3(A)
    if inv is None:
        return None
    return colour_matrix_q14(inv, [-sum(inv[i][j] * b[j] for j in range(3)) for i in range(3)])


# ---- active picture -------------------------------------------------------------------------------------------------------------
# Black bars from the row and column profiles of a clip (FeatureEngine.line_profiles, pqa_line_profiles): sums and sums of
# squares per line, exact integers.  A line of n samples is DARK in a frame iff its sum is at most L n, L = limit 2^(b - 8):
# its mean does not exceed `limit` in 8-bit code values (24: black at 16 plus what a noisy capture of it adds).  A bar is a
# run of lines from an edge that are dark in every frame that shows a picture at all.  Python ints and Fractions only.
ACTIVE_LIMIT = 24
ACTIVE_TOLERANCE = 16   # bars of the two clips that differ by more than this many lines on a side are another geometry, not a shift
ACTIVE_MIN_SIZE = 16    # the smallest frame a scoring context accepts, each way


def _edge_run(dark, n: int, skip: int):
    """(lines from the low edge, lines from the high edge) that are dark; the outermost `skip` lines of an edge count as dark
    whatever they hold, but a run that ends inside them is no bar.  None when the runs meet: no picture line is left."""
    lo = 0
    while lo < n and (lo < skip or dark[lo]):
        lo += 1
    hi = 0
    while hi < n and (hi < skip or dark[n - 1 - hi]):
        hi += 1
    if lo + hi >= n:
        return None
    return (lo if lo > skip else 0), (hi if hi > skip else 0)


def active_picture(rows, cols_of, bit_depth: int, *, limit: int = ACTIVE_LIMIT, skip: int = 0) -> dict:
    """The active picture window of a clip from its line profiles.  rows[f][y] = (sum, sum of squares) of row y of frame f
    over the full width; cols_of(top, bottom) -> cols[f][x] = the same of column x over the rows top ... H - bottom - 1 only
    (a column sum over the full height is dragged down by letterbox rows: a dim picture column would pass for a bar).
    cols_of(0, 0) is the profile that came with `rows` and costs the caller nothing; it is asked for first, for the width.

    Frames whose every row is dark (black frames, fades) are left out; `all_dark` when none remains, or when no picture
    line remains between the bars.  top = the largest t such that the rows 0 ... t - 1 are dark in every remaining frame,
    the outermost `skip` rows counting as dark whatever they hold (a caption or timecode line in row 0 of a capture); a run
    that ends inside the skipped lines is no bar.  bottom likewise; then left and right from cols_of(top, bottom) with n =
    H - top - bottom.  Returns {left, top, right, bottom, window: [x0, y0, w, h] or None, frames_used, all_dark, bar_noise}:
    bar_noise = the pooled variance (a Fraction) of the samples in the bars -- the bar rows over the full width and the bar
    columns over the active rows, without the skipped lines, over the remaining frames; None without bars."""
    b, limit, skip = int(bit_depth), int(limit), int(skip)
    if b < 8 or not 0 <= limit <= 255 or skip < 0:
        raise ValueError("active_picture needs bit_depth >= 8, 0 <= limit <= 255 and skip >= 0")
    L = limit << (b - 8)
    R = [[(int(s), int(q)) for s, q in frame] for frame in rows]
    if not R or not R[0]:
        raise ValueError("rows must be [n_frames >= 1][H >= 1][2]")
    H = len(R[0])
    full = cols_of(0, 0)
    W = len(full[0])
    none = {"left": 0, "top": 0, "right": 0, "bottom": 0, "window": None, "frames_used": 0, "all_dark": True, "bar_noise": None}
    used = [f for f in range(len(R)) if any(R[f][y][0] > L * W for y in range(H))]
    if not used:
        return none
    run = _edge_run([all(R[f][y][0] <= L * W for f in used) for y in range(H)], H, skip)
    if run is None:
        return dict(none, frames_used=len(used))
    top, bottom = run
    ah = H - top - bottom
    cols = full if top == 0 and bottom == 0 else cols_of(top, bottom)
    Cc = [[(int(s), int(q)) for s, q in cols[f]] for f in used]
    if any(len(c) != W for c in Cc):
        raise ValueError("cols_of must return [n_frames][W][2]")
    run = _edge_run([all(c[x][0] <= L * ah for c in Cc) for x in range(W)], W, skip)
    if run is None:
        return dict(none, frames_used=len(used))
    left, right = run
    # the bars' samples: lines outside the skipped ones
    bar_rows = [y for y in range(H) if (y < top or y >= H - bottom) and skip <= y < H - skip]
    bar_cols = [x for x in range(W) if (x < left or x >= W - right) and skip <= x < W - skip]
    count = len(used) * (len(bar_rows) * W + len(bar_cols) * ah)
    noise = None
    if count:
        s = sum(R[f][y][0] for f in used for y in bar_rows) + sum(c[x][0] for c in Cc for x in bar_cols)
        q = sum(R[f][y][1] for f in used for y in bar_rows) + sum(c[x][1] for c in Cc for x in bar_cols)
        noise = Fraction(q, count) - Fraction(s, count) ** 2
    return {"left": left, "top": top, "right": right, "bottom": bottom, "window": [left, top, W - left - right, ah],
            "frames_used": len(used), "all_dark": False, "bar_noise": noise}


def common_window(ref_ap: dict, dis_ap: dict, width: int, height: int, hshift: int, vshift: int, *,
                  tolerance: int = ACTIVE_TOLERANCE, min_size: int = ACTIVE_MIN_SIZE) -> dict:
    """What two active_picture() results of clips of width x height mean for a pair.  Returns {crop: [left, top, right,
    bottom], same, mismatch, scale, offset, reason}.  crop: per side the larger of the two clips' bars, rounded up to the
    chroma step (1 << hshift horizontally, 1 << vshift vertically), as registration_crop rounds -- the common inner
    rectangle; a difference of the bars within `tolerance` lines is a displacement, which is cropped and left to
    spatial_align.  same: all four bars are equal.  mismatch: a side differs by more than `tolerance` -- the capture has
    other bars than the reference, a scaler sits in the chain, and cropping through that would score geometry: crop is then
    all zero.  scale = [w_dis / w_ref, h_dis / h_ref] and offset = [centre_dis - centre_ref] per axis of the two windows, as
    Fractions (window_geometry of each window against the frame): what `register` or `resize` would have to undo.  reason:
    None when crop is to be applied, else "all dark" (either clip; scale and offset are None), "windows differ" (mismatch),
    "no bars" (crop all zero) or "window too small" (less than min_size samples remain on an axis)."""
    if ref_ap["all_dark"] or dis_ap["all_dark"]:
        return {"crop": [0, 0, 0, 0], "same": False, "mismatch": False, "scale": None, "offset": None, "reason": "all dark"}
    sides = ("left", "top", "right", "bottom")
    rb, db = [int(ref_ap[k]) for k in sides], [int(dis_ap[k]) for k in sides]
    same = rb == db
    mismatch = any(abs(r - d) > int(tolerance) for r, d in zip(rb, db))
    scale, offset = [], []
    for n, lo in ((int(width), 0), (int(height), 1)):
        geo = [window_geometry(bars[lo] * Q16, (n - bars[lo] - bars[lo + 2]) * Q16, n) for bars in (rb, db)]
        scale.append(geo[1][1] / geo[0][1])
        offset.append(geo[1][0] - geo[0][0])
    steps = (1 << int(hshift), 1 << int(vshift), 1 << int(hshift), 1 << int(vshift))
    crop = [-(-max(r, d) // st) * st for r, d, st in zip(rb, db, steps)]
    if mismatch:
        crop, reason = [0, 0, 0, 0], "windows differ"
    elif not any(crop):
        reason = "no bars"
    elif width - crop[0] - crop[2] < min_size or height - crop[1] - crop[3] < min_size:
        reason = "window too small"
    else:
        reason = None
    return {"crop": crop, "same": bool(same), "mismatch": bool(mismatch), "scale": scale, "offset": offset, "reason": reason}
