"""Coding-grid detection: whether the difference between a captured clip and its reference is a BLOCK GRID, the one artefact an
encoder leg leaves and no other leg does.  Pure Python and numpy, no GPU: the solver behind score_files(coding_grid=True).
The measurement is FeatureEngine.edge_profiles (pqa_edge_profiles, csrc/edge_profiles.hip): with R the reference and D the
captured plane, per column line x = 1 ... W - 1 (the boundary between the columns x - 1 and x) and per row line y = 1 ... H - 1

    a = the difference of R across the line      b = the difference of D across the line      (sum a^2, sum b^2, sum a b)

summed along the line; word 2 is int64 stored in the uint64 word; line 0 of each axis is zero.

What a line is worth.  The least-squares gain g = sum ab / sum a^2 splits the gradient energy of the capture as spectrum.split
splits a band: sum b^2 = g^2 sum a^2 + N, and N = sum b^2 - (sum ab)^2 / sum a^2 is the ADDED part, gradient across the line
that the reference does not explain (non-negative by Cauchy-Schwarz; all of sum b^2 where the reference is flat).  A block
edge is exactly that: a step across one line which the picture does not have.

The rule.  Line i, 2 <= i <= n - 2, VOTES when its value is strictly above both neighbours.  A hypothesis (P, phi), 0 <= phi < P,
owns the lines i = phi (mod P) of that range: k of them, s of which vote.  Without a grid three exchangeable values have their
largest in the middle with probability 1/3, and for P >= 4 the triples of a hypothesis's lines do not overlap (which is why 4 is
the smallest period), so s has mean k / 3 and variance 2 k / 9 and

    z^2 = (3 s - k)^2 / (2 k),     3 s > k required,

is accepted from z2_min = 25: one-sided 2.9e-7 a hypothesis against sum_{P = 4}^{64} P ~ 2 100 hypotheses an axis.  z^2 <= 2 k,
so a period needs at least 13 lines inside the plane.  The largest z^2 wins, compared by cross-multiplied integers; ties go to
the smaller P, then the smaller phi.  The true period P beats 2 P (half the lines: half the z^2) and P / 2 (its extra lines do
not vote).  Votes are binary: one strong outlier line is one vote and cannot fake a grid.

Phases are in the coordinates of the SCORED window -- after any crop, shift or resize score_files applied -- not of the file.
A grid at phase != 0 means the picture was cropped or shifted after the encode.

Not modelled: grids stretched by a non-integer factor (a scaler after the encode), the short period a scaler's own polyphase
pattern shows (a bilinear 4/3 or 3/2 upscale shows 4, or 3 and then 6), adaptive block sizes beyond "all edges lie on the 8- or
4-grid", and deblocking that leaves nothing to find.

Every decision is taken on Python ints and Fractions; floats are formed only for the report."""
from fractions import Fraction

import numpy as np

SUM_AA, SUM_BB, SUM_AB = range(3)
SUMS = 3
WHICH = ("added", "reference", "captured")
KINDS = ("identical", "none", "grid")
PERIODS = range(4, 65)
Z2_MIN = 25


def pool(lines) -> list:
    """[(sum a^2, sum b^2, sum a b)] per line as Python ints, added over the frames: exact however many frames there are.
    lines: uint64 [n, L, 3] or [L, 3]"""
    M = np.asarray(lines)
    if M.dtype != np.uint64 or M.ndim not in (2, 3) or M.shape[-1] != SUMS:
        raise ValueError("edge profiles are uint64 [n, lines, 3] or [lines, 3]")
    M = M.reshape((-1,) + M.shape[-2:])
    S = np.ascontiguousarray(M[..., SUM_AB]).view(np.int64)
    out = []
    for i in range(M.shape[1]):
        out.append((sum(M[:, i, SUM_AA].tolist()), sum(M[:, i, SUM_BB].tolist()), sum(S[:, i].tolist())))
    return out


def _value(aa: int, bb: int, ab: int, which: str):
    if which == "reference":
        return aa
    if which == "captured":
        return bb
    return Fraction(bb * aa - ab * ab, aa) if aa else bb


def line_values(lines, which: str = "added") -> list:
    """one value a line of the pooled profiles (a uint64 array as pool takes it, or pool's list): "added" the part of the
    capture's gradient energy the reference does not explain, "reference" sum a^2, "captured" sum b^2; ints or Fractions"""
    if which not in WHICH:
        raise ValueError('which must be "added", "reference" or "captured"')
    pooled = lines if isinstance(lines, list) else pool(lines)
    return [_value(aa, bb, ab, which) for aa, bb, ab in pooled]


def _periods(periods):
    ps = sorted(set(int(p) for p in periods))
    if not ps or ps[0] < 4 or ps[-1] > 64:
        raise ValueError("periods lie in 4 ... 64")
    return ps


def _measure(values, period: int, phase: int, pairs):
    """(contrast, excess_mse) of the lines of one hypothesis: floats for the report; contrast None on a zero denominator"""
    n = len(values)
    first = phase + period * max(0, -(-(2 - phase) // period))
    own = list(range(first, n - 1, period))
    on = sum((values[i] for i in own), Fraction(0))
    beside = sum((values[i - 1] + values[i + 1] for i in own), Fraction(0))
    contrast = float(2 * on / beside) if beside else None
    pixels = Fraction(pairs) * len(own)
    return contrast, (float((on - beside / 2) / pixels) if pixels else 0.0)


def find_grid(values, periods=PERIODS, z2_min=Z2_MIN, pairs=1):
    """the period and phase whose lines stand out of `values` (one number a line, line 0 first), or None.  pairs: the pixel
    pairs one line holds (the other side of the plane times the frames, times 4^(bits - 8) for 8-bit units): the divisor of
    excess_mse.  Returns {period, phase, lines, votes, z2, contrast, excess_mse}"""
    ps = _periods(periods)
    zmin = Fraction(z2_min)
    if zmin < 0:
        raise ValueError("z2_min must not be negative")
    n = len(values)
    votes = [0] * n
    for i in range(2, n - 1):
        votes[i] = 1 if values[i] > values[i - 1] and values[i] > values[i + 1] else 0
    best = None     # (numerator, denominator, P, phi, k, s)
    for P in ps:
        for phi in range(P):
            first = phi + P * max(0, -(-(2 - phi) // P))
            k = len(range(first, n - 1, P))
            if k == 0:
                continue
            s = sum(votes[first:n - 1:P])
            if 3 * s <= k:
                continue
            num, den = (3 * s - k) ** 2, 2 * k
            if num < zmin * den:
                continue
            if best is None or num * best[1] > best[0] * den:      # strictly: a tie keeps the smaller P, then the smaller phi
                best = (num, den, P, phi, k, s)
    if best is None:
        return None
    num, den, P, phi, k, s = best
    contrast, excess = _measure(values, P, phi, pairs)
    return {"period": P, "phase": phi, "lines": k, "votes": s, "z2": num / den, "contrast": contrast, "excess_mse": excess}


def _check(rows, cols, w: int, h: int):
    rows, cols = np.asarray(rows), np.asarray(cols)
    for M, side in ((rows, h), (cols, w)):
        if M.dtype != np.uint64 or M.ndim != 3 or M.shape[1:] != (side, SUMS):
            raise ValueError("edge profiles are uint64 rows [n, H, 3] and cols [n, W, 3]")
    if rows.shape[0] != cols.shape[0]:
        raise ValueError("rows and cols hold different numbers of frames")
    return rows, cols


def summary(rows, cols, w: int, h: int, bits: int = 8, periods=PERIODS, z2_min=Z2_MIN) -> dict:
    """the verdict on one plane of a clip pair: `kind` (identical: no line differs; none; grid), `x` / `y` the grid of the added
    gradient along the columns / rows (find_grid's dict or None), `block` [Px, Py], `phase` [phix, phiy] in the coordinates of
    the scored window, `aligned` (every phase found is 0), and under `reference_grid` / `captured_grid` the same search on the
    gradient energy of each clip alone: a grid in the reference means the "reference" is already an encode.  excess_mse is in
    8-bit code values squared."""
    rows, cols = _check(rows, cols, w, h)
    n = rows.shape[0]
    ps = _periods(periods)
    unit = 4 ** (bits - 8)
    pr, pc = pool(rows), pool(cols)
    identical = all(aa + bb - 2 * ab == 0 for aa, bb, ab in pr + pc)
    found = {}
    for which in WHICH:
        found[which] = {"x": find_grid(line_values(pc, which), ps, z2_min, pairs=h * n * unit),
                        "y": find_grid(line_values(pr, which), ps, z2_min, pairs=w * n * unit)}
    gx, gy = found["added"]["x"], found["added"]["y"]
    kind = "identical" if identical else "grid" if (gx or gy) else "none"
    grid = kind == "grid"
    return {"kind": kind, "frames": int(n), "periods": [ps[0], ps[-1]], "z2_min": float(z2_min),
            "x": gx if grid else None, "y": gy if grid else None,
            "block": [gx["period"] if gx else None, gy["period"] if gy else None] if grid else None,
            "phase": [gx["phase"] if gx else None, gy["phase"] if gy else None] if grid else None,
            "aligned": all(g["phase"] == 0 for g in (gx, gy) if g) if grid else None,
            "reference_grid": found["reference"], "captured_grid": found["captured"]}


def _frame_contrast(lines, f: int, g) -> float:
    """the contrast of frame f's own added values on the lines of grid g; 1 without a grid or on a zero denominator"""
    if not g:
        return 1.0
    n = lines.shape[1]
    P, phi = g["period"], g["phase"]
    first = phi + P * max(0, -(-(2 - phi) // P))
    S = np.ascontiguousarray(lines[f, :, SUM_AB]).view(np.int64)

    def val(i):
        return _value(int(lines[f, i, SUM_AA]), int(lines[f, i, SUM_BB]), int(S[i]), "added")

    on = beside = Fraction(0)
    for i in range(first, n - 1, P):
        on += val(i)
        beside += val(i - 1) + val(i + 1)
    return float(2 * on / beside) if beside else 1.0


def frame_rows(rows, cols, w: int, h: int, summ: dict) -> list:
    """one row a frame: {frame, blockiness_x, blockiness_y}, the contrast of that frame's own added gradient on the lines the
    clip's summary chose (keyframe pumping shows here and in no pooled figure); 1 where an axis has no grid"""
    rows, cols = _check(rows, cols, w, h)
    return [{"frame": f, "blockiness_x": _frame_contrast(cols, f, summ.get("x")),
             "blockiness_y": _frame_contrast(rows, f, summ.get("y"))} for f in range(rows.shape[0])]


def frame_columns(frames: list) -> dict:
    """the two per-frame metric columns of the luma from frame_rows' list"""
    return {k: np.array([r[k] for r in frames], np.float64) for k in ("blockiness_x", "blockiness_y")}


def analyse(rows, cols, w: int, h: int, bits: int = 8, periods=PERIODS, z2_min=Z2_MIN) -> dict:
    """{summary, frames} of one plane, json.dumps-able"""
    summ = summary(rows, cols, w, h, bits, periods, z2_min)
    return {"summary": summ, "frames": frame_rows(rows, cols, w, h, summ)}
