"""Distortion spectrum: what KIND of difference two clips have.  Pure Python and numpy, no GPU: the solver behind
score_files(spectrum=L).  The measurement is FeatureEngine.band_moments (pqa_band_moments, csrc/band_moments.hip): per level
l = 1 ... L and orientation o (0 H, 1 V, 2 D, 3 A) of the unnormalised Haar transform the exact sums
M[..., l-1, o, 0..2] = sum r_o^2, sum d_o^2, sum r_o d_o of the reference's and the captured clip's coefficients.

Per band the least-squares gain g = sum rd / sum r^2 and the residual sum d^2 - g^2 sum r^2 are VIF's signal / noise model
applied to the whole frame, and they split the band's squared error EXACTLY:

    err = sum (d - r)^2 = sum r^2 - 2 sum rd + sum d^2 = (1 - g)^2 sum r^2  +  (sum d^2 - g^2 sum r^2) = loss + noise

loss is what a gain below (or above) 1 explains -- detail the chain removed or peaked -- and noise is what is uncorrelated with
the reference: noise, ringing, blocking.  noise >= 0 by Cauchy-Schwarz.  A band whose reference is empty (sum r^2 = 0) has no
gain and all of its error is noise.

Units.  A coefficient of level l is 2^l times the orthonormal one and stands for 4^l pixels, so x / (16^l n_l) with n_l the
level's coefficients is a mean squared error per pixel; divided by 4^(b - 8) it is in 8-bit code values squared.  For planes
whose sizes are multiples of 2^L the band MSEs of H, V, D over all levels plus that of A_L add up to the plane's MSE exactly
(Parseval); otherwise a level covers `coverage` = n_l 4^l / (W H) of the plane.

Every decision is taken on Python ints and Fractions; floats are formed only by table_json / summary for the report."""
from fractions import Fraction

import numpy as np

ORIENTATIONS = ("h", "v", "d", "a")
SUM_RR, SUM_DD, SUM_RD = range(3)
MAX_LEVELS = 6


def _ratio(v, limit: int = 1 << 16) -> Fraction:
    """a threshold given as int, float or Fraction as the simplest fraction near it (0.5 -> 1/2)"""
    return Fraction(v).limit_denominator(limit)


def band_counts(width: int, height: int, levels: int) -> list:
    """[W_l * H_l for l = 1 ... levels]: the coefficients of a level, those whose 2^l x 2^l support is inside the plane"""
    if width < 1 or height < 1 or not 1 <= levels <= MAX_LEVELS:
        raise ValueError("band_counts needs a positive size and 1 ... 6 levels")
    return [(width >> l) * (height >> l) for l in range(1, levels + 1)]


def _signed(M) -> np.ndarray:
    """the moments as Python ints in an object array; the cross sums are int64 stored in the word"""
    M = np.asarray(M)
    if M.dtype != np.uint64 or M.shape[-2:] != (4, 3) or M.ndim < 3:
        raise ValueError("band moments are uint64 [..., L, 4, 3]")
    S = M.astype(object)
    S[..., SUM_RD] = np.ascontiguousarray(M[..., SUM_RD]).view(np.int64).astype(object)
    return S


def pool(M) -> np.ndarray:
    """object [L, 4, 3]: the clip-summed moments of per-frame moments [n, L, 4, 3] as Python ints (signed cross sums), exact"""
    S = _signed(M)
    if S.ndim != 4:
        raise ValueError("pool needs per-frame moments [n, L, 4, 3]")
    out = np.zeros(S.shape[1:], object)
    for f in range(S.shape[0]):
        out = out + S[f]
    return out


def split(rr: int, dd: int, rd: int):
    """(gain, err, loss, noise) of one band as Fractions, err == loss + noise; gain is None where the reference band is
    empty, and then all of the error is noise"""
    rr, dd, rd = int(rr), int(dd), int(rd)
    err = Fraction(rr - 2 * rd + dd)
    if rr == 0:
        return None, err, Fraction(0), err
    g = Fraction(rd, rr)
    return g, err, (1 - g) ** 2 * rr, dd - g * g * rr


def band_table(M_sum, width: int, height: int, bit_depth: int, frames: int = 1) -> list:
    """per level a dict {level, count, coverage, bands: {h, v, d, a}}; a band holds rr, dd, rd (ints), gain (Fraction or
    None), err, loss, noise (Fractions, err == loss + noise) and err_mse, loss_mse, noise_mse (Fractions, 8-bit code values
    squared per pixel).  M_sum: [L, 4, 3], uint64 moments of one frame pair or the output of pool(); `frames`: the pairs
    summed into it.  A level without coefficients has count 0 and MSEs of 0."""
    S = M_sum if isinstance(M_sum, np.ndarray) and M_sum.dtype == object else _signed(M_sum)
    if S.ndim != 3:
        raise ValueError("band_table needs moments [L, 4, 3]")
    levels = S.shape[0]
    counts = band_counts(width, height, levels)
    down = 4 ** (int(bit_depth) - 8)
    table = []
    for l in range(1, levels + 1):
        n = counts[l - 1] * int(frames)
        bands = {}
        for o, name in enumerate(ORIENTATIONS):
            rr, dd, rd = (int(v) for v in S[l - 1, o])
            g, err, loss, noise = split(rr, dd, rd)
            unit = Fraction(1, 16 ** l * n * down) if n else Fraction(0)
            bands[name] = {"rr": rr, "dd": dd, "rd": rd, "gain": g, "err": err, "loss": loss, "noise": noise,
                           "err_mse": err * unit, "loss_mse": loss * unit, "noise_mse": noise * unit}
        table.append({"level": l, "count": n, "coverage": Fraction(counts[l - 1] * 4 ** l, width * height), "bands": bands})
    return table


def _parts(table):
    """the bands that tile the spectrum once: H, V, D of every level and A of the last"""
    for row in table:
        for name in ("h", "v", "d"):
            yield row["level"], name, row["bands"][name]
    yield table[-1]["level"], "a", table[-1]["bands"]["a"]


def _bandwidth(table, name: str, floor: Fraction):
    for row in table:      # level 1 is the finest
        g = row["bands"][name]["gain"]
        if g is not None and g >= floor:
            return {"level": row["level"], "cycles_per_pixel": 1.0 / (1 << row["level"])}
    return {"level": None, "cycles_per_pixel": None}


def summary(table, *, min_mse=1.0, gain_floor=Fraction(1, 2)) -> dict:
    """what the table says in one object: total_mse; loss_share, noise_share; loss_by_orientation {h, v, d, a} and
    noise_by_level (and noise_a) in MSE units; noise_density_by_level: the noise per orthonormal coefficient of a level's H, V
    and D, which white noise keeps flat; bandwidth_h / bandwidth_v: the finest level whose H / V gain is at least gain_floor,
    with the band's upper edge 1 / 2^l cycles per pixel; kind: identical (no error at all), clean (total_mse < min_mse), loss
    (loss share >= 1/2), else noise; axis, for loss: horizontal if loss_H >= 2 loss_V, vertical for the reverse, else both.  The three thresholds are conventions of this report, not measurements."""
    min_mse, floor = _ratio(min_mse), _ratio(gain_floor)
    if min_mse < 0 or floor < 0:
        raise ValueError("spectrum thresholds are not negative")
    total = loss = noise = Fraction(0)
    loss_o = {k: Fraction(0) for k in ORIENTATIONS}
    noise_l = [Fraction(0)] * len(table)
    density = [Fraction(0)] * len(table)
    noise_a = Fraction(0)
    any_err = False
    for level, name, b in _parts(table):
        any_err = any_err or b["err"] != 0
        total += b["err_mse"]
        loss += b["loss_mse"]
        noise += b["noise_mse"]
        loss_o[name] += b["loss_mse"]
        if name == "a":
            noise_a += b["noise_mse"]
        else:
            noise_l[level - 1] += b["noise_mse"]
            density[level - 1] += b["noise_mse"] * 4 ** level / 3
    for row in table:      # A_l of a level above the last sees pixels that a deeper level's coverage may leave out
        any_err = any_err or any(b["err"] != 0 for b in row["bands"].values())
    if not any_err:
        kind = "identical"
    elif total < min_mse:
        kind = "clean"
    elif 2 * loss >= total:
        kind = "loss"
    else:
        kind = "noise"
    axis = None
    if kind == "loss":
        lh, lv = loss_o["h"], loss_o["v"]
        axis = "both" if lh == lv == 0 else "horizontal" if lh >= 2 * lv else "vertical" if lv >= 2 * lh else "both"
    share = (lambda x: float(x / total)) if total else (lambda x: 0.0)
    return {"total_mse": float(total), "loss_mse": float(loss), "noise_mse": float(noise),
            "loss_share": share(loss), "noise_share": share(noise),
            "loss_by_orientation": {k: float(v) for k, v in loss_o.items()},
            "noise_by_level": [float(v) for v in noise_l],
            "noise_density_by_level": [float(v) for v in density], "noise_a": float(noise_a),
            "bandwidth_h": _bandwidth(table, "h", floor), "bandwidth_v": _bandwidth(table, "v", floor),
            "kind": kind, "axis": axis, "min_mse": float(min_mse), "gain_floor": float(floor)}


def table_json(table) -> list:
    """the table with floats for the report: per level {level, count, coverage, bands: {h, v, d, a: {gain, err_mse, loss_mse,
    noise_mse}}}"""
    return [{"level": row["level"], "count": row["count"], "coverage": float(row["coverage"]),
             "bands": {k: {"gain": None if b["gain"] is None else float(b["gain"]), "err_mse": float(b["err_mse"]),
                           "loss_mse": float(b["loss_mse"]), "noise_mse": float(b["noise_mse"])}
                       for k, b in row["bands"].items()}} for row in table]


def frame_columns(M, width: int, height: int, bit_depth: int) -> dict:
    """per frame of moments [n, L, 4, 3]: detail_gain_h, detail_gain_v (the level-1 gains of H and V; 1 where the reference
    band is empty: nothing was there to lose) and noise_mse (the noise of all bands), float64 [n]"""
    S = _signed(M)
    if S.ndim != 4:
        raise ValueError("frame_columns needs per-frame moments [n, L, 4, 3]")
    n = S.shape[0]
    out = {k: np.zeros(n, np.float64) for k in ("detail_gain_h", "detail_gain_v", "noise_mse")}
    for f in range(n):
        table = band_table(S[f], width, height, bit_depth)
        for key, name in (("detail_gain_h", "h"), ("detail_gain_v", "v")):
            g = table[0]["bands"][name]["gain"]
            out[key][f] = 1.0 if g is None else float(g)
        out["noise_mse"][f] = float(sum((b["noise_mse"] for _, _, b in _parts(table)), Fraction(0)))
    return out


def analyse(M, width: int, height: int, bit_depth: int, *, min_mse=1.0, gain_floor=Fraction(1, 2)) -> dict:
    """{bands, summary} of a clip's per-frame moments [n, L, 4, 3]: the report object of one plane"""
    M = np.asarray(M)
    table = band_table(pool(M), width, height, bit_depth, frames=max(1, M.shape[0]))
    return {"bands": table_json(table), "summary": summary(table, min_mse=min_mse, gain_floor=gain_floor)}
