"""Temporal distortion: whether the MOTION of a captured clip is wrong.  Pure Python and numpy, no GPU: the solver behind
score_files(temporal=T).  The measurement is FeatureEngine.temporal_moments (pqa_temporal_moments, csrc/temporal_moments.hip):
with R_f the reference and D_f the captured plane of frame f and, per pixel of transition k = 1 ... n - 1,

    a = R_k - R_{k-1}      b = D_k - D_{k-1}      e = D_k - R_k

the exact sums M[k-1, j, i, 0..6] = sum a, sum b, sum a^2, sum b^2, sum a b, sum a e, sum e^2 over tile (i, j) of T x T pixels
(words 0, 1, 4, 5 are int64 stored in the uint64 word).

a is what moved in the reference, b what moved in the capture.  The least-squares temporal gain g = sum ab / sum a^2 and the
residual sum b^2 - g^2 sum a^2 split the temporal squared error EXACTLY, as spectrum.split does for a band:

    sum (b - a)^2 = sum a^2 - 2 sum ab + sum b^2 = (1 - g)^2 sum a^2  +  (sum b^2 - g^2 sum a^2) = loss + noise

loss is motion the chain removed (a temporal denoiser, a frame blend, a burnt-in logo over moving picture: gain 0 in its
tiles); noise is change the reference does not have (fresh noise, flicker, level pumping, an error pattern that jumps at a
keyframe).  A tile that does not move (sum a^2 = 0) has no gain and all of its change is noise.  The split is formed PER TILE on
the clip-summed moments and then added: a gain that differs from tile to tile would read as noise in a global fit.

A capture that mixes the previous reference frame in, d = (1 - beta) r_k + beta r_{k-1}, has e = -beta a, so
beta = -sum ae / sum a^2 is the blend weight and sum e^2 - (sum ae)^2 / sum a^2 what of the error the blend does not explain.

Units.  x / N with N the pixels summed is a mean squared error per pixel; divided by 4^(b - 8) it is in 8-bit code values
squared.  Every decision is taken on Python ints and Fractions; floats are formed only by the functions that build the report."""
from fractions import Fraction

import numpy as np

from . import distortion as DM
from .spectrum import _ratio, split

SUM_A, SUM_B, SUM_AA, SUM_BB, SUM_AB, SUM_AE, SUM_EE = range(7)
SUMS = 7
SIGNED = (SUM_A, SUM_B, SUM_AB, SUM_AE)
KINDS = ("identical", "clean", "blend", "loss", "noise")


def _signed(M) -> np.ndarray:
    """the moments as Python ints in an object array; words 0, 1, 4 and 5 are int64 stored in the word"""
    M = np.asarray(M)
    if M.dtype != np.uint64 or M.ndim < 1 or M.shape[-1] != SUMS:
        raise ValueError("temporal moments are uint64 [..., 7]")
    S = M.astype(object)
    for k in SIGNED:
        S[..., k] = np.ascontiguousarray(M[..., k]).view(np.int64).astype(object)
    return S


def _check(M) -> np.ndarray:
    M = np.asarray(M)
    if M.dtype != np.uint64 or M.ndim != 4 or M.shape[-1] != SUMS:
        raise ValueError("temporal moments are uint64 [n - 1, ty, tx, 7]")
    return M


def _sum_words(S) -> list:
    """the seven words of an object array [..., 7] added over every other axis, as Python ints"""
    flat = S.reshape(-1, SUMS)
    return [int(sum(flat[:, k].tolist())) for k in range(SUMS)]


def pool(M) -> np.ndarray:
    """object [ty, tx, 7]: the clip-summed moments of every tile as Python ints, exact"""
    S = _signed(_check(M))
    out = np.zeros(S.shape[1:], object)
    for f in range(S.shape[0]):
        out = out + S[f]
    return out


def blend(aa: int, ae: int, ee: int):
    """(beta, residual) as Fractions: the weight of the previous reference frame in the captured one and the part of sum e^2
    it leaves unexplained; (None, sum e^2) where nothing moved"""
    aa, ae, ee = int(aa), int(ae), int(ee)
    if aa == 0:
        return None, Fraction(ee)
    return Fraction(-ae, aa), ee - Fraction(ae * ae, aa)


def frame_table(M, width: int, height: int, bit_depth: int) -> list:
    """per transition k = 1 ... n - 1 a dict from the frame's summed tiles: frame (k), sums (the seven ints), motion_mse =
    sum a^2 / N, temporal_mse = sum (b - a)^2 / N, gain (None where nothing moved), blend, blend_residual, level_step =
    (sum b - sum a) / N, and the split loss, noise, loss_mse, noise_mse; Fractions, the MSEs in 8-bit code values squared, the
    level step in 8-bit code values"""
    S = _signed(_check(M))
    n_pix = int(width) * int(height)
    down = 4 ** (int(bit_depth) - 8)
    unit = Fraction(1, n_pix * down)
    rows = []
    for k in range(S.shape[0]):
        w = _sum_words(S[k])
        g, err, loss, noise = split(w[SUM_AA], w[SUM_BB], w[SUM_AB])
        beta, resid = blend(w[SUM_AA], w[SUM_AE], w[SUM_EE])
        rows.append({"frame": k + 1, "sums": w, "motion_mse": w[SUM_AA] * unit, "temporal_mse": err * unit, "gain": g,
                     "blend": beta, "blend_residual": resid, "level_step": Fraction(w[SUM_B] - w[SUM_A], n_pix * 2 ** (int(bit_depth) - 8)),
                     "err": err, "loss": loss, "noise": noise, "loss_mse": loss * unit, "noise_mse": noise * unit})
    return rows


def tile_table(M_sum, width: int, height: int, tile: int, bit_depth: int, transitions: int = 1) -> dict:
    """per tile of clip-summed moments [ty, tx, 7] (pool(), or uint64 of one transition): {gain (object [ty, tx]: Fraction or
    None), err, loss, noise (object [ty, tx]: Fractions, err == loss + noise), temporal_mse, loss_mse, noise_mse (float64
    [ty, tx], 8-bit code values squared per pixel and transition), counts (int64 [ty, tx])}"""
    S = M_sum if isinstance(M_sum, np.ndarray) and M_sum.dtype == object else _signed(M_sum)
    counts = DM.tile_counts(width, height, tile)
    if S.ndim != 3 or S.shape[:2] != counts.shape:
        raise ValueError("tile_table needs moments [ty, tx, 7] of this plane's grid")
    down = 4 ** (int(bit_depth) - 8)
    gain, err, loss, noise = (np.empty(counts.shape, object) for _ in range(4))
    mse = {k: np.zeros(counts.shape, np.float64) for k in ("temporal_mse", "loss_mse", "noise_mse")}
    for j in range(counts.shape[0]):
        for i in range(counts.shape[1]):
            gain[j, i], err[j, i], loss[j, i], noise[j, i] = split(S[j, i, SUM_AA], S[j, i, SUM_BB], S[j, i, SUM_AB])
            den = int(counts[j, i]) * max(1, int(transitions)) * down
            for key, v in (("temporal_mse", err[j, i]), ("loss_mse", loss[j, i]), ("noise_mse", noise[j, i])):
                mse[key][j, i] = float(v / den)
    return {"gain": gain, "err": err, "loss": loss, "noise": noise, "counts": counts, **mse}


def heatmap_pgm(tiles: dict, bit_depth: int = 8) -> bytes:
    """A binary P5 image, one pixel per tile, of a tile_table: the temporal error of a tile as a PSNR through
    distortion.heatmap_pgm (black: 50 dB and better, white: 20 dB and worse)"""
    mse = np.asarray(tiles["temporal_mse"], np.float64)
    with np.errstate(divide="ignore"):
        psnr = np.where(mse > 0, 10.0 * np.log10(255.0 ** 2 / np.where(mse > 0, mse, 1.0)), DM.psnr_cap(8))
    return DM.heatmap_pgm(np.minimum(psnr, DM.psnr_cap(8)))


def still_noise(M, width: int, height: int, tile: int, bit_depth: int, still_mse=Fraction(1, 4)):
    """(sum b^2, pixels) as ints over the tile transitions that do not move: sum a^2 <= still_mse * 4^(b - 8) * pixels of the
    tile.  What changes in the capture where the reference stands still: flicker, level pumping, fresh noise."""
    M = _check(M)
    bound = _ratio(still_mse) * 4 ** (int(bit_depth) - 8)
    if bound < 0:
        raise ValueError("temporal thresholds are not negative")
    counts = DM.tile_counts(width, height, tile)
    if M.shape[1:3] != counts.shape:
        raise ValueError("the moments are not of this plane's grid")
    # sum a^2 < 2^36 and the denominator of a _ratio is at most 2^16, the pixels of a tile at most 2^12: uint64 holds both sides
    still = M[..., SUM_AA] * np.uint64(bound.denominator) <= (counts.astype(np.uint64) * np.uint64(bound.numerator))[None]
    bb = int(sum(M[..., SUM_BB][still].tolist()))
    pix = int(sum(np.broadcast_to(counts[None], still.shape)[still].tolist()))
    return bb, pix


def find_pops(noise: list, n_pix: int, bit_depth: int, *, pop_factor=4, min_mse=1.0):
    """(pops, pop_period): the transitions k (frame numbers) whose noise exceeds pop_factor times the clip's median transition
    noise AND min_mse (8-bit code values squared per pixel); the period is the most frequent gap between consecutive pops if
    it accounts for at least half the gaps and there are at least two gaps, else None.  noise: one Fraction a transition,
    transition 1 first.  The median of an even number is the mean of the middle two."""
    factor, floor = _ratio(pop_factor), _ratio(min_mse) * 4 ** (int(bit_depth) - 8) * int(n_pix)
    if factor < 0 or floor < 0:
        raise ValueError("temporal thresholds are not negative")
    if not noise:
        return [], None
    srt = sorted(noise)
    m = len(srt)
    median = srt[m // 2] if m % 2 else (srt[m // 2 - 1] + srt[m // 2]) / 2
    pops = [k + 1 for k, v in enumerate(noise) if v > factor * median and v > floor]
    gaps = [q - p for p, q in zip(pops, pops[1:])]
    period = None
    if len(gaps) >= 2:
        best = max(sorted(set(gaps)), key=gaps.count)   # the smallest of equally frequent gaps
        if 2 * gaps.count(best) >= len(gaps):
            period = best
    return pops, period


def summary(M, width: int, height: int, tile: int, bit_depth: int, *, min_mse=1.0, blend_min=Fraction(1, 16),
            still_mse=Fraction(1, 4), pop_factor=4) -> dict:
    """what the clip's moments [n - 1, ty, tx, 7] say in one object.  Exact fields (Python ints / Fractions): err, loss, noise
    (err == loss + noise, the split per tile on the clip-summed moments, added over tiles), blend, blend_residual (on the
    clip's totals), pops, pop_period; floats for the report: motion_mse, temporal_mse, loss_mse, noise_mse, spatial_mse
    (sum e^2 over frames 1 ... n - 1), gain (of the totals), loss_share, noise_share, still_noise_mse (None where no tile
    transition stands still), still_share (of the pixels), level_step_max; kind, decided in this order: identical (no
    temporal error), clean (temporal_mse below min_mse), blend (blend >= blend_min and 2 blend_residual <= sum e^2), loss
    (loss >= noise), noise.  min_mse and still_mse are in 8-bit code values squared; the four thresholds are settings of this
    report, not measurements."""
    M = _check(M)
    v_min, v_blend = _ratio(min_mse), _ratio(blend_min)
    if v_min < 0 or v_blend < 0:
        raise ValueError("temporal thresholds are not negative")
    trans = M.shape[0]
    n_pix = int(width) * int(height)
    down = 4 ** (int(bit_depth) - 8)
    tiles = pool(M)
    tot = _sum_words(tiles) if trans else [0] * SUMS
    err = loss = noise = Fraction(0)
    for j in range(tiles.shape[0]):
        for i in range(tiles.shape[1]):
            _, e_t, l_t, n_t = split(tiles[j, i, SUM_AA], tiles[j, i, SUM_BB], tiles[j, i, SUM_AB])
            err, loss, noise = err + e_t, loss + l_t, noise + n_t
    beta, resid = blend(tot[SUM_AA], tot[SUM_AE], tot[SUM_EE])
    rows = frame_table(M, width, height, bit_depth)
    pops, period = find_pops([r["noise"] for r in rows], n_pix, bit_depth, pop_factor=pop_factor, min_mse=min_mse)
    bb_still, pix_still = still_noise(M, width, height, tile, bit_depth, still_mse)
    den = n_pix * max(trans, 1) * down
    if err == 0:
        kind = "identical"
    elif err < v_min * den:
        kind = "clean"
    elif beta is not None and beta >= v_blend and 2 * resid <= tot[SUM_EE]:
        kind = "blend"
    elif loss >= noise:
        kind = "loss"
    else:
        kind = "noise"
    share = (lambda x: float(x / err)) if err else (lambda x: 0.0)
    g_tot = split(tot[SUM_AA], tot[SUM_BB], tot[SUM_AB])[0]
    return {"kind": kind, "transitions": int(trans), "err": err, "loss": loss, "noise": noise, "blend": beta, "blend_residual": resid,
            "pops": pops, "pop_period": period,
            "motion_mse": float(Fraction(tot[SUM_AA], den)), "temporal_mse": float(err / den), "loss_mse": float(loss / den),
            "noise_mse": float(noise / den), "spatial_mse": float(Fraction(tot[SUM_EE], den)),
            "gain": None if g_tot is None else float(g_tot), "loss_share": share(loss), "noise_share": share(noise),
            "blend_weight": None if beta is None else float(beta),
            "blend_residual_share": float(resid / tot[SUM_EE]) if tot[SUM_EE] else 0.0,
            "still_noise_mse": float(Fraction(bb_still, pix_still * down)) if pix_still else None,
            "still_share": float(Fraction(pix_still, n_pix * trans)) if trans else 0.0,
            "level_step_max": max((abs(float(r["level_step"])) for r in rows), default=0.0),
            "min_mse": float(v_min), "blend_min": float(v_blend), "still_mse": float(_ratio(still_mse)),
            "pop_factor": float(_ratio(pop_factor))}


def summary_json(s: dict) -> dict:
    """the summary with floats only: the exact fields err, loss, noise, blend and blend_residual are dropped (their floats are
    temporal_mse, loss_mse, noise_mse, blend_weight and blend_residual_share)"""
    return {k: v for k, v in s.items() if k not in ("err", "loss", "noise", "blend", "blend_residual")}


def table_json(rows) -> list:
    """the frame table with floats for the report: per transition {frame, motion_mse, temporal_mse, gain, blend_weight,
    level_step, loss_mse, noise_mse}"""
    opt = lambda v: None if v is None else float(v)
    return [{"frame": r["frame"], "motion_mse": float(r["motion_mse"]), "temporal_mse": float(r["temporal_mse"]),
             "gain": opt(r["gain"]), "blend_weight": opt(r["blend"]), "level_step": float(r["level_step"]),
             "loss_mse": float(r["loss_mse"]), "noise_mse": float(r["noise_mse"])} for r in rows]


def frame_columns(M, width: int, height: int, bit_depth: int) -> dict:
    """per FRAME of a clip of n = len(M) + 1 frames: temporal_gain, temporal_noise_mse and blend_weight of the transition
    into the frame, float64 [n].  Frame 0 has no predecessor and carries the neutral values 1, 0 and 0, as `motion` carries 0
    there; so does a transition in which nothing moved (no gain to lose, no weight to find)."""
    rows = frame_table(M, width, height, bit_depth)
    n = len(rows) + 1
    out = {"temporal_gain": np.ones(n, np.float64), "temporal_noise_mse": np.zeros(n, np.float64),
           "blend_weight": np.zeros(n, np.float64)}
    for r in rows:
        k = r["frame"]
        if r["gain"] is not None:
            out["temporal_gain"][k] = float(r["gain"])
            out["blend_weight"][k] = float(r["blend"])
        out["temporal_noise_mse"][k] = float(r["noise_mse"])
    return out


def analyse(M, width: int, height: int, tile: int, bit_depth: int, *, min_mse=1.0, blend_min=Fraction(1, 16),
            still_mse=Fraction(1, 4), pop_factor=4) -> dict:
    """{summary, frames} of a clip's moments [n - 1, ty, tx, 7]: the report object of one plane, floats only"""
    s = summary(M, width, height, tile, bit_depth, min_mse=min_mse, blend_min=blend_min, still_mse=still_mse,
                pop_factor=pop_factor)
    return {"summary": summary_json(s), "frames": table_json(frame_table(M, width, height, bit_depth))}
