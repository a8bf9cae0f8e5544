"""Delta E ITP (ITU-R BT.2124): the spec of a measurement and what its sums say.

The measurement is FeatureEngine.delta_itp (pqa_delta_itp, csrc/delta_itp.hip): per frame pair the 8 sums of
include/pqa_vmaf.h.  `spec` builds the two matrices the kernel takes -- Y'CbCr code values -> R'G'B' from Kr, Kb, the range
and the bit depth, and linear display light -> LMS / 10000 from the primaries -- in Fractions, rounded once; `summary` turns
the rows of a clip into per-frame figures, a pooled mean and a verdict.  Pins: BT.2100 (PQ, HLG, ICtCp), BT.2124 (the 720 and
T = Ct / 2), BT.2087 (709 -> 2020), BT.1886 (the 2.4 power at 100 cd/m2)."""
from fractions import Fraction

import numpy as np

from . import _native as N
from .align import COLOUR_STANDARDS

TRANSFERS = {"pq": N.ITP_PQ, "hlg": N.ITP_HLG, "bt1886": N.ITP_BT1886}
DEFAULT_PEAK = {"pq": 10000.0, "hlg": 1000.0, "bt1886": 100.0}   # cd/m2; PQ does not read it
SUM_DE, SUM_DI2, SUM_DT2, SUM_DP2, MAX_DE, ABOVE, PIXELS, SUM_I = range(8)   # a row of FeatureEngine.delta_itp

# BT.2100 R G B (BT.2020 primaries) -> L M S
RGB_TO_LMS = [[Fraction(v, 4096) for v in row] for row in ((1688, 2146, 262), (683, 2951, 462), (99, 309, 3688))]
# BT.2087: linear BT.709 R G B -> linear BT.2020 R G B
BT709_TO_BT2020 = [[Fraction(v, 10000) for v in row] for row in ((6274, 3293, 433), (691, 9195, 114), (164, 880, 8956))]
PRIMARIES = {"bt2020": "bt2020", "bt709": "bt709", "bt601": "bt709"}   # the primaries a matrix name stands for (bt601: taken as 709's)


def decode_matrix(matrix: str, full_range: bool, bit_depth: int):
    """3 x 4 Fractions: rows of [Y Cb Cr 1] in code values -> R'G'B' with nominal range 0 ... 1.  Limited range: Y 16 ... 235,
    C 128 +- 112 times 2^(b - 8); full: Y 0 ... 2^b - 1, C 2^(b - 1) +- (2^b - 1) / 2."""
    if matrix not in COLOUR_STANDARDS:
        raise ValueError(f"unknown matrix {matrix!r} (one of {', '.join(sorted(COLOUR_STANDARDS))})")
    b = int(bit_depth)
    if not 8 <= b <= 16:
        raise ValueError("bit_depth must be 8 ... 16")
    kr, kb = (Fraction(v) for v in COLOUR_STANDARDS[matrix])
    kg = 1 - kr - kb
    if full_range:
        y0, ys, c0, cs = Fraction(0), Fraction((1 << b) - 1), Fraction(1 << (b - 1)), Fraction((1 << b) - 1)
    else:
        f = 1 << (b - 8)
        y0, ys, c0, cs = Fraction(16 * f), Fraction(219 * f), Fraction(128 * f), Fraction(224 * f)
    # R' = Y + 2 (1 - Kr) Cr, B' = Y + 2 (1 - Kb) Cb, G' = (Y - Kr R' - Kb B') / Kg on normalised Y, Cb, Cr
    rows = [(Fraction(1), Fraction(0), 2 * (1 - kr)),
            (Fraction(1), -2 * kb * (1 - kb) / kg, -2 * kr * (1 - kr) / kg),
            (Fraction(1), 2 * (1 - kb), Fraction(0))]
    out = []
    for gy, gu, gv in rows:
        gy, gu, gv = gy / ys, gu / cs, gv / cs
        out.append([gy, gu, gv, -(gy * y0 + (gu + gv) * c0)])
    return out


def lms_matrix(primaries: str):
    """3 x 3 Fractions: linear display light in cd/m2 of `primaries` ("bt2020" or "bt709") -> LMS / 10000"""
    if primaries not in ("bt2020", "bt709"):
        raise ValueError('primaries must be "bt2020" or "bt709"')
    m = RGB_TO_LMS
    if primaries == "bt709":
        m = [[sum(m[r][k] * BT709_TO_BT2020[k][c] for k in range(3)) for c in range(3)] for r in range(3)]
    return [[v / 10000 for v in row] for row in m]


def spec(transfer: str, matrix: str | None = None, full_range: bool = False, bit_depth: int = 10, peak: float | None = None,
         threshold: float = 1.0, height: int | None = None) -> dict:
    """The spec of a measurement: {"transfer", "matrix", "primaries", "range", "bit_depth", "peak", "threshold", "yuv_to_rgb"
    (12 floats), "rgb_to_lms" (9 floats)}, the coefficients rounded to f32 as the kernel takes them.  `matrix` None: "bt2020"
    for pq and hlg, rgb.default_matrix(height) for bt1886.  `peak` None: 1000 cd/m2 for hlg, 100 for bt1886."""
    if transfer not in TRANSFERS:
        raise ValueError(f"delta_itp transfer must be one of {', '.join(TRANSFERS)}")
    if matrix is None:
        if transfer == "bt1886":
            from .rgb import default_matrix
            matrix = default_matrix(height if height is not None else 1080)
        else:
            matrix = "bt2020"
    peak = DEFAULT_PEAK[transfer] if peak is None else float(peak)
    threshold = float(threshold)
    if not (np.isfinite(peak) and peak > 0):
        raise ValueError("itp_peak must be positive")
    if not (np.isfinite(threshold) and threshold >= 0):
        raise ValueError("itp_threshold must not be negative")
    dec = decode_matrix(matrix, bool(full_range), bit_depth)
    prim = PRIMARIES[matrix]
    f32 = lambda rows: [float(np.float32(float(v))) for row in rows for v in row]
    return {"transfer": transfer, "matrix": matrix, "primaries": prim, "range": "full" if full_range else "limited",
            "bit_depth": int(bit_depth), "peak": peak, "threshold": threshold, "yuv_to_rgb": f32(dec), "rgb_to_lms": f32(lms_matrix(prim))}


def native_spec(sp: dict) -> "N.PqaItpSpec":
    """the pqa_itp_spec of a spec()"""
    s = N.PqaItpSpec()
    s.transfer = TRANSFERS[sp["transfer"]]
    s.yuv_to_rgb[:] = [float(v) for v in sp["yuv_to_rgb"]]
    s.rgb_to_lms[:] = [float(v) for v in sp["rgb_to_lms"]]
    s.peak, s.threshold = float(sp["peak"]), float(sp["threshold"])
    return s


def frame_columns(rows) -> dict:
    """per-frame columns of rows [n, 8]: delta_e_itp (mean dE), delta_e_itp_max, itp_above_jnd (share of pixels above the
    threshold)"""
    R = np.asarray(rows, np.float64).reshape(-1, N.ITP_SUMS)
    px = np.maximum(R[:, PIXELS], 1.0)
    return {"delta_e_itp": R[:, SUM_DE] / px, "delta_e_itp_max": R[:, MAX_DE].copy(), "itp_above_jnd": R[:, ABOVE] / px}


def summary(rows, threshold: float = 1.0) -> dict:
    """What the rows [n, 8] of a clip say.  Per frame: mean dE, max dE, the share of pixels above the threshold.  Pooled over
    all pixels of the clip: mean dE, rms dE, the share above the threshold, the worst frame (largest mean), the largest dE, and
    the split of sum dE^2 = sum dI^2 + (sum dT^2 + sum dP^2) into its luminance and chroma shares.
    kind, in this order:
      "identical"  every sum is zero;
      "below_jnd"  the largest dE of the clip does not exceed the threshold: no pixel differs visibly;
      "luminance"  at least 3/4 of sum dE^2 is dI^2;
      "chroma"     at least 3/4 of sum dE^2 is dT^2 + dP^2;
      "mixed"      otherwise."""
    R = np.asarray(rows, np.float64).reshape(-1, N.ITP_SUMS)
    if R.shape[0] == 0:
        raise ValueError("no rows")
    cols = frame_columns(R)
    px = float(R[:, PIXELS].sum())
    lum, chroma = float(R[:, SUM_DI2].sum()), float(R[:, SUM_DT2].sum() + R[:, SUM_DP2].sum())
    total = lum + chroma
    max_de = float(R[:, MAX_DE].max())
    if total == 0.0 and max_de == 0.0 and not R[:, SUM_DE].any():
        kind = "identical"
    elif max_de <= threshold:
        kind = "below_jnd"
    elif lum >= 0.75 * total:
        kind = "luminance"
    elif chroma >= 0.75 * total:
        kind = "chroma"
    else:
        kind = "mixed"
    worst = int(np.argmax(cols["delta_e_itp"]))
    return {"frames": int(R.shape[0]), "threshold": float(threshold), "kind": kind,
            "mean": float(R[:, SUM_DE].sum() / max(px, 1.0)), "rms": float(np.sqrt(total / max(px, 1.0))),
            "max": max_de, "above_jnd": float(R[:, ABOVE].sum() / max(px, 1.0)),
            "luminance_share": lum / total if total > 0 else 0.0, "chroma_share": chroma / total if total > 0 else 0.0,
            "worst_frame": worst, "worst_frame_mean": float(cols["delta_e_itp"][worst]),
            "mean_intensity": float(R[:, SUM_I].sum() / max(px, 1.0)),
            "per_frame": {k: [float(v) for v in col] for k, col in cols.items()}}
