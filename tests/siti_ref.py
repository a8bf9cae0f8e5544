"""Restatement of FFmpeg's siti filter (libavfilter/vf_siti.c): ITU-T P.910 Spatial Information (SI) and Temporal
Information (TI) of a luma plane, written from the definition (parity with FFmpeg is unpinned; the items to verify are
VERIFY below and in DESIGN.md section 1).

Per frame, on the luma plane only:
  1. a limited-range clip is mapped to full range first: y' = ((256 f - 1) clamp(y - 16 f, 0, 219 f)) // (219 f), f = 1 at
     8 bit and 4 at 10 bit (truncating integer division); a full-range clip is used as it is;
  2. SI: the population standard deviation of the 3 x 3 Sobel magnitude g over the interior (w - 2) x (h - 2) pixels,
     g = f32(sqrt(f64(f32(gx^2) + f32(gy^2))));
  3. TI: the population standard deviation of m = y'_t - y'_{t-1} over the whole plane; m = 0 on the first frame of a
     chain.
Two modes for the standard deviation: "ffmpeg" copies the types of FFmpeg's std_deviation (double mean, float deviation
and square, double sum, float result); "f64" is the plain double two-pass value.  Clip summaries (print_summary): the
average, max and min of the per-frame values, summed in float ("ffmpeg") or double ("f64")."""
import math

import numpy as np

CONST = {
    "factor": {8: 1, 10: 4},        # f: limited-range levels scale with the bit depth (12 bit: no siti format)
    "limited_black": 16,            # y - 16 f, clamped to [0, 219 f]
    "limited_span": 219,            # 219 f luma steps in limited range
    "full_upper": 256,              # (256 f - 1): the full-range top   -- VERIFY
    "sobel_x": ((1, 0, -1), (2, 0, -2), (1, 0, -1)),
    "sobel_y": ((1, 2, 1), (0, 0, 0), (-1, -2, -1)),
    "min_size": 3,                  # the interior map needs w, h >= 3
}

VERIFY = (
    "full_upper = 256 f - 1 and the truncating division of the range conversion",
    "the conversion is skipped exactly when the clip says full range (Y4M XCOLORRANGE=FULL); no range counts as limited",
    "g = f32(sqrt(f64(f32(gx^2) + f32(gy^2)))): where the float roundings happen",
    "std_deviation: deviation and its square rounded to float before the double sum",
    "TI = 0 on the first frame (no previous frame) rather than no value",
    "print_summary sums SI and TI in float",
)


def to_full(y, bpc: int, full: bool = False) -> np.ndarray:
    """Luma samples -> full range (exact integers)."""
    y = np.asarray(y, np.int64)
    if full:
        return y
    f = CONST["factor"][bpc]
    c = np.clip(y - CONST["limited_black"] * f, 0, CONST["limited_span"] * f)
    return ((CONST["full_upper"] * f - 1) * c) // (CONST["limited_span"] * f)


def sobel(yf: np.ndarray):
    """(gx, gy) on the interior pixels of a full-range plane, exact int64 [(h - 2), (w - 2)]."""
    p = np.asarray(yf, np.int64)
    h, w = p.shape
    gx = np.zeros((h - 2, w - 2), np.int64)
    gy = np.zeros((h - 2, w - 2), np.int64)
    for j in range(3):
        for i in range(3):
            win = p[j:j + h - 2, i:i + w - 2]
            gx += CONST["sobel_x"][j][i] * win
            gy += CONST["sobel_y"][j][i] * win
    return gx, gy


def gradient_map(yf: np.ndarray) -> np.ndarray:
    """The f32 gradient magnitude map [(h - 2), (w - 2)] of a full-range plane."""
    gx, gy = sobel(yf)
    s = (gx * gx).astype(np.float32) + (gy * gy).astype(np.float32)
    return np.sqrt(s.astype(np.float64)).astype(np.float32)


def std(x, mode: str = "f64") -> float:
    """Population standard deviation; "ffmpeg" copies std_deviation's types, "f64" is the double two-pass value."""
    v = np.asarray(x).ravel()
    if mode == "f64":
        d = v.astype(np.float64)
        m = d.mean()
        return float(np.sqrt(np.mean((d - m) ** 2)))
    f = v.astype(np.float32)
    mean = float(np.cumsum(f.astype(np.float64))[-1]) / f.size          # double accumulation, in order
    dev = (f.astype(np.float64) - mean).astype(np.float32)               # float mean_diff
    sq = dev * dev                                                       # float product
    return float(np.float32(math.sqrt(float(np.cumsum(sq.astype(np.float64))[-1]) / f.size)))


def ti_exact(m: np.ndarray) -> float:
    """TI from the exact integer sums: sqrt(N sum m^2 - (sum m)^2) / N."""
    m = np.asarray(m, np.int64).ravel()
    n, s1, s2 = m.size, int(m.sum()), int((m * m).sum())
    return math.sqrt((n * s2 - s1 * s1) / (n * n))


def frame(cur, prev, bpc: int, full: bool = False, mode: str = "f64"):
    """(SI, TI) of one luma plane; prev None = the first frame of a chain (TI = 0)."""
    yc = to_full(cur, bpc, full)
    si = std(gradient_map(yc), mode)
    if prev is None:
        return si, 0.0
    m = yc - to_full(prev, bpc, full)
    return si, (std(m.astype(np.float32), mode) if mode == "ffmpeg" else ti_exact(m))


def clip(lumas, bpc: int, full: bool = False, mode: str = "f64", prev=None):
    """Per-frame SI and TI arrays of a run of luma planes; prev (nullable) is the plane in front of the first one."""
    si, ti = [], []
    for k, y in enumerate(lumas):
        s, t = frame(y, lumas[k - 1] if k > 0 else prev, bpc, full, mode)
        si.append(s)
        ti.append(t)
    return np.array(si), np.array(ti)


def summary(si, ti, mode: str = "f64") -> dict:
    """print_summary: average, max and min of SI and of TI."""
    out = {}
    for name, v in (("si", np.asarray(si)), ("ti", np.asarray(ti))):
        if mode == "ffmpeg":
            avg = float(np.cumsum(v.astype(np.float32))[-1] / np.float32(v.size))
        else:
            avg = float(v.mean())
        out[name] = {"avg": avg, "max": float(v.max()), "min": float(v.min())}
    return out
