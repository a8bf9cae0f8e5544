"""CPU restatement of libvmaf's float_ssim and float_ms_ssim features (numpy, float64; dtype=np.float32 restates the
kernels' arithmetic, see "f32 mode" below).  Test infrastructure next to
ab_vs_oracle.py: the GPU kernels (pqa2_amd/csrc/ssim_family.hip) are checked against it, and
tools/compare_libvmaf_log.py compares it with a real libvmaf log.

Definition (restated from public knowledge of the iqa-derived extractors float_ssim.c / float_ms_ssim.c; every item
marked [VERIFY] is unpinned against libvmaf and listed in DESIGN.md section 1):

- Luma only.  Samples become floats as s / 2^(bpc-8), so 10- and 12-bit clips land in 0..255.  L = 255, K1 = 0.01,
  K2 = 0.03, C1 = (K1 L)^2, C2 = (K2 L)^2, C3 = C2 / 2.  [VERIFY: picture_copy for float features]
- Window: 11 x 11 Gaussian, sigma 1.5, normalised to unit sum, applied over the VALID region only: the maps are
  (w - 10) x (h - 10).  [VERIFY: valid region; whether libvmaf's literal taps are rounded]
- Per pixel: mu_x, mu_y, sigma_x^2 = E[x^2] - mu_x^2, sigma_y^2, sigma_xy, and
      l = (2 mu_x mu_y + C1) / (mu_x^2 + mu_y^2 + C1)
      c = (2 sigma_x sigma_y + C2) / (sigma_x^2 + sigma_y^2 + C2)
      s = (sigma_xy + C3) / (sigma_x sigma_y + C3)
  with sigma_x sigma_y = sqrt(max(sigma_x^2, 0) * max(sigma_y^2, 0)).  [VERIFY: the clamp]
- float_ssim: decimation factor f = max(1, round(min(w, h) / 256)) (4 at 1080p, 8 at 2160p).  When f > 1 both planes
  are low-passed with an f x f box (window [x - f//2, x - f//2 + f) in each direction, half-sample symmetric border) and
  every f-th sample is kept, starting at 0: ceil(w / f) x ceil(h / f) samples.  float_ssim = mean of l*c*s over the
  map; the means of l, c and s are reported too.  [VERIFY: f rule, sample offset and border of iqa's _iqa_decimate]
- float_ms_ssim: five scales.  Between scales a 9 x 9 separable low-pass with the CDF 9/7 analysis taps (unit DC gain),
  half-sample symmetric border, samples 0, 2, 4, ... kept: ceil(n / 2).  [VERIFY: all three]  Per scale j the SEPARATE
  means l_j, c_j, s_j over the valid map; MS-SSIM = l_4^a4 * prod_j c_j^b_j * s_j^g_j with b = g = MS_WEIGHTS and
  a = (0, 0, 0, 0, MS_WEIGHTS[4]) (Wang 2003 as iqa states it).  [VERIFY: separate means of c and s]
- C pow semantics: x^0 = 1 for every x; a NEGATIVE mean under a fractional exponent gives NaN, which propagates into
  float_ms_ssim (a zero mean gives 0).  That is the defined outcome, on the device as here (ms_combine).
- Minimum sizes: every map non-empty -- ceil-halved 5th scale >= 11 in both directions (w, h >= 161) for MS-SSIM, the
  decimated plane >= 11 for float_ssim.  [VERIFY: libvmaf's own limit]

f32 mode (dtype=np.float32 on lcs_maps, lpf97_decimate, float_ssim, ms_ssim, ext_record; the default float64 path is
untouched, bit for bit -- tests/test_ssim_localized_ref.py holds it against a frozen copy): every filter and every map
value stays in f32, and the moments are formed on x - o with o the plane's background value (its median: on a flat frame
with a small patch that is the flat level, on any frame a value inside the sample range).  That is the kernels'
per-thread-offset formulation: variance and covariance do not change, and a flat window gives exactly zero moments.  Means
are accumulated in f64 in both modes.  The f32 mode is no second definition: it measures how far honest f32 arithmetic is
from f64 (the f32 oracle of tests/fuzz_parity.py's rule).
"""
from __future__ import annotations

import math

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

L_MAX = 255.0
K1, K2 = 0.01, 0.03
C1 = (K1 * L_MAX) ** 2
C2 = (K2 * L_MAX) ** 2
C3 = C2 / 2.0
WIN = 11
MS_SCALES = 5
MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
MS_ALPHA = (0.0, 0.0, 0.0, 0.0, 0.1333)
LPF97 = np.array([0.026748757411, -0.016864118443, -0.078223266529, 0.266864118443, 0.602949018236,
                  0.266864118443, -0.078223266529, -0.016864118443, 0.026748757411])


def gaussian_taps(n: int = WIN, sigma: float = 1.5) -> np.ndarray:
    x = np.arange(n, dtype=np.float64) - (n // 2)
    g = np.exp(-(x * x) / (2.0 * sigma * sigma))
    return g / g.sum()


def gaussian_window() -> np.ndarray:
    g = gaussian_taps()
    return np.outer(g, g)


def _is_f32(dtype) -> bool:
    dt = np.dtype(dtype)
    if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError(f"dtype must be float32 or float64, not {dt}")
    return dt == np.dtype(np.float32)


def to_float(plane: np.ndarray, bpc: int, dtype=np.float64) -> np.ndarray:
    if _is_f32(dtype):
        return np.asarray(plane, np.float32) / np.float32(1 << (bpc - 8))   # exact: integers over a power of two
    return np.asarray(plane, np.float64) / float(1 << (bpc - 8))


def decimation_factor(w: int, h: int) -> int:
    return max(1, int(math.floor(min(w, h) / 256.0 + 0.5)))


def ms_scale_sizes(w: int, h: int):
    out = [(w, h)]
    for _ in range(MS_SCALES - 1):
        w, h = (w + 1) // 2, (h + 1) // 2
        out.append((w, h))
    return out


def float_ssim_fits(w: int, h: int) -> bool:
    f = decimation_factor(w, h)
    return -(-w // f) >= WIN and -(-h // f) >= WIN


def ms_ssim_fits(w: int, h: int) -> bool:
    w4, h4 = ms_scale_sizes(w, h)[-1]
    return w4 >= WIN and h4 >= WIN


# ---- filters ----------------------------------------------------------------------------------------------------
def filter_valid_2d(img: np.ndarray, win: np.ndarray) -> np.ndarray:
    """Valid-region 2-D correlation through sliding_window_view (row blocks keep the view's working set small)."""
    kh, kw = win.shape
    oh, ow = img.shape[0] - kh + 1, img.shape[1] - kw + 1
    out = np.empty((oh, ow), img.dtype)
    step = max(1, (1 << 22) // max(1, ow * kh * kw))
    for y0 in range(0, oh, step):
        y1 = min(oh, y0 + step)
        v = sliding_window_view(img[y0:y1 + kh - 1], (kh, kw))
        out[y0:y1] = np.einsum("ijkl,kl->ij", v, win, optimize=False)
    return out


def filter_valid_sep(img: np.ndarray, g: np.ndarray) -> np.ndarray:
    """The same window as two 1-D valid passes (horizontal, then vertical)."""
    n = len(g)
    ow, oh = img.shape[1] - n + 1, img.shape[0] - n + 1
    hz = sum(g[k] * img[:, k:k + ow] for k in range(n))
    return sum(g[k] * hz[k:k + oh, :] for k in range(n))


def _sym_index(n: int, lo: int, hi: int) -> np.ndarray:
    """Indices lo..hi-1 folded by the half-sample symmetric rule: -1 -> 0, -2 -> 1, n -> n-1, n+1 -> n-2."""
    i = np.arange(lo, hi)
    i = np.where(i < 0, -1 - i, i)
    i = np.where(i >= n, 2 * n - 1 - i, i)
    return np.clip(i, 0, n - 1)


def box_decimate(img: np.ndarray, f: int) -> np.ndarray:
    if f == 1:
        return img
    h, w = img.shape
    a = f // 2
    ys = _sym_index(h, -a, h - a + f)          # window of sample y = k*f: rows k*f - a ... k*f - a + f - 1
    xs = _sym_index(w, -a, w - a + f)
    pad = img[np.ix_(ys, xs)]
    ow, oh = -(-w // f), -(-h // f)
    acc = np.zeros((oh, ow), img.dtype)
    for dy in range(f):
        for dx in range(f):
            acc += pad[dy:dy + oh * f:f, dx:dx + ow * f:f]
    return acc / img.dtype.type(f * f)      # f32 planes stay f32 (the sums are integers over a power of two: exact)


def lpf97_decimate(img: np.ndarray, dtype=np.float64) -> np.ndarray:
    taps = LPF97
    if _is_f32(dtype):
        img, taps = np.asarray(img, np.float32), LPF97.astype(np.float32)
    h, w = img.shape
    pad = img[np.ix_(_sym_index(h, -4, h + 4), _sym_index(w, -4, w + 4))]
    hz = sum(taps[k] * pad[:, k:k + w] for k in range(9))
    full = sum(taps[k] * hz[k:k + h, :] for k in range(9))
    return full[::2, ::2]


# ---- SSIM maps --------------------------------------------------------------------------------------------------
def _lcs_maps_f32(x: np.ndarray, y: np.ndarray, separable: bool):
    """lcs_maps in f32 throughout, moments about the planes' background values (the kernels' per-thread offsets)."""
    f = np.float32
    x, y = np.asarray(x, f), np.asarray(y, f)
    ox, oy = f(np.median(x)), f(np.median(y))
    if separable:
        g = gaussian_taps().astype(f)
        flt = lambda a: filter_valid_sep(a, g)  # noqa: E731
    else:
        win = gaussian_window().astype(f)
        flt = lambda a: filter_valid_2d(a, win)  # noqa: E731
    dx, dy = x - ox, y - oy
    mu, mv = flt(dx), flt(dy)
    sxx = flt(dx * dx) - mu * mu
    syy = flt(dy * dy) - mv * mv
    sxy = flt(dx * dy) - mu * mv
    mx, my = mu + ox, mv + oy
    sxsy = np.sqrt(np.maximum(sxx, f(0)) * np.maximum(syy, f(0)))
    l = (f(2) * (mx * my) + f(C1)) / ((mx * mx + my * my) + f(C1))
    c = (f(2) * sxsy + f(C2)) / ((sxx + syy) + f(C2))
    s = (sxy + f(C3)) / (sxsy + f(C3))
    assert l.dtype == c.dtype == s.dtype == f
    return l, c, s


def _mean(a: np.ndarray) -> float:
    """Mean accumulated in f64 whatever the map's type."""
    return float(a.mean()) if a.dtype == np.float64 else float(a.mean(dtype=np.float64))


def lcs_maps(x: np.ndarray, y: np.ndarray, separable: bool = False, dtype=np.float64):
    """l, c, s maps over the valid region of two float planes."""
    if _is_f32(dtype):
        return _lcs_maps_f32(x, y, separable)
    if separable:
        g = gaussian_taps()
        flt = lambda a: filter_valid_sep(a, g)  # noqa: E731
    else:
        win = gaussian_window()
        flt = lambda a: filter_valid_2d(a, win)  # noqa: E731
    mx, my = flt(x), flt(y)
    sxx = flt(x * x) - mx * mx
    syy = flt(y * y) - my * my
    sxy = flt(x * y) - mx * my
    sxsy = np.sqrt(np.maximum(sxx, 0.0) * np.maximum(syy, 0.0))
    l = (2.0 * mx * my + C1) / (mx * mx + my * my + C1)
    c = (2.0 * sxsy + C2) / (sxx + syy + C2)
    s = (sxy + C3) / (sxsy + C3)
    return l, c, s


def _cpow(b: float, e: float) -> float:
    """C pow for the cases MS-SSIM meets: x^0 = 1, negative base under a fractional exponent = NaN."""
    if e == 0.0:
        return 1.0
    if math.isnan(b) or b < 0.0:
        return float("nan")
    return b ** e


def ms_combine(lm, cm, sm) -> float:
    """MS-SSIM from per-scale means (the order of the product is the device's: c, s per scale, then l_4)."""
    v = 1.0
    for j in range(MS_SCALES):
        v *= _cpow(cm[j], MS_WEIGHTS[j]) * _cpow(sm[j], MS_WEIGHTS[j])
    return v * _cpow(lm[MS_SCALES - 1], MS_ALPHA[MS_SCALES - 1])


def float_ssim(ref: np.ndarray, dis: np.ndarray, bpc: int = 8, separable: bool = False, dtype=np.float64) -> dict:
    h, w = ref.shape
    if not float_ssim_fits(w, h):
        raise ValueError(f"{w}x{h} is too small for float_ssim")
    f = decimation_factor(w, h)
    x, y = box_decimate(to_float(ref, bpc, dtype), f), box_decimate(to_float(dis, bpc, dtype), f)
    l, c, s = lcs_maps(x, y, separable, dtype)
    return {"float_ssim": _mean(l * c * s), "l": _mean(l), "c": _mean(c), "s": _mean(s)}


def ms_ssim(ref: np.ndarray, dis: np.ndarray, bpc: int = 8, separable: bool = False, dtype=np.float64) -> dict:
    h, w = ref.shape
    if not ms_ssim_fits(w, h):
        raise ValueError(f"{w}x{h} is too small for float_ms_ssim")
    x, y = to_float(ref, bpc, dtype), to_float(dis, bpc, dtype)
    lm, cm, sm = [], [], []
    for j in range(MS_SCALES):
        l, c, s = lcs_maps(x, y, separable, dtype)
        lm.append(_mean(l)); cm.append(_mean(c)); sm.append(_mean(s))
        if j + 1 < MS_SCALES:
            x, y = lpf97_decimate(x, dtype), lpf97_decimate(y, dtype)
    return {"float_ms_ssim": ms_combine(lm, cm, sm), "l": lm, "c": cm, "s": sm}


def ext_record(ref: np.ndarray, dis: np.ndarray, bpc: int = 8, want_float_ssim: bool = True,
               want_ms_ssim: bool = True, separable: bool = True, dtype=np.float64) -> np.ndarray:
    """The 24-double extension record the library returns for this pair (PQA_EXT_* layout; NaN where not run)."""
    e = np.full(24, np.nan)
    if want_float_ssim:
        fs = float_ssim(ref, dis, bpc, separable, dtype)
        e[0:4] = [fs["float_ssim"], fs["l"], fs["c"], fs["s"]]
    if want_ms_ssim:
        ms = ms_ssim(ref, dis, bpc, separable, dtype)
        e[4] = ms["float_ms_ssim"]
        e[5:10], e[10:15], e[15:20] = ms["l"], ms["c"], ms["s"]
    return e
