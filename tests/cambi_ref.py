"""libvmaf's cambi feature (banding index) restated in numpy: the repository's contract, from memory of libvmaf's cambi.c
with default options (no libvmaf here, so parity is unpinned; DESIGN.md section 1 lists the VERIFY items).

Integer stages are exact; each c-value is an integer product converted to f32 and divided in IEEE f32, as the kernels do;
pooling is in f64.  Every constant of the definition is in CONST: pinning against a real libvmaf log changes that table."""
import math

import numpy as np

CONST = {
    # preprocessing: samples -> 10 bit (8-bit x 4, 10-bit as is), no resize                 (VERIFY: 2x2 anti-dither at 8 bit)
    "bit_depths": (8, 10),
    # spatial mask: D = 1 where a sample equals its right and lower neighbours, 7x7 box sum, M = S > T   (VERIFY: T)
    "mask_size": 7, "mask_threshold": 24,
    # window: ws = ((ws_num * (W + H)) // ws_den) >> ws_shift, r = ws >> 1                    (VERIFY: rounding)
    "ws_num": 65, "ws_den": 375, "ws_shift": 4,
    # scales: decimation by 2 and a separable 3x3 mode filter at s > 0                        (VERIFY: min vs middle, rows)
    "num_scales": 5,
    # TVI: BT.1886 EOTF, L(v + d) - L(v) > tvi_threshold * L(v)                               (VERIFY: EOTF constants)
    "eotf_gamma": 2.4, "eotf_lw": 300.0, "eotf_lb": 0.01, "black": 64, "white": 940, "tvi_threshold": 0.019,
    # c-values: max over d = 1..4 of contrast_weights[d - 1] * p0 * q / (p0 + q)              (VERIFY: weights)
    "num_diffs": 4, "contrast_weights": (1, 2, 3, 4),
    # pooling: mean of the k = clamp(int(topk * N), 1, N) largest c-values per scale, then      (VERIFY: truncation)
    # sum_s scale_weights[s] * P_s / pixels_in_window
    "topk": 0.6, "scale_weights": (16, 8, 4, 2, 1),
}
N_PARAMS = 22   # pqa_debug_cambi_params: ws, r, piw, T, tvi[4], weights[4], (w_s, h_s)[5]


def window(w, h):
    """(ws, r, pixels_in_window) at frame size w x h."""
    ws = ((CONST["ws_num"] * (w + h)) // CONST["ws_den"]) >> CONST["ws_shift"]
    r = ws >> 1
    return ws, r, (2 * r + 1) ** 2


def eotf(v):
    """BT.1886 EOTF of a 10-bit code value (cd/m^2)."""
    g, lw, lb = CONST["eotf_gamma"], CONST["eotf_lw"], CONST["eotf_lb"]
    a = (lw ** (1 / g) - lb ** (1 / g)) ** g
    b = lb ** (1 / g) / (lw ** (1 / g) - lb ** (1 / g))
    V = (v - CONST["black"]) / (CONST["white"] - CONST["black"])
    return a * max(V + b, 0.0) ** g


def tvi_for_diff():
    """[4]: the largest v in [64, 940 - d] with L(v + d) - L(v) > thr * L(v), d = 1..4 (the condition is monotone in v)."""
    out = []
    for d in range(1, CONST["num_diffs"] + 1):
        best = CONST["black"] - 1
        for v in range(CONST["black"], CONST["white"] - d + 1):
            if eotf(v + d) - eotf(v) > CONST["tvi_threshold"] * eotf(v):
                best = v
        out.append(best)
    return out


def scale_sizes(w, h):
    out = []
    for s in range(CONST["num_scales"]):
        out.append((w, h))
        w, h = (w + 1) >> 1, (h + 1) >> 1
    return out


def params(w, h):
    """The pqa_debug_cambi_params table: ws, r, pixels_in_window, T, tvi[1..4], contrast weights[4], (w_s, h_s) x 5."""
    ws, r, piw = window(w, h)
    out = [ws, r, piw, CONST["mask_threshold"], *tvi_for_diff(), *CONST["contrast_weights"]]
    for sw, sh in scale_sizes(w, h):
        out += [sw, sh]
    assert len(out) == N_PARAMS
    return out


def preprocess(y, bpc):
    if bpc not in CONST["bit_depths"]:
        raise ValueError(f"cambi: bit depth {bpc} unsupported")
    y = np.asarray(y).astype(np.int32)
    return y * 4 if bpc == 8 else y


def box_sum(a, r):
    """(2r+1)^2 box sum centred on every element, out-of-frame terms 0 (exact, int64)."""
    h, w = a.shape
    p = np.zeros((h + 2 * r + 1, w + 2 * r + 1), np.int64)
    p[r + 1:r + 1 + h, r + 1:r + 1 + w] = a
    c = p.cumsum(0).cumsum(1)
    return c[2 * r + 1:, 2 * r + 1:] - c[:h, 2 * r + 1:] - c[2 * r + 1:, :w] + c[:h, :w]


def spatial_mask(p):
    """M (bool) of a preprocessed plane: D at full resolution, its 7x7 box sum, S > T."""
    h, w = p.shape
    eq_r = np.ones((h, w), bool)
    eq_d = np.ones((h, w), bool)
    eq_r[:, :-1] = p[:, :-1] == p[:, 1:]
    eq_d[:-1, :] = p[:-1, :] == p[1:, :]
    d = (eq_r & eq_d).astype(np.int64)
    return box_sum(d, CONST["mask_size"] // 2) > CONST["mask_threshold"]


def mode3(a, b, c):
    return np.where((a == b) | (a == c), a, np.where(b == c, b, np.minimum(np.minimum(a, b), c)))


def mode_filter(x):
    """Separable 3x3 mode: horizontal over columns 1..w-2, vertical on that over rows 1..h-2; rows 0, h-1 keep x."""
    h, w = x.shape
    hz = x.copy()
    if w >= 3:
        hz[:, 1:-1] = mode3(x[:, :-2], x[:, 1:-1], x[:, 2:])
    out = x.copy()
    if h >= 3:
        out[1:-1, :] = mode3(hz[:-2, :], hz[1:-1, :], hz[2:, :])
    return out


def scales(y, bpc):
    """[(plane, mask)] for s = 0..4."""
    p = preprocess(y, bpc)
    m = spatial_mask(p)
    out = [(p, m)]
    for _ in range(1, CONST["num_scales"]):
        p = mode_filter(p[::2, ::2].copy())
        m = m[::2, ::2].copy()
        out.append((p, m))
    return out


def c_values(p, m, r, tvi):
    """f32 c-value map of one scale (0 where M = 0 or no d qualifies)."""
    h, w = p.shape
    wts = CONST["contrast_weights"]
    vmax = max(tvi)
    need = (m & (p <= vmax))
    c = np.zeros((h, w), np.float32)
    if not need.any():
        return c
    vals = np.unique(p[need])
    cnt = {}
    def count(u):   # window count of masked samples equal to u, at every centre
        if u not in cnt:
            cnt[u] = box_sum((m & (p == u)).astype(np.int64), r) if u >= 0 else np.zeros((h, w), np.int64)
        return cnt[u]
    for v in vals:
        sel = need & (p == v)
        p0 = count(v)[sel]
        best = np.zeros(p0.shape, np.float32)
        for d in range(1, CONST["num_diffs"] + 1):
            if v > tvi[d - 1]:
                continue
            q = np.maximum(count(v + d)[sel], count(v - d)[sel])
            num = (wts[d - 1] * p0 * q).astype(np.float32)
            den = (p0 + q).astype(np.float32)
            with np.errstate(divide="ignore", invalid="ignore"):
                cv = np.where(p0 + q > 0, num / np.where(den > 0, den, np.float32(1)), np.float32(0)).astype(np.float32)
            best = np.maximum(best, cv)
        c[sel] = best
    return c


def pool(c):
    """Mean of the k largest c-values (f64), k = clamp(int(topk * N), 1, N)."""
    v = np.sort(c.ravel().astype(np.float64))[::-1]
    n = v.size
    k = min(max(int(CONST["topk"] * n), 1), n)
    return float(v[:k].sum() / k)


def cambi_detail(y, bpc):
    """(cambi, [P_s], [c-map_s]) of one luma plane."""
    h, w = np.asarray(y).shape
    _, r, piw = window(w, h)
    tvi = tvi_for_diff()
    ps, cs = [], []
    for p, m in scales(y, bpc):
        c = c_values(p, m, r, tvi)
        cs.append(c)
        ps.append(pool(c))
    score = sum(wt * P for wt, P in zip(CONST["scale_weights"], ps)) / piw
    return float(score), ps, cs


def cambi(y, bpc):
    return cambi_detail(y, bpc)[0]


def full_reference(cambi_dis, cambi_src):
    """cambi_full_reference = max(cambi - cambi_source, 0)                                          (VERIFY)"""
    if math.isnan(cambi_dis) or math.isnan(cambi_src):
        return float("nan")
    return max(cambi_dis - cambi_src, 0.0)
