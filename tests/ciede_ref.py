"""libvmaf's ciede feature (log key `ciede2000`) restated in numpy: YUV -> RGB -> linear sRGB -> XYZ -> Lab per luma
pixel, the CIEDE2000 colour difference (Sharma, Wu & Dalal 2005) of each reference / distorted pixel pair, the frame
mean and the score 45 - 20 * log10(mean).  f64 by default; dtype=np.float32 evaluates the same expressions in f32 (the
frame mean is still accumulated in f64) to state how far f32 evaluation alone sits from f64.

Every constant of the definition is in CONST: pinning against a real libvmaf log changes that table only.  The items
DESIGN.md section 1 lists as VERIFY are marked there and below."""
import math

import numpy as np

CONST = {
    # sample normalisation: s = 2^(bpc - 8); Y = y / (255 s), U = u / (255 s) - chroma_offset        (VERIFY: 0.5 or 128/255)
    "full_scale": 255.0,
    "chroma_offset": 0.5,
    # BT.709 analog Y'UV -> R'G'B', no clamp to [0, 1]                                              (VERIFY: matrix, clamp)
    "r_v": 1.28033, "g_u": -0.21482, "g_v": -0.38059, "b_u": 2.12798,
    # sRGB transfer: c > thr ? ((c + off) / (1 + off))^gamma : c / lin_slope, then x 100
    "srgb_thr": 0.04045, "srgb_off": 0.055, "srgb_gamma": 2.4, "srgb_lin_slope": 12.92, "srgb_scale": 100.0,
    # linear sRGB -> XYZ, 4-digit D65 matrix                                                        (VERIFY: vs 7-digit)
    "xyz": ((0.4124, 0.3576, 0.1805), (0.2126, 0.7152, 0.0722), (0.0193, 0.1192, 0.9505)),
    # Lab: white point, f(t) = t > eps ? cbrt(t) : kappa * t + 16 / 116
    "white": (95.047, 100.0, 108.883), "lab_eps": 0.008856, "lab_kappa": 7.787,
    # CIEDE2000 weights kL = kC = kH = 1
    "kL": 1.0, "kC": 1.0, "kH": 1.0,
    # score = score_offset - score_gain * log10(mean dE00); mean 0 -> +inf                         (VERIFY: value at 0)
    "score_offset": 45.0, "score_gain": 20.0,
}


def de00(L1, a1, b1, L2, a2, b2, dtype=np.float64):
    """CIEDE2000 of Lab pairs (broadcasting arrays), Sharma et al. 2005 eqs. (2)-(21): h' = 0 where a' = b = 0, the
    hue-difference and hue-mean rules of eqs. (10) and (14) as published."""
    f = lambda v: np.asarray(v, dtype)
    L1, a1, b1, L2, a2, b2 = map(f, (L1, a1, b1, L2, a2, b2))
    c = lambda v: dtype(v)
    C1, C2 = np.hypot(a1, b1), np.hypot(a2, b2)
    Cb = (C1 + C2) * c(0.5)
    Cb7 = Cb ** 7
    G = c(0.5) * (c(1) - np.sqrt(Cb7 / (Cb7 + c(25.0 ** 7))))
    a1p, a2p = (c(1) + G) * a1, (c(1) + G) * a2
    C1p, C2p = np.hypot(a1p, b1), np.hypot(a2p, b2)
    deg = c(180.0 / math.pi)
    h1 = np.where((a1p == 0) & (b1 == 0), c(0), np.mod(np.arctan2(b1, a1p) * deg, c(360)))
    h2 = np.where((a2p == 0) & (b2 == 0), c(0), np.mod(np.arctan2(b2, a2p) * deg, c(360)))
    h1 = np.where(h1 >= 360, h1 - c(360), h1)   # mod of a tiny negative angle may round to 360 itself
    h2 = np.where(h2 >= 360, h2 - c(360), h2)
    dL = L2 - L1
    dC = C2p - C1p
    zero = C1p * C2p == 0
    dh = h2 - h1
    dh = np.where(dh > 180, dh - c(360), np.where(dh < -180, dh + c(360), dh))
    dh = np.where(zero, c(0), dh)
    dH = c(2) * np.sqrt(C1p * C2p) * np.sin(dh / deg * c(0.5))
    Lb = (L1 + L2) * c(0.5)
    Cbp = (C1p + C2p) * c(0.5)
    hs = h1 + h2
    hb = np.where(np.abs(h1 - h2) <= 180, hs * c(0.5), np.where(hs < 360, (hs + c(360)) * c(0.5), (hs - c(360)) * c(0.5)))
    hb = np.where(zero, hs, hb)
    r = lambda d: (hb + c(d)) / deg
    T = (c(1) - c(0.17) * np.cos(r(-30)) + c(0.24) * np.cos(c(2) * hb / deg) + c(0.32) * np.cos((c(3) * hb + c(6)) / deg)
         - c(0.20) * np.cos((c(4) * hb - c(63)) / deg))
    dtheta = c(30) * np.exp(-(((hb - c(275)) / c(25)) ** 2))
    Cbp7 = Cbp ** 7
    RC = c(2) * np.sqrt(Cbp7 / (Cbp7 + c(25.0 ** 7)))
    l50 = (Lb - c(50)) ** 2
    SL = c(1) + c(0.015) * l50 / np.sqrt(c(20) + l50)
    SC = c(1) + c(0.045) * Cbp
    SH = c(1) + c(0.015) * Cbp * T
    RT = -np.sin(c(2) * dtheta / deg) * RC
    tl = dL / (c(CONST["kL"]) * SL)
    tc = dC / (c(CONST["kC"]) * SC)
    th = dH / (c(CONST["kH"]) * SH)
    return np.sqrt(tl * tl + tc * tc + th * th + RT * tc * th)


def hue_delta_from_180(L1, a1, b1, L2, a2, b2):
    """| |h1' - h2'| - 180 | in degrees (f64): how close a pair sits to the hue-mean discontinuity of ΔE00."""
    a1, b1, a2, b2 = (np.asarray(v, np.float64) for v in (a1, b1, a2, b2))
    Cb = (np.hypot(a1, b1) + np.hypot(a2, b2)) * 0.5
    G = 0.5 * (1 - np.sqrt(Cb ** 7 / (Cb ** 7 + 25.0 ** 7)))
    h1 = np.mod(np.degrees(np.arctan2(b1, (1 + G) * a1)), 360)
    h2 = np.mod(np.degrees(np.arctan2(b2, (1 + G) * a2)), 360)
    return np.abs(np.abs(h1 - h2) - 180)


def upsample(plane, w, h, hs, vs):
    """Chroma plane -> luma size by replication: luma (x, y) takes chroma (x >> hs, y >> vs)."""
    p = np.asarray(plane)
    return np.repeat(np.repeat(p, 1 << vs, axis=0), 1 << hs, axis=1)[:h, :w]


def yuv_to_lab(y, u, v, bpc, hs=1, vs=1, dtype=np.float64):
    """Luma plane y (h x w) and chroma planes u, v -> (L, a, b) per luma pixel."""
    c = lambda x: dtype(x)
    h, w = np.asarray(y).shape
    s = c(CONST["full_scale"] * (1 << (bpc - 8)))
    Y = np.asarray(y, dtype) / s
    U = upsample(u, w, h, hs, vs).astype(dtype) / s - c(CONST["chroma_offset"])
    V = upsample(v, w, h, hs, vs).astype(dtype) / s - c(CONST["chroma_offset"])
    R = Y + c(CONST["r_v"]) * V
    G = Y + c(CONST["g_u"]) * U + c(CONST["g_v"]) * V
    B = Y + c(CONST["b_u"]) * U

    def lin(x):   # negative values take the linear branch
        xp = np.maximum(x, c(CONST["srgb_thr"]))
        pw = ((xp + c(CONST["srgb_off"])) / c(1 + CONST["srgb_off"])) ** c(CONST["srgb_gamma"])
        return np.where(x > c(CONST["srgb_thr"]), pw, x / c(CONST["srgb_lin_slope"])) * c(CONST["srgb_scale"])

    R, G, B = lin(R), lin(G), lin(B)
    m = CONST["xyz"]
    X = c(m[0][0]) * R + c(m[0][1]) * G + c(m[0][2]) * B
    Yy = c(m[1][0]) * R + c(m[1][1]) * G + c(m[1][2]) * B
    Z = c(m[2][0]) * R + c(m[2][1]) * G + c(m[2][2]) * B

    def f(t):     # negative values take the linear branch
        tp = np.maximum(t, c(CONST["lab_eps"]))
        return np.where(t > c(CONST["lab_eps"]), np.cbrt(tp), c(CONST["lab_kappa"]) * t + c(16.0 / 116.0))

    wx, wy, wz = CONST["white"]
    fx, fy, fz = f(X / c(wx)), f(Yy / c(wy)), f(Z / c(wz))
    return c(116) * fy - c(16), c(500) * (fx - fy), c(200) * (fy - fz)


def frame_de(ref_planes, dis_planes, bpc, hs=1, vs=1, dtype=np.float64):
    """Per-pixel ΔE00 map of one frame (planes: [Y, U, V] of the reference and the distorted frame)."""
    Lr = yuv_to_lab(*ref_planes[:3], bpc, hs, vs, dtype)
    Ld = yuv_to_lab(*dis_planes[:3], bpc, hs, vs, dtype)
    return de00(*Lr, *Ld, dtype=dtype)


def score(mean_de):
    """libvmaf's ciede2000 value of a frame from its mean ΔE00 (in double; mean 0 gives +inf)."""
    m = float(mean_de)
    if m == 0.0:
        return math.inf
    return CONST["score_offset"] - CONST["score_gain"] * math.log10(m)


def frame_slots(ref_planes, dis_planes, bpc, hs=1, vs=1, dtype=np.float64):
    """(ciede2000, mean ΔE00) of one frame: extension slots 20 and 21."""
    mean = float(np.mean(frame_de(ref_planes, dis_planes, bpc, hs, vs, dtype).astype(np.float64)))
    return score(mean), mean
