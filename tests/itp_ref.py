"""Delta E ITP (ITU-R BT.2124) restated in numpy: f64 by default, every operation in f32 with dtype=np.float32.

Written from the recommendations, independent of pqa2_amd/itp.py:
  BT.2100  PQ (ST 2084) EOTF and its inverse, the HLG inverse OETF and OOTF, RGB -> LMS, L'M'S' -> ICtCp
  BT.2124  dE_ITP = 720 sqrt(dI^2 + dT^2 + dP^2), T = Ct / 2
  BT.2087  linear BT.709 RGB -> linear BT.2020 RGB
  BT.1886  L = Lw max(V, 0)^2.4 (zero black level)
The f32 mode is the yardstick of the GPU tests: its distance from the f64 mode on the same inputs is what plain f32 arithmetic
with correctly rounded powers costs."""
import numpy as np

M1, M2 = 2610 / 16384, 2523 / 4096 * 128
C1, C2, C3 = 3424 / 4096, 2413 / 4096 * 32, 2392 / 4096 * 32
HLG_A, HLG_B, HLG_C = 0.17883277, 0.28466892, 0.55991073
RGB_TO_LMS = np.array([[1688, 2146, 262], [683, 2951, 462], [99, 309, 3688]], np.float64) / 4096
LMS_TO_ICTCP = np.array([[2048, 2048, 0], [6610, -13613, 7003], [17933, -17390, -543]], np.float64) / 4096
BT709_TO_BT2020 = np.array([[0.6274, 0.3293, 0.0433], [0.0691, 0.9195, 0.0114], [0.0164, 0.0880, 0.8956]])
KR_KB = {"bt2020": (0.2627, 0.0593), "bt709": (0.2126, 0.0722), "bt601": (0.299, 0.114)}
SCALE = np.array([720.0, 360.0, 720.0])   # (I, Ct, Cp) -> (dI, dT, dP) units


def pq_eotf(e, dtype=np.float64):
    """signal in [0, 1] -> luminance / 10000"""
    t = dtype
    p = np.power(np.asarray(e, t), t(1 / M2))
    return np.power(np.maximum(p - t(C1), t(0)) / (t(C2) - t(C3) * p), t(1 / M1))


def pq_inverse(y, dtype=np.float64):
    """luminance / 10000 >= 0 -> signal"""
    t = dtype
    yp = np.power(np.asarray(y, t), t(M1))
    return np.power((t(C1) + t(C2) * yp) / (t(1) + t(C3) * yp), t(M2))


def hlg_inverse_oetf(e, dtype=np.float64):
    t = dtype
    e = np.asarray(e, t)
    hi = (np.exp((e - t(HLG_C)) / t(HLG_A)) + t(HLG_B)) / t(12)
    return np.where(e <= t(0.5), e * e / t(3), hi).astype(t)


def hlg_gamma(peak):
    return 1.2 + 0.42 * np.log10(peak / 1000.0)


def decode_matrix(matrix, full_range, bit_depth):
    """[3, 4] f64: rows of [Y Cb Cr 1] in code values -> R'G'B'"""
    kr, kb = KR_KB[matrix]
    kg = 1 - kr - kb
    if full_range:
        y0, ys, c0, cs = 0.0, (1 << bit_depth) - 1.0, float(1 << (bit_depth - 1)), (1 << bit_depth) - 1.0
    else:
        f = 1 << (bit_depth - 8)
        y0, ys, c0, cs = 16.0 * f, 219.0 * f, 128.0 * f, 224.0 * f
    g = np.array([[1, 0, 2 * (1 - kr)], [1, -2 * kb * (1 - kb) / kg, -2 * kr * (1 - kr) / kg], [1, 2 * (1 - kb), 0]], np.float64)
    g = g / np.array([ys, cs, cs])
    return np.column_stack([g, -(g[:, 0] * y0 + (g[:, 1] + g[:, 2]) * c0)])


def lms_matrix(primaries):
    """[3, 3] f64: display light in cd/m2 -> LMS / 10000"""
    m = RGB_TO_LMS @ BT709_TO_BT2020 if primaries == "bt709" else RGB_TO_LMS
    return m / 10000.0


DEFAULT_PEAK = {"pq": 10000.0, "hlg": 1000.0, "bt1886": 100.0}


def make_spec(transfer, matrix=None, full_range=False, bit_depth=10, peak=None, threshold=1.0):
    matrix = matrix or ("bt2020" if transfer != "bt1886" else "bt709")
    return {"transfer": transfer, "yuv_to_rgb": decode_matrix(matrix, full_range, bit_depth),
            "rgb_to_lms": lms_matrix("bt2020" if matrix == "bt2020" else "bt709"),
            "peak": DEFAULT_PEAK[transfer] if peak is None else float(peak), "threshold": float(threshold)}


def display_light(rgb, transfer, peak, dtype=np.float64):
    """R'G'B' [..., 3] -> display light in cd/m2"""
    t = dtype
    rgb = np.asarray(rgb, t)
    if transfer == "pq":
        return pq_eotf(np.clip(rgb, t(0), t(1)), t) * t(10000)
    if transfer == "hlg":
        e = hlg_inverse_oetf(np.maximum(rgb, t(0)), t)
        ys = t(0.2627) * e[..., 0] + t(0.6780) * e[..., 1] + t(0.0593) * e[..., 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            s = np.where(ys > 0, t(peak) * np.power(ys, t(hlg_gamma(peak) - 1.0)), t(0)).astype(t)
        return s[..., None] * e
    if transfer == "bt1886":
        return t(peak) * np.power(np.maximum(rgb, t(0)), t(2.4))
    raise ValueError(transfer)


def ictcp(yuv, spec, dtype=np.float64):
    """code triples [..., 3] = (Y, Cb, Cr) -> (720 I, 360 Ct, 720 Cp) [..., 3]"""
    t = dtype
    yuv = np.asarray(yuv, t)
    m = np.asarray(spec["yuv_to_rgb"], np.float64).reshape(3, 4).astype(t)
    rgb = yuv[..., 0:1] * m[:, 0] + yuv[..., 1:2] * m[:, 1] + yuv[..., 2:3] * m[:, 2] + m[:, 3]
    f = display_light(rgb, spec["transfer"], spec["peak"], t)
    q = np.asarray(spec["rgb_to_lms"], np.float64).reshape(3, 3).astype(t)
    lms = np.maximum(f[..., 0:1] * q[:, 0] + f[..., 1:2] * q[:, 1] + f[..., 2:3] * q[:, 2], t(0))
    p = pq_inverse(lms, t)
    c = LMS_TO_ICTCP.astype(t)
    out = p[..., 0:1] * c[:, 0] + p[..., 1:2] * c[:, 1] + p[..., 2:3] * c[:, 2]
    return (out * SCALE.astype(t)).astype(t)


def delta_e(yuv_ref, yuv_dis, spec, dtype=np.float64):
    """(dE, dI, dT, dP) of code triples [..., 3]"""
    d = ictcp(yuv_ref, spec, dtype) - ictcp(yuv_dis, spec, dtype)
    return np.sqrt((d * d).sum(axis=-1)), d[..., 0], d[..., 1], d[..., 2]


def upsample(frame, hs, vs):
    """[h, w, 3] code triples of a frame [Y, Cb, Cr]: chroma by replication"""
    y, u, v = (np.asarray(p) for p in frame)
    h, w = y.shape
    up = lambda c: np.repeat(np.repeat(c, 1 << vs, axis=0), 1 << hs, axis=1)[:h, :w]
    return np.stack([y, up(u), up(v)], axis=-1).astype(np.float64)


def frame_de(ref, dis, spec, hs, vs, dtype=np.float64):
    """the dE map [h, w] of a frame pair, and the reference's 720 I"""
    a, b = upsample(ref, hs, vs), upsample(dis, hs, vs)
    ia, ib = ictcp(a, spec, dtype), ictcp(b, spec, dtype)
    d = ia - ib
    return np.sqrt((d * d).sum(axis=-1)), d, ia[..., 0]


def frame_sums(ref, dis, spec, hs, vs, dtype=np.float64):
    """the 8 sums of include/pqa_vmaf.h, f64 accumulation"""
    de, d, i_ref = frame_de(ref, dis, spec, hs, vs, dtype)
    de, d = de.astype(np.float64), d.astype(np.float64)
    return np.array([de.sum(), (d[..., 0] ** 2).sum(), (d[..., 1] ** 2).sum(), (d[..., 2] ** 2).sum(), de.max(),
                     float((de > spec["threshold"]).sum()), float(de.size), i_ref.astype(np.float64).sum() / 720.0])
