"""libvmaf's psnr_hvs feature restated in numpy: the repository's contract, from memory of libvmaf's psnr_hvs.c and of
Daala's od_bin_fdct8x8 (no libvmaf here, so parity is unpinned; DESIGN.md section 1 lists the VERIFY items).

Per plane, 8x8 blocks at a step of 7 (corners x = 0, 7, 14, ... while x < w - 7; the same for y).  Per block, on both
frames: the global and the four 4x4 quadrant variances give g = sum of quadrant vars / global var (0 for a flat block);
Daala's integer lifting DCT; the masks sqrt(g * sum_{AC} coef^2 M) / 32, m = the larger of the two; then
sum_{ij} (max(|coef_ref - coef_dis| - m / M_ij, 0) * CSF_ij)^2 (no threshold at DC).  mse_p = sum / (64 * blocks),
psnr_hvs_p = 10 log10(max^2 / mse_p), psnr_hvs from 0.8 mse_Y + 0.1 (mse_Cb + mse_Cr).

Two float modes: "f64" (the definition the kernel is held to; the DCT is exact integer either way) and "f32", a copy of
libvmaf's scalar f32 arithmetic including its one f32 running sum per plane (how far that drifts: DESIGN.md section 1).
Every constant of the definition is in CONST: pinning against a real libvmaf log changes that table."""
import numpy as np

CONST = {
    # blocks: 8x8, corners every `step` samples while x < w - 7 (overlap by one sample, remainders not covered)
    "block": 8, "step": 7,
    # variances scaled by n / (n - 1): 64 / 63 (global), 16 / 15 (quadrants)                 (VERIFY: as libvmaf writes them)
    "gvar_scale": 64.0 / 63.0, "qvar_scale": 16.0 / 15.0,
    # masking table M = (mask_k * CSF)^2, mask = sqrt(g * sum coef^2 M) / mask_div
    "mask_k": 0.3885746225901003, "mask_div": 32.0,
    # combination of the plane MSEs before the dB step                                          (VERIFY: weights, order)
    "weights": (0.8, 0.1, 0.1),
    # od_bin_fdct8 lifting steps (multiplier, shift): t +/-= (u * mul + (1 << (shift - 1))) >> shift   (VERIFY: constants)
    "lifts": ((13573, 15), (11585, 14), (13573, 15), (21895, 15), (15137, 14), (21895, 15), (19195, 15), (11585, 14),
              (7489, 13), (3227, 15), (6393, 15), (3227, 15), (2485, 13), (18205, 15), (2485, 13)),
    # Daala's contrast sensitivity tables; the 4:2:0 chroma tables serve every subsampling  (VERIFY: 4:2:2 / 4:4:4)
    "csf_y": (
        (1.6193873005, 2.2901594831, 2.08509755623, 1.48366094411, 1.00227514334, 0.678296995242, 0.466224900598, 0.3265091542),
        (2.2901594831, 1.94321815382, 2.04793073064, 1.68731108984, 1.2305666963, 0.868920337363, 0.61280991668, 0.436405793551),
        (2.08509755623, 2.04793073064, 1.34329019223, 1.09205635862, 0.875748795257, 0.670882927016, 0.501731932449, 0.372504254596),
        (1.48366094411, 1.68731108984, 1.09205635862, 0.772819797575, 0.605636379554, 0.48309405692, 0.380429446972, 0.295774038565),
        (1.00227514334, 1.2305666963, 0.875748795257, 0.605636379554, 0.448996256676, 0.352889268808, 0.283006984131, 0.226951348204),
        (0.678296995242, 0.868920337363, 0.670882927016, 0.48309405692, 0.352889268808, 0.27032073436, 0.215017739696, 0.17408067321),
        (0.466224900598, 0.61280991668, 0.501731932449, 0.380429446972, 0.283006984131, 0.215017739696, 0.168869545842, 0.136153931001),
        (0.3265091542, 0.436405793551, 0.372504254596, 0.295774038565, 0.226951348204, 0.17408067321, 0.136153931001, 0.109083846276)),
    "csf_cb420": (
        (1.91113096927, 2.46074210438, 1.18284184739, 1.14982565193, 1.05017074788, 0.898018824055, 0.74725392039, 0.615105596242),
        (2.46074210438, 1.58529308355, 1.21363250036, 1.38190029285, 1.33100189972, 1.17428548929, 0.996404342439, 0.830890433625),
        (1.18284184739, 1.21363250036, 0.978712413627, 1.02624506078, 1.03145147362, 0.960060382087, 0.849823426169, 0.731221236837),
        (1.14982565193, 1.38190029285, 1.02624506078, 0.861317501629, 0.801821139099, 0.751437590932, 0.685398513368, 0.608694761374),
        (1.05017074788, 1.33100189972, 1.03145147362, 0.801821139099, 0.676555426187, 0.605503172737, 0.55002013668, 0.495804539034),
        (0.898018824055, 1.17428548929, 0.960060382087, 0.751437590932, 0.605503172737, 0.514674450957, 0.454353482512, 0.407050308965),
        (0.74725392039, 0.996404342439, 0.849823426169, 0.685398513368, 0.55002013668, 0.454353482512, 0.389234902883, 0.342353999733),
        (0.615105596242, 0.830890433625, 0.731221236837, 0.608694761374, 0.495804539034, 0.407050308965, 0.342353999733, 0.295530605237)),
    "csf_cr420": (
        (2.03871978502, 2.62502345193, 1.26180942886, 1.11019789803, 1.01397751469, 0.867069376285, 0.721500455585, 0.593906509971),
        (2.62502345193, 1.69112867013, 1.17180569821, 1.3342742857, 1.28513006198, 1.13381474809, 0.962064122248, 0.802254508198),
        (1.26180942886, 1.17180569821, 0.944981930573, 0.990876405848, 0.995903384143, 0.926972725286, 0.820534991409, 0.706020324706),
        (1.11019789803, 1.3342742857, 0.990876405848, 0.831632933426, 0.77418706195, 0.725539939514, 0.661776842059, 0.587716619023),
        (1.01397751469, 1.28513006198, 0.995903384143, 0.77418706195, 0.653238524286, 0.584635025748, 0.531064164893, 0.478717061273),
        (0.867069376285, 1.13381474809, 0.926972725286, 0.725539939514, 0.584635025748, 0.496936637883, 0.438694579826, 0.393021669543),
        (0.721500455585, 0.962064122248, 0.820534991409, 0.661776842059, 0.531064164893, 0.438694579826, 0.375820256136, 0.330555063063),
        (0.593906509971, 0.802254508198, 0.706020324706, 0.587716619023, 0.478717061273, 0.393021669543, 0.330555063063, 0.285345396658)),
}
CSF_KEYS = ("csf_y", "csf_cb420", "csf_cr420")   # plane kind 0 / 1 / 2
TABLE_FLOATS = 384                               # pqa_debug_psnr_hvs_tables: CSF[3][8][8], then M[3][8][8] (f32)


def csf(kind, dtype=np.float64):
    return np.asarray(CONST[CSF_KEYS[kind]], dtype)


def mask_table(kind, dtype=np.float64):
    """M = (mask_k * CSF)^2.  f32: as libvmaf stores it (f32 CSF times the double constant, squared in double, to f32)."""
    c = csf(kind, np.float32).astype(np.float64) if dtype == np.float32 else csf(kind)
    return ((c * CONST["mask_k"]) * (c * CONST["mask_k"])).astype(dtype)


def tables_f32():
    """[384] f32: what pqa_debug_psnr_hvs_tables returns."""
    return np.concatenate([csf(k, np.float32).ravel() for k in range(3)] + [mask_table(k, np.float32).ravel() for k in range(3)])


# ---- Daala's integer DCT -----------------------------------------------------------------------------------------------
def _rshift(a, b):
    """OD_DCT_RSHIFT: arithmetic shift right rounding toward zero (the sign bit is added before the shift, int32)."""
    return (a + ((a >> 31) & ((1 << b) - 1))) >> b


def _mul(u, k, track):
    m, s = CONST["lifts"][k]
    p = u * m + (1 << (s - 1))
    if track is not None:
        track[0] = max(track[0], int(np.abs(p).max(initial=0)))
    return p >> s


def fdct8(x, track=None):
    """od_bin_fdct8 along the last axis of an int64 array; `track` ([0]): the largest |u * mul + r| seen (int32 check)."""
    t0, t4, t2, t6, t7, t3, t5, t1 = (x[..., i] for i in range(8))
    t1 = t0 - t1
    t1h = _rshift(t1, 1)
    t0 = t0 - t1h
    t4 = t4 + t5
    t4h = _rshift(t4, 1)
    t5 = t5 - t4h
    t3 = t2 - t3
    t2 = t2 - _rshift(t3, 1)
    t6 = t6 + t7
    t6h = _rshift(t6, 1)
    t7 = t6h - t7
    t0 = t0 + t6h
    t6 = t0 - t6
    t2 = t4h - t2
    t4 = t2 - t4
    t0 = t0 - _mul(t4, 0, track)
    t4 = t4 + _mul(t0, 1, track)
    t0 = t0 - _mul(t4, 2, track)
    t6 = t6 - _mul(t2, 3, track)
    t2 = t2 + _mul(t6, 4, track)
    t6 = t6 - _mul(t2, 5, track)
    t3 = t3 + _mul(t5, 6, track)
    t5 = t5 + _mul(t3, 7, track)
    t3 = t3 - _mul(t5, 8, track)
    t7 = _rshift(t5, 1) - t7
    t5 = t5 - t7
    t3 = t1h - t3
    t1 = t1 - t3
    t7 = t7 + _mul(t1, 9, track)
    t1 = t1 - _mul(t7, 10, track)
    t7 = t7 + _mul(t1, 11, track)
    t5 = t5 + _mul(t3, 12, track)
    t3 = t3 - _mul(t5, 13, track)
    t5 = t5 + _mul(t3, 14, track)
    return np.stack([t0, t1, t2, t3, t4, t5, t6, t7], axis=-1)


def fdct8x8(blocks, track=None):
    """od_bin_fdct8x8 of [..., 8, 8] integer blocks (rows i, columns j): od_bin_fdct8 down every column, the results
    written as rows, then again.  Out [..., i, j]: vertical frequency i, horizontal j (orthonormal scale)."""
    x = np.asarray(blocks, np.int64)
    z = fdct8(np.swapaxes(x, -1, -2), track)
    return fdct8(np.swapaxes(z, -1, -2), track)


# ---- blocks ----------------------------------------------------------------------------------------------------------
def n_blocks(w, h):
    """(blocks across, blocks down) of a w x h plane."""
    s = CONST["step"]
    return (max(0, (w - 1) // s) if w >= 8 else 0), (max(0, (h - 1) // s) if h >= 8 else 0)


def blocks_of(plane):
    """[nby, nbx, 8, 8] int64 blocks of a 2-D plane (row-major block order)."""
    p = np.asarray(plane, np.int64)
    nbx, nby = n_blocks(p.shape[1], p.shape[0])
    s = CONST["step"]
    iy = (np.arange(nby) * s)[:, None] + np.arange(8)[None, :]
    ix = (np.arange(nbx) * s)[:, None] + np.arange(8)[None, :]
    return p[iy[:, None, :, None], ix[None, :, None, :]]


_QUAD = ((np.arange(8)[:, None] >= 4).astype(int) + 2 * (np.arange(8)[None, :] >= 4).astype(int))   # [i][j] -> quadrant


def _g64(x):
    """g = sum of quadrant vars / global var (0 when the global var is 0), f64, over [N, 8, 8] blocks."""
    xf = x.astype(np.float64)
    gm = xf.sum((1, 2)) / 64.0
    gv = ((xf - gm[:, None, None]) ** 2).sum((1, 2)) * CONST["gvar_scale"]
    qv = np.zeros_like(gv)
    for q in range(4):
        sel = xf[:, _QUAD == q]
        qm = sel.sum(1) / 16.0
        qv += ((sel - qm[:, None]) ** 2).sum(1) * CONST["qvar_scale"]
    return np.where(gv > 0, qv / np.where(gv > 0, gv, 1.0), 0.0)


def _block_err64(xs, xd, kind):
    c_s, c_d = fdct8x8(xs), fdct8x8(xd)
    M, C = mask_table(kind), csf(kind)
    ac = np.ones((8, 8))
    ac[0, 0] = 0.0
    ms = np.sqrt(_g64(xs) * (c_s.astype(np.float64) ** 2 * M * ac).sum((1, 2))) / CONST["mask_div"]
    md = np.sqrt(_g64(xd) * (c_d.astype(np.float64) ** 2 * M * ac).sum((1, 2))) / CONST["mask_div"]
    m = np.maximum(ms, md)
    e = np.abs(c_s - c_d).astype(np.float64)
    e = np.where(ac > 0, np.maximum(e - m[:, None, None] / M, 0.0), e)
    return ((e * C) ** 2).sum((1, 2))


def _f32_terms(xs, xd, kind):
    """libvmaf's per-block scalar f32 arithmetic, in its loop order, vectorised over blocks: [N, 64] f32 terms."""
    f = np.float32
    C, M = csf(kind, f), mask_table(kind, f)
    n = xs.shape[0]
    out = []
    gs = []
    for x in (xs, xd):
        xf = x.astype(f)
        gmean = np.zeros(n, f)
        qmean = np.zeros((4, n), f)
        for i in range(8):
            for j in range(8):
                gmean = gmean + xf[:, i, j]
                qmean[_QUAD[i, j]] = qmean[_QUAD[i, j]] + xf[:, i, j]
        gmean = gmean / f(64)
        qmean = qmean / f(16)
        gvar = np.zeros(n, f)
        qvar = np.zeros((4, n), f)
        for i in range(8):
            for j in range(8):
                d = xf[:, i, j] - gmean
                gvar = gvar + d * d
                q = _QUAD[i, j]
                dq = xf[:, i, j] - qmean[q]
                qvar[q] = qvar[q] + dq * dq
        gvar = gvar * (f(1) / f(63) * f(64))
        qvar = qvar * (f(1) / f(15) * f(16))
        qsum = ((qvar[0] + qvar[1]) + qvar[2]) + qvar[3]
        with np.errstate(divide="ignore", invalid="ignore"):
            gs.append(np.where(gvar > 0, qsum / gvar, gvar).astype(f))
    cs, cd = fdct8x8(xs), fdct8x8(xd)
    masks = []
    for c, g in ((cs, gs[0]), (cd, gs[1])):
        acc = np.zeros(n, f)
        for i in range(8):
            for j in range(1 if i == 0 else 0, 8):
                acc = acc + (c[:, i, j] * c[:, i, j]).astype(f) * M[i, j]
        masks.append((np.sqrt((acc * g).astype(np.float64)) / 32.0).astype(f))
    m = np.where(masks[1] > masks[0], masks[1], masks[0])
    for i in range(8):
        for j in range(8):
            err = np.abs(cs[:, i, j] - cd[:, i, j]).astype(f)
            if i or j:
                thr = m / M[i, j]
                err = np.where(err < thr, f(0), err - thr)
            t = err * C[i, j]
            out.append(t * t)
    return np.stack(out, 1)


def block_errors(ref, dis, kind, mode="f64"):
    """[nby, nbx] per-block error sums of one plane (plane kind 0 = Y, 1 = Cb, 2 = Cr)."""
    bs, bd = blocks_of(ref), blocks_of(dis)
    shp = bs.shape[:2]
    xs, xd = bs.reshape(-1, 8, 8), bd.reshape(-1, 8, 8)
    if mode == "f64":
        return _block_err64(xs, xd, kind).reshape(shp)
    return _f32_terms(xs, xd, kind).sum(1, dtype=np.float64).reshape(shp)


def plane_mse(ref, dis, kind, mode="f64"):
    """mse_p of one plane.  f32: libvmaf's single f32 running sum over every term of every block, / (64 blocks) in f32."""
    bs, bd = blocks_of(ref), blocks_of(dis)
    nb = bs.shape[0] * bs.shape[1]
    if nb == 0:
        return float("nan")
    xs, xd = bs.reshape(-1, 8, 8), bd.reshape(-1, 8, 8)
    if mode == "f64":
        return float(_block_err64(xs, xd, kind).sum() / (64.0 * nb))
    run = np.cumsum(_f32_terms(xs, xd, kind).ravel(), dtype=np.float32)[-1]   # sequential f32 accumulation
    return float(np.float32(run) / np.float32(64 * nb))


def db(mse, bpc):
    """10 log10(max^2 / mse), max = 2^bpc - 1; +inf at mse 0."""
    if np.isnan(mse):
        return float("nan")
    peak = float((1 << bpc) - 1)
    return float("inf") if mse <= 0 else float(10.0 * np.log10(peak * peak / mse))


def psnr_hvs(ref_planes, dis_planes, bpc, mode="f64"):
    """{psnr_hvs_y, psnr_hvs_cb, psnr_hvs_cr, psnr_hvs, mse: (Y, Cb, Cr)} of one frame (three planes each)."""
    mse = tuple(plane_mse(ref_planes[k], dis_planes[k], k, mode) for k in range(3))
    wy, wb, wr = CONST["weights"]
    comb = wy * mse[0] + (wb * mse[1] + wr * mse[2])
    return {"psnr_hvs_y": db(mse[0], bpc), "psnr_hvs_cb": db(mse[1], bpc), "psnr_hvs_cr": db(mse[2], bpc),
            "psnr_hvs": db(comb, bpc), "mse": mse}
