"""numpy restatement of FFmpeg's xpsnr filter (libavfilter/vf_xpsnr.c) as DESIGN.md section 1 writes it down: the block
size, the spatial high-pass (per sample, or per 2 x 2 group above 2048 x 1152), the temporal term of the previous one or
two reference frames, the weights, the minimum smoothing, WSSE, per-frame dB and the clip summary.  Written from the
definition, not from the kernels: integer work in int64 numpy, the weights and sums as sequential Python doubles."""
from __future__ import annotations

import math

import numpy as np

GAMMA = 2


def block_size(w: int, h: int) -> int:
    r = (w * h) / (3840.0 * 2160.0)
    return 4 * int(32.0 * math.sqrt(r) + 0.5)


def bv_of(w: int, h: int) -> int:
    return 2 if w * h > 2048 * 1152 else 1


def amplitude(w: int, h: int, bit_depth: int) -> float:
    r = (w * h) / (3840.0 * 2160.0)
    return math.sqrt(16.0 * float(1 << (2 * bit_depth - 9)) / math.sqrt(max(0.00001, r)))


def _shift(P, pad, dy, dx, h, w):
    return P[pad + dy:pad + dy + h, pad + dx:pad + dx + w]


def highpass(o: np.ndarray, bv: int) -> np.ndarray:
    """|f| at every sample (bv 1) or at every even (y, x) (bv 2, the group's top-left sample); zeros outside the plane
    (never read: the picture-edge margins exclude those positions)."""
    h, w = o.shape
    pad = 3
    P = np.zeros((h + 2 * pad, w + 2 * pad), np.int64)
    P[pad:pad + h, pad:pad + w] = o
    s = lambda dy, dx: _shift(P, pad, dy, dx, h, w)   # noqa: E731
    if bv == 1:
        f = 12 * s(0, 0) - 2 * (s(0, -1) + s(0, 1) + s(-1, 0) + s(1, 0)) - (s(-1, -1) + s(-1, 1) + s(1, -1) + s(1, 1))
        return np.abs(f)
    f = (12 * (s(0, 0) + s(0, 1) + s(1, 0) + s(1, 1))
         - 3 * (s(-1, 0) + s(-1, 1) + s(2, 0) + s(2, 1))
         - 3 * (s(0, -1) + s(1, -1) + s(0, 2) + s(1, 2))
         - 2 * (s(-1, -1) + s(-1, 2) + s(2, -1) + s(2, 2))
         - (s(-2, -1) + s(-2, 0) + s(-2, 1) + s(-2, 2) + s(3, -1) + s(3, 0) + s(3, 1) + s(3, 2)
            + s(-1, -2) + s(0, -2) + s(1, -2) + s(2, -2) + s(-1, 3) + s(0, 3) + s(1, 3) + s(2, 3)))
    return np.abs(f[::2, ::2])


def _sum22(a: np.ndarray) -> np.ndarray:
    return a[::2, ::2] + a[::2, 1::2] + a[1::2, ::2] + a[1::2, 1::2]


def temporal(o, o1, o2, bv: int, hfr: bool) -> np.ndarray:
    """|t| per sample (bv 1) or per 2 x 2 group (bv 2); o1 / o2 None = zero planes."""
    o = o.astype(np.int64)
    z = np.zeros_like(o)
    p1 = z if o1 is None else o1.astype(np.int64)
    p2 = z if o2 is None else o2.astype(np.int64)
    if bv == 2:
        o, p1, p2 = _sum22(o), _sum22(p1), _sum22(p2)
    return np.abs(o - 2 * p1 + p2) if hfr else np.abs(o - p1)


def blocks(o, o1, o2, r, hfr: bool):
    """Luma blocks in raster order: list of dicts {x0, y0, bw, bh, xa, wa, ya, ha, sse, sa, ta} (sa = ta = 0 and one
    block covering the plane when b < 4)."""
    h, w = o.shape
    b = block_size(w, h)
    bv = bv_of(w, h)
    d = o.astype(np.int64) - r.astype(np.int64)
    sq = d * d
    if b < 4:
        return [dict(x0=0, y0=0, bw=w, bh=h, xa=0, wa=w, ya=0, ha=h, sse=int(sq.sum()), sa=0, ta=0, act=False)]
    hp = highpass(o.astype(np.int64), bv)
    tt = temporal(o, o1, o2, bv, hfr)
    out = []
    for y0 in range(0, h, b):
        bh = min(b, h - y0)
        for x0 in range(0, w, b):
            bw = min(b, w - x0)
            xa = bv if x0 == 0 else 0
            wa = bw - bv if x0 + bw >= w else bw
            ya = bv if y0 == 0 else 0
            ha = bh - bv if y0 + bh >= h else bh
            blk = dict(x0=x0, y0=y0, bw=bw, bh=bh, xa=xa, wa=wa, ya=ya, ha=ha,
                       sse=int(sq[y0:y0 + bh, x0:x0 + bw].sum()), sa=0, ta=0, act=wa > xa and ha > ya)
            if blk["act"]:
                if bv == 1:
                    blk["sa"] = int(hp[y0 + ya:y0 + ha, x0 + xa:x0 + wa].sum())
                    blk["ta"] = GAMMA * int(tt[y0:y0 + bh, x0:x0 + bw].sum())
                else:
                    blk["sa"] = int(hp[(y0 + ya) // 2:(y0 + ha) // 2, (x0 + xa) // 2:(x0 + wa) // 2].sum())
                    blk["ta"] = GAMMA * int(tt[y0 // 2:(y0 + bh) // 2, x0 // 2:(x0 + bw) // 2].sum())
            out.append(blk)
    return out


def block_weight(blk: dict, bit_depth: int) -> float:
    if not blk["act"]:
        return 1.0
    ms = blk["sa"] / (float(blk["wa"] - blk["xa"]) * float(blk["ha"] - blk["ya"]))
    ms += blk["ta"] / (float(blk["bw"]) * float(blk["bh"]))
    lo = float(1 << (bit_depth - 6))
    if ms < lo:
        ms = lo
    ms *= ms
    return 1.0 / math.sqrt(ms)


def smooth(wts: list, w: int, h: int, b: int) -> list:
    """The in-line minimum smoothing of frames <= 640 x 480, sequential over the raster (a copy is returned)."""
    wt = list(wts)
    w_blk = (w + b - 1) // b
    k = 0
    for y in range(0, h, b):
        for x in range(0, w, b):
            if x == 0:
                p = wt[k - 2] if k > 1 else 0.0
            else:
                p = max(wt[k - 2], wt[k]) if x > b else wt[k]
            if k > w_blk:
                p = max(p, wt[k - 1 - w_blk])
            if k > 0 and wt[k - 1] > p:
                wt[k - 1] = p
            if x + b >= w and y + b >= h and k > w_blk:
                p = max(wt[k - 1], wt[k - w_blk])
                if wt[k] > p:
                    wt[k] = p
            k += 1
    return wt


def chroma_sse_blocks(oc, rc, w: int, h: int):
    """SSE of the chroma blocks (b * wc) / w x (b * hc) / h in raster order."""
    hc, wc = oc.shape
    b = block_size(w, h)
    bx, by = (b * wc) // w, (b * hc) // h
    d = oc.astype(np.int64) - rc.astype(np.int64)
    sq = d * d
    return [int(sq[y:y + by, x:x + bx].sum()) for y in range(0, hc, by) for x in range(0, wc, bx)]


def frame(ref_planes, dis_planes, o1, o2, bit_depth: int, hfr: bool = False):
    """One frame: (wsse [planes] ints, db [planes], luma blocks, weights).  ref_planes / dis_planes: Y (and U, V) arrays;
    o1 / o2: the reference luma one / two frames earlier (None = zero plane)."""
    o, r = ref_planes[0], dis_planes[0]
    h, w = o.shape
    b = block_size(w, h)
    blks = blocks(o, o1, o2, r, hfr)
    wsse = []
    wts = None
    if b < 4:
        for p in range(len(ref_planes)):
            d = ref_planes[p].astype(np.int64) - dis_planes[p].astype(np.int64)
            wsse.append(int((d * d).sum()))
    else:
        A = amplitude(w, h, bit_depth)
        wts = [block_weight(k, bit_depth) for k in blks]
        if w * h <= 640 * 480:
            wts = smooth(wts, w, h, b)
        s = 0.0
        for k, blk in enumerate(blks):
            s += float(blk["sse"]) * wts[k]
        wsse.append(0 if s <= 0.0 else int(s * A + 0.5))
        for p in range(1, len(ref_planes)):
            sc = 0.0
            for k, e in enumerate(chroma_sse_blocks(ref_planes[p], dis_planes[p], w, h)):
                sc += float(e) * wts[k]
            wsse.append(0 if sc <= 0.0 else int(sc * A + 0.5))
    db = [frame_db(wsse[p], ref_planes[p].shape[1], ref_planes[p].shape[0], bit_depth) for p in range(len(wsse))]
    return wsse, db, blks, wts


def frame_db(wsse: int, w: int, h: int, bit_depth: int) -> float:
    if wsse == 0:
        return math.inf
    mx = (1 << bit_depth) - 1
    return 10.0 * math.log10(float(mx * mx * w * h) / float(wsse))


def clip(refs, diss, bit_depth: int, hfr: bool = False, history=(None, None)):
    """Every frame of a chain; history = (frame -1, frame -2) luma planes in front of it (None: zero, a chain start).
    Returns (wsse [n][planes], db [n][planes])."""
    h1, h2 = history
    W, D = [], []
    for i in range(len(refs)):
        o1 = refs[i - 1][0] if i >= 1 else h1
        o2 = refs[i - 2][0] if i >= 2 else (h1 if i == 1 else h2)
        wsse, db, _, _ = frame(refs[i], diss[i], o1, o2, bit_depth, hfr)
        W.append(wsse)
        D.append(db)
    return np.array(W, dtype=np.float64), np.array(D, dtype=np.float64)


def summary(wsse, db, plane_sizes, bit_depth: int):
    """FFmpeg's clip aggregate per plane (square-mean-root, or the mean dB when sum sqrt(WSSE) < N)."""
    wsse = np.asarray(wsse, dtype=np.float64)
    n = wsse.shape[0]
    out = []
    mx = (1 << bit_depth) - 1
    for p in range(wsse.shape[1]):
        w, h = plane_sizes[p]
        s = 0.0
        for x in wsse[:, p]:
            s += math.sqrt(x)
        if s >= n:
            avg = s / n
            out.append(10.0 * math.log10(float(w * h * mx * mx) / (avg * avg)))
        else:
            t = 0.0
            for x in np.asarray(db)[:, p]:
                t += float(x)
            out.append(t / n)
    return out
