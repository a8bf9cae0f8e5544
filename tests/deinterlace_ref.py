"""The deinterlacer restated in numpy, int64 (csrc/deinterlace.hip, include/pqa_vmaf.h: pqa_deinterlace).

A clip has n planes S_t of w x h samples, h >= 2 (a sample above top = 2^bits - 1 is read as top); S_t with t < 0 is S_0 and
with t >= n it is S_{n-1}.  first: the parity of the rows whose field comes first in time.  An output plane is made from a
source frame t and a kept parity p: rate "frame" gives O_t = (t, first), rate "field" O_{2t} = (t, first) and
O_{2t+1} = (t, 1 - first).  q = 1 - p; P, C, N = S_{t-1}, S_t, S_{t+1}; p == first: B = P, A = C, otherwise B = C, A = N.
row(F, r, k) is row min(max(r, k), last_k) of F, last_k the largest row index below h of parity k.  Rows of parity p are C's.
Rows y of parity q (every shift an arithmetic one):

    c  = row(C, y-1, p)   e  = row(C, y+1, p)   c3 = row(C, y-3, p)   e3 = row(C, y+3, p)
    sp = (5077 (c + e) - 981 (c3 + e3)) >> 13
    intra:     O[y] = clip(sp, 0, top)
    adaptive:  s(k) = row(B, y+k, q) + row(A, y+k, q), k in {-4, -2, 0, 2, 4};  d = s(0) >> 1
               td0 = |row(B, y, q) - row(A, y, q)|;  td1 = (|row(P, y-1, p) - c| + |row(P, y+1, p) - e|) >> 1;  td2: with N
               diff = max(td0 >> 1, td1, td2);  diff == 0: O[y] = d; otherwise
               bb = (s(-2) >> 1) - c, ff = (s(2) >> 1) - e, dc = d - c, de = d - e
               diff = max(diff, min(de, dc, max(bb, ff)), -max(de, dc, min(bb, ff)))
               v = |c - e| > td0 ? (((5570 s(0) - 3801 (s(-2) + s(2)) + 1016 (s(-4) + s(4))) >> 2) + 4309 (c + e) - 213 (c3 + e3)) >> 13 : sp
               O[y] = clip(clip(v, d - diff, d + diff), 0, top)

deinterlace(..., stats=dict) also counts, over the interpolated samples of the adaptive mode, the branches taken (still,
temporal, spatial, clamp) and keeps the largest magnitude any intermediate reached."""
import numpy as np

MODES = ("intra", "adaptive")
RATES = ("frame", "field")


def _row(F, r, k):
    h = F.shape[0]
    last = h - 1 - ((h - 1 - k) & 1)
    return F[min(max(r, k), last)]


def _note(stats, *values):
    if stats is not None:
        stats["peak"] = max(stats.get("peak", 0), *(int(np.abs(v).max()) for v in values))


def one_plane(P, C, N, p, first, mode, top, stats=None):
    """the output plane of the kept parity p of C between P and N (int64 planes, none above top)"""
    h = C.shape[0]
    q = 1 - p
    B, A = (P, C) if p == first else (C, N)
    O = C.copy()
    for y in range(q, h, 2):
        c, e, c3, e3 = _row(C, y - 1, p), _row(C, y + 1, p), _row(C, y - 3, p), _row(C, y + 3, p)
        sp_sum = 5077 * (c + e) - 981 * (c3 + e3)
        sp = sp_sum >> 13
        if mode == "intra":
            _note(stats, sp_sum)
            O[y] = np.clip(sp, 0, top)
            continue
        s = {k: _row(B, y + k, q) + _row(A, y + k, q) for k in (-4, -2, 0, 2, 4)}
        d = s[0] >> 1
        td0 = np.abs(_row(B, y, q) - _row(A, y, q))
        td1 = (np.abs(_row(P, y - 1, p) - c) + np.abs(_row(P, y + 1, p) - e)) >> 1
        td2 = (np.abs(_row(N, y - 1, p) - c) + np.abs(_row(N, y + 1, p) - e)) >> 1
        diff0 = np.maximum(td0 >> 1, np.maximum(td1, td2))
        bb, ff, dc, de = (s[-2] >> 1) - c, (s[2] >> 1) - e, d - c, d - e
        hi = np.maximum(np.maximum(de, dc), np.minimum(bb, ff))
        lo = np.minimum(np.minimum(de, dc), np.maximum(bb, ff))
        diff = np.maximum(diff0, np.maximum(lo, -hi))
        t_sum = 5570 * s[0] - 3801 * (s[-2] + s[2]) + 1016 * (s[-4] + s[4])
        v_sum = (t_sum >> 2) + 4309 * (c + e) - 213 * (c3 + e3)
        temporal = np.abs(c - e) > td0
        v = np.where(temporal, v_sum >> 13, sp)
        moved = np.clip(np.clip(v, d - diff, d + diff), 0, top)
        O[y] = np.where(diff0 == 0, d, moved)
        _note(stats, sp_sum, t_sum, v_sum, d + diff, d - diff)
        if stats is not None:
            live = diff0 != 0
            stats["samples"] = stats.get("samples", 0) + live.size
            stats["still"] = stats.get("still", 0) + int((~live).sum())
            stats["temporal"] = stats.get("temporal", 0) + int((live & temporal).sum())
            stats["spatial"] = stats.get("spatial", 0) + int((live & ~temporal).sum())
            stats["clamp"] = stats.get("clamp", 0) + int((live & ((v < d - diff) | (v > d + diff))).sum())
    return O


def deinterlace(frames, mode="adaptive", first=0, rate="frame", bits=8, stats=None):
    """the n or 2 n output planes of the n source planes `frames`, in their dtype"""
    assert mode in MODES and rate in RATES and first in (0, 1)
    top = (1 << bits) - 1
    S = [np.minimum(np.asarray(f).astype(np.int64), top) for f in frames]
    n = len(S)
    out = []
    for t in range(n):
        P, C, N = S[max(t - 1, 0)], S[t], S[min(t + 1, n - 1)]
        for p in ((first,) if rate == "frame" else (first, 1 - first)):
            out.append(one_plane(P, C, N, p, first, mode, top, stats).astype(np.asarray(frames[0]).dtype))
    return out


def interlace(planes, first=0):
    """2 n progressive planes woven into n frames: the rows of parity `first` from plane 2 t, the others from plane 2 t + 1"""
    out = []
    for t in range(len(planes) // 2):
        f = planes[2 * t].copy()
        f[1 - first::2] = planes[2 * t + 1][1 - first::2]
        out.append(f)
    return out


def psnr(a, b, top=255):
    mse = float(((np.asarray(a).astype(np.int64) - np.asarray(b).astype(np.int64)) ** 2).mean())
    return 10.0 * np.log10(top * top / mse) if mse else float("inf")


def half_static_clip(seed, bits, w=70, h=21, shift=0):
    """three planes of noise whose columns below w // 2 + shift are the same in all three"""
    rng = np.random.default_rng(seed)
    top = (1 << bits) - 1
    dt = np.uint8 if bits == 8 else np.uint16
    frames = [rng.integers(0, top + 1, (h, w)).astype(dt) for _ in range(3)]
    for f in frames[1:]:
        f[:, :w // 2 + shift] = frames[0][:, :w // 2 + shift]
    return frames


def extreme_planes(bits, w=8, h=12):
    """all 0, all top, the one-row checker and its inverse, the two-row checker and its inverse"""
    top = (1 << bits) - 1
    dt = np.uint8 if bits == 8 else np.uint16
    y, x = np.mgrid[0:h, 0:w]
    one, two = ((y + x) & 1) * top, (((y >> 1) + x) & 1) * top
    return [a.astype(dt) for a in (np.zeros((h, w)), np.full((h, w), top), one, top - one, two, top - two)]
