"""The host-frame staging that every side analysis and plane transform shares (csrc/pqa_side.hip, csrc/host_stage.h), on the
MI355X, past its second chunk: a context with max_batch = 2 stages 2 frames of its own size per pinned chunk, so 7 frames
make four chunks, the last one partial -- a pinned chunk packed again before its upload has left it, or a wrong slot behind
a ring wrap, changes the integers.  Every result is compared with the numpy restatements as integers; refused calls leave
the context usable, and each of the older entries keeps the answers it has always given."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import align_ref as AR
from tests import level_ref as LR
from tests import spatial_align_ref as SR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, N = 48, 32, 7


def _engine(w=W, h=H, bpc=8, **kw):
    from pqa2_amd import _native as Nt
    from pqa2_amd.engine import FeatureEngine
    return FeatureEngine(w, h, bit_depth=bpc, n_planes=kw.pop("n_planes", 1), features=kw.pop("features", Nt.FEAT_PSNR), max_batch=2, **kw)


def _padded(frames, pad=5, lead=1):
    """the same frames as views into one buffer: rows `pad` samples longer than a row, base `lead` samples in"""
    h, w = frames[0].shape
    buf = np.zeros((len(frames), h, w + pad), frames[0].dtype)
    buf[:, :, lead:lead + w] = np.stack(frames)
    return buf, [buf[i, :, lead:lead + w] for i in range(len(frames))]


def _on_device(buf, lead):
    """(tensor kept alive, device address of frame 0's first sample, row pitch, frame pitch) of a [n, h, pitch] buffer"""
    import torch
    t = torch.from_numpy(buf.view(np.uint8).reshape(-1)).cuda()
    torch.cuda.synchronize()
    return t, t.data_ptr() + lead * buf.dtype.itemsize, buf.strides[1], buf.strides[0]


def _distinct(a):
    return len({a[f].tobytes() for f in range(len(a))}) == len(a)


# ---- spatial and level alignment: the reference through pinned chunk 0, the capture through chunk 1 -------------------
@pytest.mark.parametrize("bpc", [8, 10])
def test_shift_sse_four_chunks(bpc):
    ref, dis = SR.random_pair(70 + bpc, N, W, H, bpc)
    want = SR.shift_sse(ref, dis, 2)
    assert _distinct(want)
    rbuf, rv = _padded(ref)
    dbuf, dv = _padded(dis)
    with _engine(bpc=bpc) as eng:
        assert np.array_equal(eng.shift_sse(ref, dis, 2), want)
        assert np.array_equal(eng.shift_sse(rv, dv, 2), want)
        tr, rp, rrow, rframe = _on_device(rbuf, 1)
        td, dp, drow, dframe = _on_device(dbuf, 1)
        assert np.array_equal(eng.shift_sse_resident(rp, rrow, rframe, dp, drow, dframe, N, 2), want)


@pytest.mark.parametrize("bpc", [8, 10])
def test_level_stats_four_chunks(bpc):
    ref, dis = LR.random_pair(70 + bpc, N, W, H, bpc)
    want = LR.level_stats(ref, dis, bpc)
    assert _distinct(want)
    rbuf, rv = _padded(ref)
    dbuf, dv = _padded(dis)
    with _engine(bpc=bpc) as eng:
        assert np.array_equal(eng.level_stats(ref, dis), want)
        assert np.array_equal(eng.level_stats(rv, dv), want)
        tr, rp, rrow, rframe = _on_device(rbuf, 1)
        td, dp, drow, dframe = _on_device(dbuf, 1)
        assert np.array_equal(eng.level_stats_resident(rp, rrow, rframe, dp, drow, dframe, N), want)


def test_level_stats_chroma_plane_four_chunks():
    """plane 1 of a 4:2:0 context: 24 x 16 samples that travel through the staging at their own size"""
    ref, dis = LR.random_pair(81, N, W // 2, H // 2)
    want = LR.level_stats(ref, dis, 8)
    assert _distinct(want)
    rbuf, rv = _padded(ref, pad=3)
    dbuf, dv = _padded(dis, pad=3)
    with _engine(n_planes=3, chroma_shift=(1, 1)) as eng:
        assert eng.plane_shape(1) == (H // 2, W // 2)
        assert np.array_equal(eng.level_stats(ref, dis, 1), want)
        assert np.array_equal(eng.level_stats(rv, dv, 1), want)
        tr, rp, rrow, rframe = _on_device(rbuf, 1)
        td, dp, drow, dframe = _on_device(dbuf, 1)
        assert np.array_equal(eng.level_stats_resident(rp, rrow, rframe, dp, drow, dframe, N, 1), want)


# ---- luma statistics: one clip, its chunks alternate between the two pinned chunks --------------------------------------
def _luma_sums(frames, thr, gray):
    from tests.test_bookend import _cv2_style_gray
    c = np.stack([_cv2_style_gray(f, 8) if gray else f for f in frames]).astype(np.int64)
    return np.stack([c.sum((1, 2)), (c * c).sum((1, 2)), (c > thr).sum((1, 2))], 1).astype(np.uint64)


@pytest.mark.parametrize("gray", [False, True])
def test_luma_stats_four_chunks(gray):
    from pqa2_amd import _native as Nt
    frames = SR.random_pair(90, N, W, H)[0]
    want = _luma_sums(frames, 120, gray)
    assert _distinct(want)
    _, views = _padded(frames)
    with _engine() as eng:
        eng.set_luma_gray(Nt.GRAY_BT601_FULL if gray else Nt.GRAY_LUMA)
        assert np.array_equal(eng.luma_stats(frames, 120), want)
        assert np.array_equal(eng.luma_stats(views, 120), want)


def test_luma_stats_second_result_group():
    """2 053 frames in one call, 1 027 chunks: every launch writes its results behind the one before, they come back once,
    and the chunk parity carries on throughout.  Five distinct 16 x 16 arrays, over and over."""
    n = 2048 + 5
    base = SR.random_pair(91, 5, 16, 16)[0]
    order = [(3 * i + i // 5) % 5 for i in range(n)]
    sums = _luma_sums(base, 100, False)
    want = sums[order]
    assert _distinct(sums) and all(order[i] != order[i + 1] for i in range(n - 1))   # a result one frame off would show
    with _engine(16, 16) as eng:
        assert np.array_equal(eng.luma_stats([base[k] for k in order], 100), want)


# ---- temporal alignment: one ring slot per frame, and the ring wraps ---------------------------------------------------
K_LO, K_HI, N_REF, N_DIS = -3, 5, 40, 45    # two reference tiles, the second partial; a captured ring of 31 + 9 = 40 slots


def _cross_clip(bpc):
    ref, _ = SR.random_pair(100 + bpc, N_REF, W, H, bpc)
    dis, _ = SR.random_pair(200 + bpc, N_DIS, W, H, bpc)
    return ref, dis


def _cross_both_entries(bpc):
    """(host entry, resident entry) of the clip: with 2 frames a chunk, one of two captured frames straddles the wrap 39 -> 0"""
    ref, dis = _cross_clip(bpc)
    rbuf, _ = _padded(ref, pad=0, lead=0)
    dbuf, _ = _padded(dis, pad=0, lead=0)
    with _engine(bpc=bpc) as eng:
        host = eng.cross_sse(ref, dis, K_LO, K_HI)
        tr, rp, rrow, rframe = _on_device(rbuf, 0)
        td, dp, drow, dframe = _on_device(dbuf, 0)
        return host, eng.cross_sse_resident(rp, rrow, rframe, N_REF, dp, drow, dframe, N_DIS, K_LO, K_HI)


@pytest.mark.parametrize("bpc", [8, 10])
def test_cross_sse_ring_wrap(bpc):
    ref, dis = _cross_clip(bpc)
    want = AR.cross_sse(ref, dis, K_LO, K_HI)
    assert _distinct(want) and int(want[0, 0]) == int(AR.SENTINEL)
    host, resident = _cross_both_entries(bpc)
    assert np.array_equal(host, want) and np.array_equal(resident, want)


_CHILD = """
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
from tests.test_gpu_side_staging import _cross_both_entries
host, resident = _cross_both_entries(8)
np.savez(sys.argv[2], host=host, resident=resident)
"""


def test_cross_sse_ring_wrap_on_the_valu_path(tmp_path):
    """the same at 8 bit with PQA_XSSE_MFMA=0 (read at pqa_create): the host entry then skips its per-frame norm launches"""
    script, res = tmp_path / "child.py", tmp_path / "valu.npz"
    script.write_text(_CHILD)
    r = subprocess.run([sys.executable, str(script), ROOT, str(res)], env=dict(os.environ, PQA_XSSE_MFMA="0"),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    ref, dis = _cross_clip(8)
    want = AR.cross_sse(ref, dis, K_LO, K_HI)
    got = np.load(res)
    assert np.array_equal(got["host"], want) and np.array_equal(got["resident"], want)


# ---- refused calls leave the context usable --------------------------------------------------------------------------
def _ptrs(frames, hole=None):
    a = (C.c_void_p * len(frames))(*[f.ctypes.data for f in frames])
    if hole is not None:
        a[hole] = None
    return a


@pytest.mark.parametrize("entry", ["luma_stats", "cross_sse", "shift_sse", "level_stats"])
def test_refused_calls_leave_the_context_usable(entry):
    """a null frame pointer in the middle of the list and a stride one byte short: PQA_EINVAL before anything is queued
    (`out` keeps its fill), and the next valid call returns the right numbers"""
    from pqa2_amd import _native as Nt
    ref, dis = SR.random_pair(110, N, W, H)
    out = np.full(N * 3 * 256, 0xA5A5A5A5A5A5A5A5, np.uint64)    # the largest result of the four: level_stats
    with _engine() as eng:
        lib, ctx, o = eng.lib, eng._ctx, out.ctypes.data
        calls = {
            "luma_stats": lambda r, rs, d, ds: lib.pqa_luma_stats(ctx, r, rs, N, 120, o),
            "cross_sse": lambda r, rs, d, ds: lib.pqa_cross_sse(ctx, r, rs, N, d, ds, N, -1, 1, o),
            "shift_sse": lambda r, rs, d, ds: lib.pqa_shift_sse(ctx, r, rs, d, ds, N, 2, o),
            "level_stats": lambda r, rs, d, ds: lib.pqa_level_stats(ctx, r, rs, d, ds, N, 0, o),
        }
        call = calls[entry]
        bad = [(_ptrs(ref, hole=3), W, _ptrs(dis), W), (_ptrs(ref), W - 1, _ptrs(dis), W)]
        if entry != "luma_stats":    # the captured list has the same rules
            bad += [(_ptrs(ref), W, _ptrs(dis, hole=N - 2), W), (_ptrs(ref), W, _ptrs(dis), W - 1)]
        for args in bad:
            assert call(*args) == Nt.PQA_EINVAL
            assert lib.pqa_last_error(ctx)
            assert (out == 0xA5A5A5A5A5A5A5A5).all()
        assert call(_ptrs(ref), W, _ptrs(dis), W) == Nt.PQA_OK    # the raw call itself works
        want = {"luma_stats": lambda: _luma_sums(ref, 120, False), "cross_sse": lambda: AR.cross_sse(ref, dis, -1, 1),
                "shift_sse": lambda: SR.shift_sse(ref, dis, 2), "level_stats": lambda: LR.level_stats(ref, dis, 8)}[entry]()
        assert np.array_equal(out[:want.size].reshape(want.shape), want)
        got = {"luma_stats": lambda: eng.luma_stats(ref, 120), "cross_sse": lambda: eng.cross_sse(ref, dis, -1, 1),
               "shift_sse": lambda: eng.shift_sse(ref, dis, 2), "level_stats": lambda: eng.level_stats(ref, dis)}[entry]()
        assert np.array_equal(got, want)


def test_cross_sse_argument_rules_speak():
    """each rule of the two temporal entries names itself in pqa_last_error (with a null context none of them is reached:
    tests/test_align.py::test_argument_rules_need_no_device)"""
    from pqa2_amd import _native as Nt
    buf = np.zeros((4, 16, 16), np.uint8)
    ptrs = _ptrs(list(buf))
    out = np.zeros(1024, np.uint64)
    with _engine(16, 16) as eng:
        lib, ctx, p, o = eng.lib, eng._ctx, buf.ctypes.data, out.ctypes.data

        def dev(ref=p, n_ref=2, dis=p, n_dis=2, k_lo=-1, k_hi=1, o=o):
            return lib.pqa_cross_sse_device(ctx, ref, 16, 256, n_ref, dis, 16, 256, n_dis, k_lo, k_hi, o)

        def host(ref=ptrs, n_ref=2, dis=ptrs, n_dis=2, k_lo=-1, k_hi=1, o=o):
            return lib.pqa_cross_sse(ctx, ref, 16, n_ref, dis, 16, n_dis, k_lo, k_hi, o)
        for call in (dev, host):
            for kw, word in ((dict(ref=None), b"null"), (dict(dis=None), b"null"), (dict(o=None), b"null"),
                             (dict(n_ref=-1), b"negative"), (dict(n_dis=-1), b"negative"), (dict(k_lo=2, k_hi=1), b"k_lo"),
                             (dict(k_lo=-65, k_hi=0), b"outside"), (dict(k_lo=0, k_hi=65), b"outside"),
                             (dict(k_lo=-100, k_hi=100), b"outside")):
                assert call(**kw) == Nt.PQA_EINVAL, kw
                assert word in lib.pqa_last_error(ctx) and lib.pqa_last_error(ctx).startswith(b"cross_sse: "), kw
        assert host() == Nt.PQA_OK and out[:6].tolist() == [2 ** 64 - 1, 0, 0, 0, 0, 2 ** 64 - 1]


# ---- what the older entries have always answered ------------------------------------------------------------------------
FILL = 0xA5A5A5A5A5A5A5A5


def _bottom_up(frames):
    """(pointer list, stride) that name each frame by its last row, rows a negative stride apart: read top-down from
    there, a frame is its vertically flipped copy"""
    a = [np.ascontiguousarray(f) for f in frames]
    ptrs = (C.c_void_p * len(a))(*[f.ctypes.data + (f.shape[0] - 1) * f.strides[0] for f in a])
    return a, ptrs, -a[0].strides[0]


@pytest.mark.parametrize("bpc", [8, 10])
def test_bottom_up_frames_pass_where_they_always_did(bpc):
    """pqa_luma_stats, pqa_shift_sse and pqa_cross_sse let a negative stride pass and copy the rows bottom-up: they return
    the integers of the flipped frames"""
    from pqa2_amd import _native as Nt
    ref, dis = SR.random_pair(120 + bpc, N, W, H, bpc)
    thr = 120 << (bpc - 8)
    flip = lambda fs: [f[::-1] for f in fs]
    xr, xd = _cross_clip(bpc)
    with _engine(bpc=bpc) as eng:
        lib, ctx = eng.lib, eng._ctx
        kr, rp, rs = _bottom_up(ref)
        kd, dp, ds = _bottom_up(dis)
        assert rs == -W * ref[0].itemsize
        out = np.full((N, 3), FILL, np.uint64)
        assert lib.pqa_luma_stats(ctx, rp, rs, N, thr, out.ctypes.data) == Nt.PQA_OK
        want = _luma_sums(flip(ref), thr, False)
        assert _distinct(want) and np.array_equal(out, want)
        out = np.full((N, 5, 5), FILL, np.uint64)
        assert lib.pqa_shift_sse(ctx, rp, rs, dp, ds, N, 2, out.ctypes.data) == Nt.PQA_OK
        want = SR.shift_sse(flip(ref), flip(dis), 2)
        assert not np.array_equal(want, SR.shift_sse(ref, dis, 2)) and np.array_equal(out, want)
        kxr, xrp, xrs = _bottom_up(xr)
        kxd, xdp, xds = _bottom_up(xd)
        out = np.full((N_REF, K_HI - K_LO + 1), FILL, np.uint64)
        assert lib.pqa_cross_sse(ctx, xrp, xrs, N_REF, xdp, xds, N_DIS, K_LO, K_HI, out.ctypes.data) == Nt.PQA_OK
        assert np.array_equal(out, AR.cross_sse(flip(xr), flip(xd), K_LO, K_HI))
        # one clip top-down, the other bottom-up: the strides are each clip's own
        top = _ptrs([np.ascontiguousarray(f) for f in ref])
        out = np.full((N, 5, 5), FILL, np.uint64)
        assert lib.pqa_shift_sse(ctx, top, W * ref[0].itemsize, dp, ds, N, 2, out.ctypes.data) == Nt.PQA_OK
        assert np.array_equal(out, SR.shift_sse(ref, flip(dis), 2))


def _sad_call(eng, anchor, frames, n_planes):
    """(return code, out) of pqa_frame_sad on planes as they lie (views keep their strides): a frame of the list is three
    pointers whatever n_planes is, the ones the context has no plane for null"""
    P, S = C.c_void_p * 3, C.c_int64 * 3
    ap, as_, st = P(), S(), S()
    ptrs = (C.c_void_p * (3 * len(frames)))()
    for p in range(n_planes):
        ap[p], as_[p], st[p] = anchor[p].ctypes.data, anchor[p].strides[0], frames[0][p].strides[0]
        for f, planes in enumerate(frames):
            assert planes[p].strides[0] == st[p]
            ptrs[3 * f + p] = planes[p].ctypes.data
    out = np.full((len(frames), 3), FILL, np.uint64)
    return eng.lib.pqa_frame_sad(eng._ctx, C.byref(ap), C.byref(as_), ptrs, C.byref(st), len(frames), out.ctypes.data), out


def _sads(anchor, frames, n_planes):
    out = np.zeros((len(frames), 3), np.uint64)
    for f, planes in enumerate(frames):
        for p in range(n_planes):
            out[f, p] = np.abs(planes[p].astype(np.int64) - anchor[p].astype(np.int64)).sum()
    return out


@pytest.mark.parametrize("bpc", [8, 10])
def test_bottom_up_frames_are_refused_where_they_always_were(bpc):
    """pqa_level_stats and pqa_frame_sad answer a negative stride with PQA_EINVAL before anything is queued: `out` keeps its
    fill, and the next valid call is right"""
    from pqa2_amd import _native as Nt
    ref, dis = LR.random_pair(130 + bpc, N, W, H, bpc)
    with _engine(bpc=bpc, features=Nt.FEAT_PSNR | Nt.FEAT_INTEGRITY) as eng:
        lib, ctx = eng.lib, eng._ctx
        kr, rp, rs = _bottom_up(ref)
        kd, dp, ds = _bottom_up(dis)
        top_r, top_d, stride = _ptrs(kr), _ptrs(kd), W * ref[0].itemsize
        out = np.full((N, 1 << bpc, 3), FILL, np.uint64)
        for args in ((rp, rs, top_d, stride), (top_r, stride, dp, ds)):
            assert lib.pqa_level_stats(ctx, *args, N, 0, out.ctypes.data) == Nt.PQA_EINVAL
            assert lib.pqa_last_error(ctx).startswith(b"level_stats: ") and b"stride smaller than a row" in lib.pqa_last_error(ctx)
            assert (out == FILL).all()
        assert lib.pqa_level_stats(ctx, top_r, stride, top_d, stride, N, 0, out.ctypes.data) == Nt.PQA_OK
        assert np.array_equal(out, LR.level_stats(ref, dis, bpc))
        # pqa_frame_sad: the frames bottom-up (the views' own negative strides)
        anchor, frames = [kd[0]], [[f] for f in kr]
        rc, out = _sad_call(eng, anchor, [[f[0][::-1]] for f in frames], 1)
        assert rc == Nt.PQA_EINVAL and lib.pqa_last_error(ctx) == b"plane 0 stride smaller than a row" and (out == FILL).all()
        rc, out = _sad_call(eng, anchor, frames, 1)
        want = _sads(anchor, frames, 1)
        assert rc == Nt.PQA_OK and _distinct(want) and np.array_equal(out, want)


def test_no_frames_pass_before_a_pitch_is_looked_at():
    """pqa_shift_sse_device and pqa_level_stats_device with zero frames and a row pitch one byte short of a row: PQA_OK"""
    from pqa2_amd import _native as Nt
    buf = np.zeros((1, H, W), np.uint8)
    with _engine() as eng:
        t, p, row, frame = _on_device(buf, 0)
        assert eng.lib.pqa_shift_sse_device(eng._ctx, p, W - 1, frame, p, W - 1, frame, 0, 2, None) == Nt.PQA_OK
        assert eng.lib.pqa_level_stats_device(eng._ctx, p, W - 1, frame, p, W - 1, frame, 0, 0, None) == Nt.PQA_OK
        assert eng.lib.pqa_shift_sse_device(eng._ctx, p, W - 1, frame, p, W - 1, frame, 1, 2, np.zeros(25, np.uint64).ctypes.data) == Nt.PQA_EINVAL


def test_luma_stats_device_has_no_rule_on_the_row_pitch():
    """rows W / 2 bytes apart overlap: pqa_luma_stats_device sums them as they lie, three frames"""
    rng = np.random.default_rng(140)
    pitch, n = W // 2, 3
    frame = (H - 1) * pitch + W + 8          # a frame's last row ends inside it
    buf = rng.integers(0, 256, n * frame, dtype=np.uint8)
    views = np.lib.stride_tricks.as_strided(buf, (n, H, W), (frame, pitch, 1), writeable=False)
    want = _luma_sums(list(views), 120, False)
    assert _distinct(want)
    with _engine() as eng:
        import torch
        t = torch.from_numpy(buf).cuda()
        torch.cuda.synchronize()
        assert np.array_equal(eng.luma_stats_resident(t.data_ptr(), pitch, frame, n, 120), want)


@pytest.mark.parametrize("n_planes", [3, 1])
def test_frame_sad_views_four_chunks(n_planes):
    """7 frames of a 4:2:0 context as views into padded buffers against an anchor with another pad: the numpy SADs, and what
    pqa_frame_sad_device returns on the same bytes; on a one-plane context the list still holds three pointers a frame"""
    from pqa2_amd import _native as Nt
    rng = np.random.default_rng(150 + n_planes)
    shapes = [(H, W), (H // 2, W // 2), (H // 2, W // 2)][:n_planes]
    planes = [[rng.integers(0, 256, s, dtype=np.uint8) for _ in range(N + 1)] for s in shapes]    # [plane][frame]; the last is the anchor
    bufs, views, abufs, anchor = [], [], [], []
    for p, pad in zip(range(n_planes), (5, 3, 3)):
        b, v = _padded(planes[p][:N], pad=pad)
        ab, av = _padded(planes[p][N:], pad=pad + 4, lead=2)
        bufs.append(b), views.append(v), abufs.append(ab), anchor.append(av[0])
    frames = [[views[p][f] for p in range(n_planes)] for f in range(N)]
    want = _sads(anchor, frames, n_planes)
    assert _distinct(want) and (want[:, :n_planes] > 0).all() and (want[:, n_planes:] == 0).all()
    kw = dict(n_planes=3, chroma_shift=(1, 1)) if n_planes == 3 else {}
    with _engine(features=Nt.FEAT_PSNR | Nt.FEAT_INTEGRITY, **kw) as eng:
        rc, out = _sad_call(eng, anchor, frames, n_planes)
        assert rc == Nt.PQA_OK and np.array_equal(out, want)
        dev = [_on_device(b, 1) for b in bufs]
        adev = [_on_device(b, 2) for b in abufs]
        got = eng.frame_sad_resident([a[1] for a in adev], [a[2] for a in adev], [d[1] for d in dev], [d[2] for d in dev],
                                     [d[3] for d in dev], N)
        assert np.array_equal(got, want)


# ---- the staging of the plane transforms and of the analyses of planes of the call's own size ---------------------------
N9 = 9    # two chunks of the host entries (8 frames a chunk), the second partial


@pytest.mark.parametrize("fmt,lay,bits", [("bgra", "420left", 8), ("r210", "422", 10)])
def test_rgb_convert_across_the_chunk(fmt, lay, bits):
    """9 different host frames of 17 x 5: the ninth travels in a second chunk, through pinned and device buffers the first
    chunk has used, and lands behind the eighth in the caller's planes -- three planes and luma only"""
    from tests import rgb_ref as R
    from tests import test_gpu_rgb as TR
    w, h = 17, 5
    dst, m = (*TR.LAYOUTS[lay], bits), TR._matrix("bt709", fmt, bits)
    frames = TR._frames(300 + bits, fmt, w, h, n=N9, stride=R.file_stride(fmt, w))
    assert _distinct(np.stack(frames))
    want = [R.convert(fr, fmt, w, h, m, dst) for fr in frames]
    with TR._engine() as eng:
        TR._same(eng.rgb_convert(frames, fmt, (h, w), dst, m), want, (fmt, lay, "three planes"))
        TR._same(eng.rgb_convert(frames, fmt, (h, w), dst, m, luma_only=True), [[p[0]] for p in want], (fmt, lay, "luma only"))


def _interleaved_calls():
    """(name, call on an engine) in the order of the test below; every call has 9 frames, of its own size or of the context's"""
    from tests import format_convert_ref as FR
    rng = np.random.default_rng(77)
    u8 = lambda h, w: [rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(N9)]
    small, lut, blend, fill = u8(9, 33), rng.permutation(256).astype(np.uint8), u8(9, 33), u8(9, 33)
    nodes = rng.integers(0, 257, (4, 10)).astype(np.uint16)    # steps of 4 samples over 33 x 9
    table_in, packed, chroma = u8(16, 16), u8(6, 68), u8(12, 17)    # UYVY rows of 34 pixels; the 4:2:2 chroma plane of 34 x 12
    ref3 = [[a, b, c] for a, b, c in zip(u8(H, W), u8(H // 2, W // 2), u8(H // 2, W // 2))]
    dis3 = [[a, b, c] for a, b, c in zip(u8(H, W), u8(H // 2, W // 2), u8(H // 2, W // 2))]
    matrix = [3 << 14, 15000, -700, 900, 2 << 14, 300, 16000, -500, 1 << 14, -400, 600, 17000]
    resample = ("resample", lambda e: e.resample(small, (32, 64)))
    ref_y, dis_y, ref_u, dis_u = [f[0] for f in ref3], [f[0] for f in dis3], [f[1] for f in ref3], [f[1] for f in dis3]
    return [resample,
            ("shift_sse", lambda e: e.shift_sse(ref_y, dis_y, 2)),
            ("table_apply", lambda e: e.table_apply(table_in, lut, plane=None)),
            ("level_stats", lambda e: e.level_stats(ref_y, dis_y)),
            ("mask_blend", lambda e: e.mask_blend(blend, nodes, (2, 2), fill, plane=None)),
            ("level_stats chroma", lambda e: e.level_stats(ref_u, dis_u, 1)),
            ("unpack", lambda e: e.unpack(packed, "uyvy422", (6, 34))),
            ("luma_stats", lambda e: e.luma_stats(dis_y, 120)),
            ("format_convert", lambda e: e.format_convert(chroma, (12, 34), (1, 0, FR.COSITED, 0, 8), (1, 1, FR.COSITED, FR.CENTRE, 8))),
            ("colour_moments", lambda e: e.colour_moments(ref3, dis3)),
            ("cross_sse", lambda e: e.cross_sse(ref_y, dis_y, -1, 1)),
            ("colour_apply", lambda e: e.colour_apply(dis3, matrix)),
            ("frame_sad", lambda e: e.frame_sad(ref3[0], dis3)),
            ("tile_moments", lambda e: e.tile_moments(ref_y, dis_y)),
            ("line_profiles", lambda e: e.line_profiles(dis_y)),
            ("resample again", resample[1])]


def _flat(result):
    """the arrays of a result, whatever its nesting"""
    if isinstance(result, np.ndarray):
        return [result]
    return [a for part in result for a in _flat(part)]


def test_entries_interleaved_on_one_context():
    """the entries that stage host frames, of their own size or of the context's, one after the other on one context, each with
    two chunks or more: every call both grows and under-fills the pinned chunks and staging buffers the call before it left,
    and returns what it returns on a fresh context"""
    from pqa2_amd import _native as Nt
    calls = _interleaved_calls()
    kw = dict(n_planes=3, chroma_shift=(1, 1), features=Nt.FEAT_PSNR | Nt.FEAT_INTEGRITY)
    with _engine(**kw) as eng:
        got = [_flat(call(eng)) for _, call in calls]
    for (name, call), mine in zip(calls, got):
        with _engine(**kw) as fresh:
            want = _flat(call(fresh))
        assert len(mine) == len(want) and len(want) >= 1, name
        for k, (a, b) in enumerate(zip(mine, want)):
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (name, k)
    assert _distinct(np.stack(got[0])) and _distinct(np.stack(got[1]))    # the frames of a call differ: one in the wrong slot shows
