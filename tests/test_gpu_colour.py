"""Colour-matrix alignment on the MI355X (csrc/colour_moments.hip; pqa_colour_moments / pqa_colour_apply and their _device
forms): the 28 sums and the applied planes equal the numpy restatement (tests/colour_ref.py) as integers -- 8 / 10 / 12 bit,
4:2:0 / 4:2:2 / 4:4:4 / 4:4:0, a frame smaller than any context takes (8 x 2, through pqa_debug_colour), padded rows on an unaligned
base, odd sizes with partial edge blocks, and 1100 x 150, which spans several workgroup tiles (256 x 32 chroma samples for
the moments, 256 x 16 for the apply) both ways with a partial last one; both masks, a frame masked whole, more pairs than a
chunk, full-scale frames against the closed form; the argument rules; the calls leave the scoring chain alone; and a
bt709 -> bt601 Y4M pair through score_files(colour_align=) gives the records of the capture corrected by hand."""
import ctypes as C
import json

import numpy as np
import pytest

from tests import colour_ref as R

pytestmark = pytest.mark.gpu

SHIFTS = {"420": (1, 1), "422": (1, 0), "444": (0, 0), "440": (0, 1)}
IDENT = [0, 16384, 0, 0, 0, 0, 16384, 0, 0, 0, 0, 16384]


def _engine(w, h, bd=8, ss="420", **kw):
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    return FeatureEngine(w, h, bit_depth=bd, n_planes=kw.pop("n_planes", 3), chroma_shift=SHIFTS[ss],
                         features=kw.pop("features", N.FEAT_PSNR), **kw)


def _negative(bd):
    f = 1 << (bd - 8)
    return [2000 * f, 14000, -3000, 2500, -50000 * f, -1500, 17000, -2200, 90000 * f, 1200, -2600, 15000]


def _both_clamps(bd):
    """gains of 3.5 about the middle: the low third of every plane lands below 0, the high third above top"""
    top = (1 << bd) - 1
    off = -int(1.25 * top * 16384)
    return [off, 57344, 0, 0, off, 0, 57344, 0, off, 0, 0, 57344]


def _same(got, want):
    return all(np.array_equal(g[p], w[p]) for g, w in zip(got, want) for p in range(3))


def _debug(bd, hs, vs, w, h, ref, dis, lo, hi, m=None):
    """pqa_debug_colour on one frame pair -> (sums, applied planes or None)"""
    from pqa2_amd import _native as N
    lib = N.load()
    P = C.c_void_p * 3
    ref = [np.ascontiguousarray(p) for p in ref]
    dis = [np.ascontiguousarray(p) for p in dis]
    out = np.zeros(28, np.uint64)
    res = [np.zeros_like(p) for p in dis] if m is not None else None
    mm = (C.c_int32 * 12)(*m) if m is not None else None
    rc = lib.pqa_debug_colour(bd, hs, vs, w, h, C.byref(P(*[p.ctypes.data for p in ref])), C.byref(P(*[p.ctypes.data for p in dis])),
                              lo, hi, out.ctypes.data, C.byref(mm) if m is not None else None,
                              C.byref(P(*[p.ctypes.data for p in res])) if m is not None else None)
    assert rc == N.PQA_OK, lib.pqa_last_error(None)
    return out, res


def _resident(eng, ref, dis, m, pad=5, lead=3):
    """frames as device clips with rows `pad` samples longer than a row and a base `lead` samples in (not 16-byte aligned):
    (sums under the default mask, sums under the keep-all mask, dis applied through m)"""
    import torch
    n, es = len(ref), ref[0][0].dtype.itemsize
    top = (1 << eng.bit_depth) - 1
    bufs, ptrs, outs = [], [[], [], []], []
    pitches = ([], [])
    for p in range(3):
        h, w = ref[0][p].shape
        for k, clip in enumerate((ref, dis, None)):
            buf = np.zeros((n, h, w + pad), ref[0][0].dtype)
            if clip is not None:
                buf[:, :, lead:lead + w] = np.stack([f[p] for f in clip])
            t = torch.from_numpy(buf.view(np.uint8).reshape(-1)).cuda()
            bufs.append(t)
            ptrs[k].append(t.data_ptr() + lead * es)
            if k == 2:
                outs.append((t, buf.shape, w))
        pitches[0].append((w + pad) * es)
        pitches[1].append(h * (w + pad) * es)
    torch.cuda.synchronize()
    g_default = eng.colour_moments_resident(ptrs[0], ptrs[1], pitches[0], pitches[1], n)
    g_all = eng.colour_moments_resident(ptrs[0], ptrs[1], pitches[0], pitches[1], n, 0, top)
    eng.colour_apply_resident(m, ptrs[1], ptrs[2], pitches[0], pitches[1], n)
    planes = []
    for t, shape, w in outs:
        back = t.cpu().numpy().view(ref[0][0].dtype).reshape(shape)
        assert not back[:, :, :lead].any() and not back[:, :, lead + w:].any()      # nothing written outside the rows
        planes.append(back[:, :, lead:lead + w])
    return g_default, g_all, [[planes[p][f] for p in range(3)] for f in range(n)]


@pytest.mark.parametrize("ss", ["420", "422", "444", "440"])
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_sums_and_planes_equal_the_restatement(bd, ss):
    from pqa2_amd import align as AL
    hs, vs = SHIFTS[ss]
    top = (1 << bd) - 1
    neg, clamp = _negative(bd), _both_clamps(bd)
    fix = [int(v) for v in AL.colour_correction({"kind": "bt709_to_bt601"}, bd)]      # the Q14 inverse of the CPU recovery case

    # 8 x 2: smaller than any context accepts
    (r,), (d,) = R.noise_frames(100 + bd, 8, 2, bd, hs, vs), R.noise_frames(200 + bd, 8, 2, bd, hs, vs)
    for lo, hi in ((1, top - 1), (0, top)):
        got, planes = _debug(bd, hs, vs, 8, 2, r, d, lo, hi, neg)
        assert np.array_equal(got, R.colour_moments([r], [d], bd, hs, vs, lo, hi)[0])
        assert _same([planes], [R.apply(d, neg, bd, hs, vs)])

    # 66 x 34, rows longer than a row, base not 16-byte aligned: the per-sample path of every lane
    ref, dis = R.noise_frames(300 + bd, 66, 34, bd, hs, vs, 2), R.noise_frames(400 + bd, 66, 34, bd, hs, vs, 2)
    with _engine(66, 34, bd, ss) as eng:
        g_default, g_all, planes = _resident(eng, ref, dis, clamp)
        assert np.array_equal(g_default, R.colour_moments(ref, dis, bd, hs, vs))
        assert np.array_equal(g_all, R.colour_moments(ref, dis, bd, hs, vs, 0, top))
        want = [R.apply(f, clamp, bd, hs, vs) for f in dis]
        assert _same(planes, want)
        assert all((w[p] == 0).any() and (w[p] == top).any() for w in want for p in range(3))      # both clamps were reached
        assert np.array_equal(eng.colour_moments(ref, dis), g_default)                                # the host entry, wide loads

    # 131 x 77: odd both ways, partial edge blocks
    ref, dis = R.noise_frames(500 + bd, 131, 77, bd, hs, vs, 2), R.noise_frames(600 + bd, 131, 77, bd, hs, vs, 2)
    with _engine(131, 77, bd, ss) as eng:
        assert np.array_equal(eng.colour_moments(ref, dis), R.colour_moments(ref, dis, bd, hs, vs))
        assert np.array_equal(eng.colour_moments(ref, dis, 0, top), R.colour_moments(ref, dis, bd, hs, vs, 0, top))
        assert _same(eng.colour_apply(dis, IDENT), dis)                                               # bit for bit
        assert _same(eng.colour_apply(dis, neg), [R.apply(f, neg, bd, hs, vs) for f in dis])
        assert _same(eng.colour_apply(dis, fix), [R.apply(f, fix, bd, hs, vs) for f in dis])

    # 1100 x 150: several workgroup tiles both ways, the last one partial
    ref, dis = R.noise_frames(700 + bd, 1100, 150, bd, hs, vs, 1), R.noise_frames(800 + bd, 1100, 150, bd, hs, vs, 1)
    with _engine(1100, 150, bd, ss) as eng:
        assert np.array_equal(eng.colour_moments(ref, dis), R.colour_moments(ref, dis, bd, hs, vs))
        assert np.array_equal(eng.colour_moments(ref, dis, 0, top), R.colour_moments(ref, dis, bd, hs, vs, 0, top))
        assert _same(eng.colour_apply(dis, fix), [R.apply(f, fix, bd, hs, vs) for f in dis])
        assert _same(eng.colour_apply(dis, clamp), [R.apply(f, clamp, bd, hs, vs) for f in dis])


def test_a_frame_masked_whole_and_more_pairs_than_a_chunk():
    """9 pairs cross the chunk of 8; pair 4's captured frame is all zeros (every sample masked: entry 0 = 0, all sums 0); the
    host entry equals the device entry"""
    ref, dis = R.noise_frames(1, 66, 34, 8, 1, 1, 9), R.noise_frames(2, 66, 34, 8, 1, 1, 9)
    dis[4] = [np.zeros_like(p) for p in dis[4]]
    want = R.colour_moments(ref, dis, 8, 1, 1)
    assert not want[4].any() and want[3, 0] > 0
    with _engine(66, 34) as eng:
        host = eng.colour_moments(ref, dis)
        assert host.dtype == np.uint64 and host.shape == (9, 28) and np.array_equal(host, want)
        g_default, g_all, planes = _resident(eng, ref, dis, _negative(8), pad=14, lead=0)      # 16-byte aligned rows: the wide loads
        assert np.array_equal(g_default, host) and np.array_equal(g_all, R.colour_moments(ref, dis, 8, 1, 1, 0, 255))
        assert _same(planes, [R.apply(f, _negative(8), 8, 1, 1) for f in dis])
        assert _same(eng.colour_apply(dis, _negative(8)), planes)


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_full_scale_frames_against_the_closed_form(bd):
    """1024 x 512 at 4:2:0, every sample 2^bd - 1: each of the 131 072 chroma samples adds (4 top)^2 to the largest entry -- at
    12 bit a lane's 32-bit partial holds eight of them"""
    top, n = (1 << bd) - 1, 512 * 256
    frame = [np.full((512, 1024), top, R.dtype_of(bd)), np.full((256, 512), top, R.dtype_of(bd)), np.full((256, 512), top, R.dtype_of(bd))]
    z = [1, 4 * top, top, top, 4 * top, top, top]
    want = np.array([n * z[i] * z[j] for i in range(7) for j in range(i, 7)], np.uint64)
    with _engine(1024, 512, bd) as eng:
        got = eng.colour_moments([frame, frame], [frame, frame], 0, top)
        assert np.array_equal(got[0], want) and np.array_equal(got[1], want)
        assert not eng.colour_moments([frame], [frame]).any()      # default mask: top is a clipped sample
    if bd == 12:
        assert int(want[7]) == n * 16380 * 16380 > 1 << 44


def test_argument_rules():
    from pqa2_amd import _native as N
    ref, dis = R.noise_frames(5, 32, 16, 8, 1, 1, 1), R.noise_frames(6, 32, 16, 8, 1, 1, 1)
    with _engine(32, 16) as eng:
        lib, ctx = eng.lib, eng._ctx
        want = R.colour_moments(ref, dis, 8, 1, 1)
        assert eng.lib.pqa_colour_sums() == 28
        assert eng.colour_moments([], []).shape == (0, 28) and eng.colour_apply([], IDENT) == []
        keep_r, rp, rs = eng._frame_list(ref, "reference")
        keep_d, dp, ds = eng._frame_list(dis, "captured")
        out = np.zeros(28, np.uint64)
        m = (C.c_int32 * 12)(*IDENT)
        ok = lambda: lib.pqa_colour_moments(ctx, rp, C.byref(rs), dp, C.byref(ds), 1, 1, 254, out.ctypes.data)
        assert ok() == N.PQA_OK and np.array_equal(out, want[0])
        short = (C.c_int64 * 3)(31, 16, 16)
        empty = (C.c_void_p * 3)()
        for rc in (lib.pqa_colour_moments(ctx, None, C.byref(rs), dp, C.byref(ds), 1, 1, 254, out.ctypes.data),
                   lib.pqa_colour_moments(ctx, rp, C.byref(rs), dp, C.byref(ds), 1, 1, 254, None),
                   lib.pqa_colour_moments(ctx, rp, C.byref(rs), empty, C.byref(ds), 1, 1, 254, out.ctypes.data),      # null plane
                   lib.pqa_colour_moments(ctx, rp, C.byref(short), dp, C.byref(ds), 1, 1, 254, out.ctypes.data),      # stride < row
                   lib.pqa_colour_moments(ctx, rp, C.byref(rs), dp, C.byref(ds), -1, 1, 254, out.ctypes.data),
                   lib.pqa_colour_moments(ctx, rp, C.byref(rs), dp, C.byref(ds), 1, 9, 8, out.ctypes.data),           # lo > hi
                   lib.pqa_colour_moments(ctx, rp, C.byref(rs), dp, C.byref(ds), 1, 0, 256, out.ctypes.data),         # hi > top
                   lib.pqa_colour_moments_device(ctx, None, None, 1, 1, 254, out.ctypes.data),
                   lib.pqa_colour_moments_device(ctx, C.byref(N.PqaDeviceClip()), C.byref(N.PqaDeviceClip()), 1, 1, 254, out.ctypes.data),
                   lib.pqa_colour_apply(ctx, None, dp, C.byref(ds), dp, C.byref(ds), 1),
                   lib.pqa_colour_apply(ctx, C.byref(m), dp, C.byref(ds), None, C.byref(ds), 1),
                   lib.pqa_colour_apply(ctx, C.byref(m), dp, C.byref(ds), dp, C.byref(ds), -1),
                   lib.pqa_colour_apply_device(ctx, C.byref(m), None, None, 1)):
            assert rc == N.PQA_EINVAL
        for i, v in ((1, 65536), (6, -65536), (0, 1 << 28), (8, -(1 << 28))):      # an entry on the edge of its range
            bad = (C.c_int32 * 12)(*IDENT)
            bad[i] = v
            assert lib.pqa_colour_apply(ctx, C.byref(bad), dp, C.byref(ds), dp, C.byref(ds), 1) == N.PQA_EINVAL
            assert lib.pqa_colour_apply_device(ctx, C.byref(bad), None, None, 0) == N.PQA_EINVAL
        assert lib.pqa_colour_moments(ctx, None, None, None, None, 0, 1, 254, None) == N.PQA_OK      # n_frames == 0 writes nothing
        assert lib.pqa_colour_apply_device(ctx, C.byref(m), None, None, 0) == N.PQA_OK
        with pytest.raises(ValueError):
            eng.colour_moments(ref, dis[:0])
        with pytest.raises(ValueError):
            eng.colour_moments([[ref[0][0], ref[0][0], ref[0][2]]], dis)      # a luma-sized plane where chroma belongs
        assert ok() == N.PQA_OK and np.array_equal(out, want[0])             # refused calls leave the context usable
        del keep_r, keep_d
    with _engine(32, 16, n_planes=1) as eng:
        out = np.zeros(28, np.uint64)
        assert eng.lib.pqa_colour_moments(eng._ctx, None, None, None, None, 0, 1, 254, out.ctypes.data) == N.PQA_EINVAL
        assert b"n_planes" in eng.lib.pqa_last_error(eng._ctx)
        with pytest.raises(N.PqaError):
            eng.colour_moments(ref, dis)


def test_independent_of_the_scoring_chain():
    from pqa2_amd import _native as N
    ref, dis = R.clip(7, 64, 48, 8, 1, 1, 6), R.clip(8, 64, 48, 8, 1, 1, 6)

    def run(with_call):
        with _engine(64, 48, features=N.FEAT_VMAF | N.FEAT_PSNR | N.FEAT_SSIM, max_batch=4) as eng:
            sums = []
            for i in range(6):
                eng.submit(i, ref[i], dis[i])
                if with_call and i in (0, 2, 4):      # inside a pending batch, and right after one was launched
                    sums.append(eng.colour_moments(ref, dis))
                    eng.colour_apply(dis[:2], _negative(8))
            return eng.collect(0, 6), sums
    plain, _ = run(False)
    mixed, sums = run(True)
    assert np.array_equal(plain.view(np.uint64), mixed.view(np.uint64))
    want = R.colour_moments(ref, dis, 8, 1, 1)
    assert len(sums) == 3 and all(np.array_equal(s, want) for s in sums)


# ---- end to end -----------------------------------------------------------------------------------------------------------
W, H, N_FRAMES = 96, 64, 6


def _write_pairs(tmp_path):
    """a limited-range 4:2:0 reference, its capture through bt709_to_bt601 (rounded), and the capture corrected by hand with
    the restated apply and the matrix the solver gives"""
    from pqa2_amd import align as AL
    from pqa2_amd.yuvio import VideoInfo, write_y4m
    info = VideoInfo(width=W, height=H, fps_num=24, fps_den=1, bit_depth=8, mono=False, hshift=1, vshift=1, chroma_tag="420")
    ref = R.clip(41, W, H, 8, 1, 1, N_FRAMES)
    cap = [R.convert(f, *AL.named_colour_map("bt709_to_bt601", 8), 8, 1, 1) for f in ref]
    m = AL.colour_correction({"kind": "bt709_to_bt601"}, 8)
    back = [R.apply(f, m, 8, 1, 1) for f in cap]
    paths = {}
    for key, clip in (("ref", ref), ("dis", cap), ("dis_back", back)):
        paths[key] = str(tmp_path / (key + ".y4m"))
        write_y4m(paths[key], clip, info)
    return paths, [int(v) for v in m]


def test_end_to_end_report_and_apply(tmp_path):
    from pqa2_amd.pipeline import score_files
    p, m = _write_pairs(tmp_path)
    plain = score_files(p["ref"], p["dis"], "vmaf_v0.6.1")
    rep = score_files(p["ref"], p["dis"], "vmaf_v0.6.1", colour_align="report")
    col = rep["alignment"]["colour"]
    assert (col["kind"], col["mismatch"], col["cross_plane"], col["applied"], col["frames"], col["degenerate"]) == \
        ("bt709_to_bt601", True, True, False, N_FRAMES, False)
    assert col["correction"] == m
    assert "alignment" not in plain and np.array_equal(rep["records"].view(np.uint64), plain["records"].view(np.uint64))
    done = score_files(p["ref"], p["dis"], "vmaf_v0.6.1", colour_align="apply")
    assert done["alignment"]["colour"]["applied"] is True
    by_hand = score_files(p["ref"], p["dis_back"], "vmaf_v0.6.1")
    assert done["records"].shape == by_hand["records"].shape == (N_FRAMES, 24)
    assert np.array_equal(done["records"].view(np.uint64), by_hand["records"].view(np.uint64))
    assert not np.array_equal(done["records"].view(np.uint64), plain["records"].view(np.uint64))
    for k in done["metrics"]:
        assert np.array_equal(np.asarray(done["metrics"][k]), np.asarray(by_hand["metrics"][k])), k
    same = score_files(p["ref"], p["ref"], "vmaf_v0.6.1", colour_align="apply")
    assert (same["alignment"]["colour"]["kind"], same["alignment"]["colour"]["applied"]) == ("identity", False)


def test_analyzer_corrects_and_writes_the_colour_object(tmp_path):
    from pqa2_amd.vmaf_analyzer import VMAFAnalyzer
    p, m = _write_pairs(tmp_path)
    an = VMAFAnalyzer()
    an.set_output_directory(str(tmp_path))
    an.set_test_name("colour")
    an.set_advanced_options(colour_correct_enabled=True)
    lines = []
    an.status_update.connect(lines.append)
    results = an.analyze_videos(p["ref"], p["dis"])
    assert results and results["alignment"]["colour"]["kind"] == "bt709_to_bt601"
    col = json.load(open(results["json_path"]))["alignment"]["colour"]
    assert col["applied"] is True and col["mismatch"] is True and col["frames"] == N_FRAMES and col["correction"] == m
    assert any("decoded as bt709 and encoded as bt601" in s and s.endswith(", corrected") for s in lines)
