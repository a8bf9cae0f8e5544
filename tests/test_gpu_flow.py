"""Sub-pixel and scale registration on the MI355X (csrc/flow_moments.hip, pqa_flow_moments / pqa_flow_moments_device): the
tile moments equal the numpy restatement (tests/flow_ref.py) as integers -- smallest call, argument rules, row tails / pitches
/ odd base addresses at 8 / 10 / 12 bit, last tiles one counted pixel wide and high, the accumulator limits at the sample
extremes; the calls leave the scoring chain alone; align.register driven by the engine walks the same integers as when driven
by the restatements; and warped Y4M pairs through score_files(register=) and VMAFAnalyzer give the records of the clips
registered and cropped by hand."""
import ctypes as C
import json

import numpy as np
import pytest

from tests import flow_ref as F
from tests import resample_ref as R
from tests import spatial_align_ref as S

pytestmark = pytest.mark.gpu


def _engine(w=64, h=48, bpc=8, **kw):
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    return FeatureEngine(w, h, bit_depth=bpc, n_planes=1, features=kw.pop("features", N.FEAT_PSNR), **kw)


def _pair(seed, n, w, h, bpc=8):
    return S.random_pair(seed, n, w, h, bpc)


def _padded(frames, pad=5, lead=1):
    h, w = frames[0].shape
    buf = np.zeros((len(frames), h, w + pad), frames[0].dtype)
    buf[:, :, lead:lead + w] = np.stack(frames)
    return buf, [buf[i, :, lead:lead + w] for i in range(len(frames))]


def _resident(eng, ref_buf, dis_buf, lead, shape, n, tile):
    import torch
    es = ref_buf.dtype.itemsize
    tr = torch.from_numpy(ref_buf.view(np.uint8).reshape(-1)).cuda()
    td = torch.from_numpy(dis_buf.view(np.uint8).reshape(-1)).cuda()
    torch.cuda.synchronize()
    return eng.flow_moments_resident(tr.data_ptr() + lead * es, ref_buf.strides[1], ref_buf.strides[0], td.data_ptr() + lead * es,
                                     dis_buf.strides[1], dis_buf.strides[0], shape, n, tile)


def test_smallest_calls_and_frame_counts():
    """3 x 3 at T = 8: one counted pixel, so the six sums are the six products of its gx, gy, dt; 16 x 16 at T = 8: four
    tiles; no frames at all"""
    with _engine() as eng:
        ref, dis = _pair(1, 2, 3, 3)
        got = eng.flow_moments(ref, dis, 8)
        assert got.dtype == np.int64 and got.shape == (2, 1, 1, 6) and np.array_equal(got, F.moments(ref, dis, 8))
        gx, gy, dt = (int(v[0, 0]) for v in F._fields(ref[1], dis[1], 8))
        assert got[1, 0, 0].tolist() == [gx * gx, gx * gy, gy * gy, gx * dt, gy * dt, dt * dt]
        ref, dis = _pair(2, 2, 16, 16)
        got = eng.flow_moments(ref, dis, 8)
        assert got.shape == (2, 2, 2, 6) and np.array_equal(got, F.moments(ref, dis, 8))
        assert eng.flow_moments([], [], 16).shape[0] == 0
        assert eng.flow_moments_resident(0, 16, 256, 0, 16, 256, (16, 16), 0, 8).shape == (0, 2, 2, 6)


def test_argument_rules():
    from pqa2_amd import _native as N
    ref, dis = _pair(3, 1, 40, 24)
    with _engine() as eng:
        good = eng.flow_moments(ref, dis, 8)
        small = _pair(4, 1, 2, 9)
        for call in (lambda: eng.flow_moments(ref, dis, 12),                                  # tiles are 8, 16, 32, 64
                     lambda: eng.flow_moments(ref, dis, 128),
                     lambda: eng.flow_moments(ref, dis, 0),
                     lambda: eng.flow_moments(*small, 8),                                      # a side below 3
                     lambda: eng.flow_moments_resident(4096, 8193, 8193 * 3, 8192, 8193, 8193 * 3, (3, 8193), 1, 8),
                     lambda: eng.flow_moments_resident(0, 40, 960, 8192, 40, 960, (24, 40), 1, 8),       # null planes
                     lambda: eng.flow_moments_resident(4096, 40, 960, 0, 40, 960, (24, 40), 1, 8),
                     lambda: eng.flow_moments_resident(4096, 39, 960, 8192, 40, 960, (24, 40), 1, 8),    # short rows
                     lambda: eng.flow_moments_resident(4096, 40, 960, 8192, 39, 960, (24, 40), 1, 8),
                     lambda: eng.flow_moments_resident(4096, 40, 960, 8192, 40, 960, (24, 40), -1, 8)):
            with pytest.raises(N.PqaError) as e:
                call()
            assert e.value.code == N.PQA_EINVAL
        sp = eng._flow_spec((24, 40), 8)
        rp, dp = (C.c_void_p * 1)(ref[0].ctypes.data), (C.c_void_p * 1)(dis[0].ctypes.data)
        out = np.zeros((1, 3, 5, 6), np.int64)
        lib, ctx = eng.lib, eng._ctx
        assert lib.pqa_flow_moments(ctx, None, rp, 40, dp, 40, 1, out.ctypes.data) == N.PQA_EINVAL
        assert lib.pqa_flow_moments(ctx, C.byref(sp), None, 40, dp, 40, 1, out.ctypes.data) == N.PQA_EINVAL
        assert lib.pqa_flow_moments(ctx, C.byref(sp), rp, 40, None, 40, 1, out.ctypes.data) == N.PQA_EINVAL
        assert lib.pqa_flow_moments(ctx, C.byref(sp), rp, 40, (C.c_void_p * 1)(), 40, 1, out.ctypes.data) == N.PQA_EINVAL
        assert lib.pqa_flow_moments(ctx, C.byref(sp), rp, 40, dp, 40, 1, None) == N.PQA_EINVAL
        assert lib.pqa_flow_moments(ctx, C.byref(sp), rp, 39, dp, 40, 1, out.ctypes.data) == N.PQA_EINVAL
        assert lib.pqa_flow_moments(ctx, C.byref(sp), rp, 40, dp, -40, 1, out.ctypes.data) == N.PQA_EINVAL
        assert lib.pqa_flow_moments(ctx, C.byref(sp), rp, 40, dp, 40, -1, out.ctypes.data) == N.PQA_EINVAL
        sp.struct_size -= 4
        assert lib.pqa_flow_moments(ctx, C.byref(sp), rp, 40, dp, 40, 1, out.ctypes.data) == N.PQA_EINVAL
        sp.struct_size += 4
        assert not out.any()
        assert lib.pqa_flow_moments(ctx, C.byref(sp), rp, 40, dp, 40, 1, out.ctypes.data) == N.PQA_OK
        assert np.array_equal(out, good) and np.array_equal(good, F.moments(ref, dis, 8))   # refused calls leave the context usable
    with _engine(bpc=10) as eng:      # a 16-bit context: pitches are whole samples
        with pytest.raises(N.PqaError) as e:
            eng.flow_moments_resident(4096, 81, 81 * 24, 8192, 80, 80 * 24, (24, 40), 1, 8)
        assert e.value.code == N.PQA_EINVAL


@pytest.mark.parametrize("tile", [8, 16])
@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_tails_pitches_and_depths(bpc, tile):
    """50 x 18: a row is no whole number of tiles; rows padded by 5 samples, base one sample in; the host entry on contiguous
    frames, on views, and the resident entry agree"""
    ref, dis = _pair(10 + bpc, 3, 50, 18, bpc)
    want = F.moments(ref, dis, tile, bpc)
    rbuf, rv = _padded(ref)
    dbuf, dv = _padded(dis)
    with _engine(bpc=bpc) as eng:
        assert np.array_equal(eng.flow_moments(ref, dis, tile), want)
        assert np.array_equal(eng.flow_moments(rv, dv, tile), want)
        assert np.array_equal(_resident(eng, rbuf, dbuf, 1, (18, 50), 3, tile), want)


@pytest.mark.parametrize("bpc,tile,w,h", [(8, 32, 67, 35), (10, 64, 130, 66), (8, 8, 65, 65), (12, 16, 130, 66)])
def test_tile_and_block_edges(bpc, tile, w, h):
    """67 x 35 at T = 32 and 130 x 66 at T = 64: the last tiles hold one counted pixel each way (x = 65 of 67, x = 128 of 130),
    and 130 x 66 is three workgroups across and two down; 65 x 65 at T = 8: the last tile holds column 64 only, which is not
    counted -- zeros; three frames for the per-frame stride"""
    ref, dis = _pair(20 + tile, 3, w, h, bpc)
    want = F.moments(ref, dis, tile, bpc)
    with _engine(bpc=bpc) as eng:
        got = eng.flow_moments(ref, dis, tile)
    assert got.shape == (3, -(-h // tile), -(-w // tile), 6) and np.array_equal(got, want)
    assert len({want[f].tobytes() for f in range(3)}) == 3
    if (tile, w) == (8, 65):
        assert not got[:, :, -1].any() and not got[:, -1].any() and got[:, :-1, :-1].any()


def test_nine_frames_cross_a_chunk():
    ref, dis = _pair(31, 9, 40, 24)
    with _engine() as eng:
        assert np.array_equal(eng.flow_moments(ref, dis, 16), F.moments(ref, dis, 16))


def test_accumulator_limits_at_the_extremes():
    """12 bit, 64 x 64 tiles (128 x 64 planes: two of them), samples 0xffff in the container (read as 4095).  Constant planes
    at the two extremes: dt = 16 * 4095 = 65 520 at every counted pixel, dt^2 > 2^31 a pixel.  A vertical step edge 0 | 4095
    in the reference against a constant 4095: beside the edge |gx| = 4 * 4095 with |dt| up to 12 * 4095; the same edge in both
    planes: gx = 8 * 4095 = 32 760, the bound.  The restatement's Python-int form is the reference."""
    top = 4095
    zero, full = np.zeros((64, 128), np.uint16), np.full((64, 128), 0xffff, np.uint16)
    edge = np.zeros((64, 128), np.uint16)
    edge[:, 32:] = 0xffff
    hedge = np.zeros((64, 128), np.uint16)
    hedge[31:] = 0xffff
    cases = [(zero, full), (full, zero), (edge, full), (edge, edge), (hedge, zero), (edge, hedge)]
    with _engine(bpc=12) as eng:
        got = eng.flow_moments([c[0] for c in cases], [c[1] for c in cases], 64)
    for k, (r, d) in enumerate(cases):
        assert got[k].tolist() == F.moments_exact(r, d, 64, 12), k
    assert got[0, 0, 0].tolist() == [0, 0, 0, 0, 0, 63 * 62 * (16 * top) ** 2]      # x = 1 ... 63 of the first tile
    assert got[0, 0, 1, 5] == 63 * 62 * (16 * top) ** 2 and got[0, 0, 0, 5] > 2 ** 43
    assert got[3, 0, 0, 0] == 2 * 62 * (8 * top) ** 2          # the two columns beside the edge, gx at its bound


def test_independent_of_the_scoring_chain():
    from pqa2_amd import _native as N
    rng = np.random.default_rng(7)
    ref = [rng.integers(0, 256, (48, 64)).astype(np.uint8) for _ in range(6)]
    dis = [np.clip(r.astype(int) + rng.integers(-9, 10, r.shape), 0, 255).astype(np.uint8) for r in ref]
    big_r, big_d = _pair(50, 2, 200, 120)

    def run(with_call):
        with _engine(64, 48, features=N.FEAT_VMAF | N.FEAT_PSNR | N.FEAT_SSIM, max_batch=4) as eng:
            outs = []
            for i in range(6):
                eng.submit(i, [ref[i]], [dis[i]])
                if with_call and i in (0, 2, 4):    # inside a pending batch, and right after one was launched
                    outs.append(eng.flow_moments(big_r, big_d, 32))
                    outs.append(eng.flow_moments(ref, dis, 8))
            return eng.collect(0, 6), outs
    plain, _ = run(False)
    mixed, outs = run(True)
    assert np.array_equal(plain.view(np.uint64), mixed.view(np.uint64))
    assert len(outs) == 6
    assert all(np.array_equal(o, F.moments(big_r, big_d, 32)) for o in outs[0::2])
    assert all(np.array_equal(o, F.moments(ref, dis, 8)) for o in outs[1::2])


# ---- the driver and end to end ----------------------------------------------------------------------------------------------
W, H, N_FRAMES = 192, 128, 6
GEOMETRY = (0.37, -0.61, 1.012, 0.992)      # the first geometry of tests/test_flow.py


def test_register_walks_the_same_integers_on_the_engine():
    from pqa2_amd import align as AL
    ref = [f[0] for f in S.natural_planes(41, 2, W, H)]
    dis = [F.capture(r, *GEOMETRY, noise=3, seed=100 + i) for i, r in enumerate(ref)]
    want_trace, got_trace = [], []
    want = AL.register(*F.restatements(8), ref, dis, filter="bicubic", tile=16, levels=1, trace=want_trace)
    with _engine(W, H) as eng:
        got = AL.register(eng.flow_moments, eng.resample, ref, dis, filter="bicubic", tile=16, levels=1, trace=got_trace)
    assert got == want and got["converged"] and got["iterations"] >= 1
    assert len(got_trace) == len(want_trace) >= 3
    for (gl, gw, gm), (wl, ww, wm) in zip(got_trace, want_trace):
        assert (gl, gw) == (wl, ww) and np.array_equal(gm, wm)


def _info(w, h, mono):
    from pqa2_amd.yuvio import VideoInfo
    return VideoInfo(width=w, height=h, fps_num=24, fps_den=1, bit_depth=8, mono=mono, hshift=0 if mono else 1,
                     vshift=0 if mono else 1, chroma_tag="mono" if mono else "420")


def _write(path, clip, mono, w=W, h=H):
    from pqa2_amd.yuvio import write_y4m
    write_y4m(str(path), clip, _info(w, h, mono))
    return str(path)


def _clips(tmp_path, mono):
    """reference and a capture of the geometry above (chroma: the same map at half the shift) plus noise of +-3"""
    frames = S.natural_planes(41, N_FRAMES, W, H, 0 if mono else 1, 0 if mono else 1, mono)
    dx, dy, sx, sy = GEOMETRY
    cap = [[F.capture(p, dx / (1 if k == 0 else 2), dy / (1 if k == 0 else 2), sx, sy, noise=3, seed=1000 + 10 * i + k)
            for k, p in enumerate(planes)] for i, planes in enumerate(frames)]
    return frames, cap, _write(tmp_path / "ref.y4m", frames, mono), _write(tmp_path / "dis.y4m", cap, mono)


def _by_hand(tmp_path, frames, cap, mono):
    """what score_files(register="bicubic") does, restated: align.register on the restatements over the sampled luma pairs,
    every captured plane through resample_ref with the plane's window, both clips cut to the crop"""
    from pqa2_amd import align as AL
    from pqa2_amd.pipeline import REGISTER_TILE, registration_crop, spatial_sample
    idx = spatial_sample(N_FRAMES, 8)
    geo = AL.register(*F.restatements(8), [frames[i][0] for i in idx], [cap[i][0] for i in idx], filter="bicubic",
                      tile=REGISTER_TILE, levels=None)
    assert AL.geometry_applied(geo)
    crop = registration_crop(geo, W, H, 0 if mono else 1, 0 if mono else 1)
    left, top, right, bottom = crop
    wc, hc = W - left - right, H - top - bottom
    dx, sx = AL.window_geometry(geo["x0_q16"], geo["w_q16"], W)
    dy, sy = AL.window_geometry(geo["y0_q16"], geo["h_q16"], H)

    def warp(plane, k):
        h, w = plane.shape
        (x0, ww), (y0, wh) = (AL.geometry_window(dx / (1 if k == 0 else 2), sx, w), AL.geometry_window(dy / (1 if k == 0 else 2), sy, h))
        return R.resize(plane, (h, w), "bicubic", 8, tuple(v / 65536.0 for v in (x0, y0, ww, wh)))

    def cut(planes):
        out = [planes[0][top:top + hc, left:left + wc]]
        for c in planes[1:]:
            out.append(c[top >> 1:(top >> 1) + (-(-hc >> 1)), left >> 1:(left >> 1) + (-(-wc >> 1))])
        return out
    ref_cut = [cut(f) for f in frames]
    dis_cut = [cut([warp(p, k) for k, p in enumerate(f)]) for f in cap]
    return geo, crop, _write(tmp_path / "ref_cut.y4m", ref_cut, mono, wc, hc), _write(tmp_path / "dis_cut.y4m", dis_cut, mono, wc, hc)


@pytest.mark.parametrize("mono", [True, False])
def test_end_to_end_equals_clips_registered_by_hand(tmp_path, mono):
    from pqa2_amd.pipeline import score_files
    frames, cap, ref_path, dis_path = _clips(tmp_path, mono)
    geo, crop, ref_cut, dis_cut = _by_hand(tmp_path, frames, cap, mono)
    res = score_files(ref_path, dis_path, "vmaf_v0.6.1", register="bicubic")
    g = res["alignment"]["geometry"]
    assert g["applied"] is True and g["filter"] == "bicubic" and g["frames"] == N_FRAMES and g["crop"] == crop
    assert {k: g[k] for k in geo} == geo
    assert abs(g["dx"] - GEOMETRY[0]) < 0.02 and abs(g["dy"] - GEOMETRY[1]) < 0.02
    assert abs(g["sx"] - GEOMETRY[2]) < 1e-3 and abs(g["sy"] - GEOMETRY[3]) < 1e-3
    by_hand = score_files(ref_cut, dis_cut, "vmaf_v0.6.1")
    assert res["records"].shape == by_hand["records"].shape == (N_FRAMES, 24)
    assert np.array_equal(res["records"].view(np.uint64), by_hand["records"].view(np.uint64))
    assert list(res["metrics"]) == list(by_hand["metrics"]) and ("psnr_cb" in res["metrics"]) == (not mono)
    plain = score_files(ref_path, dis_path, "vmaf_v0.6.1")
    assert "alignment" not in plain
    assert float(np.mean(res["metrics"]["vmaf"])) > float(np.mean(plain["metrics"]["vmaf"]))
    with pytest.raises(ValueError):
        score_files(ref_path, dis_path, "vmaf_v0.6.1", register="nearest")


def test_negative_controls(tmp_path):
    from pqa2_amd.pipeline import score_files
    frames, cap, ref_path, dis_path = _clips(tmp_path, True)
    same = score_files(ref_path, ref_path, "vmaf_v0.6.1", register="bicubic")
    g = same["alignment"]["geometry"]
    assert g["applied"] is False and g["converged"] is True and g["corner_px"] == 0.0 and g["crop"] == [0, 0, 0, 0]
    plain = score_files(ref_path, ref_path, "vmaf_v0.6.1")
    assert np.array_equal(same["records"].view(np.uint64), plain["records"].view(np.uint64))
    flat = [[np.full((H, W), 90, np.uint8)] for _ in range(N_FRAMES)]
    flat_path = _write(tmp_path / "flat.y4m", flat, True)
    res = score_files(flat_path, dis_path, "vmaf_v0.6.1", register="bicubic")      # a flat reference: sum gx^2 is the capture's alone
    res2 = score_files(flat_path, flat_path, "vmaf_v0.6.1", register="bicubic")    # flat against flat: the singular system
    g2 = res2["alignment"]["geometry"]
    assert g2["applied"] is False and g2["converged"] is False and g2["iterations"] == 0
    plain2 = score_files(flat_path, flat_path, "vmaf_v0.6.1")
    assert np.array_equal(res2["records"].view(np.uint64), plain2["records"].view(np.uint64))
    assert res["records"].shape == (N_FRAMES, 24)


def test_analyzer_writes_the_geometry_into_the_json(tmp_path):
    from pqa2_amd.vmaf_analyzer import VMAFAnalyzer
    frames, cap, ref_path, dis_path = _clips(tmp_path, True)
    an = VMAFAnalyzer()
    an.set_output_directory(str(tmp_path))
    an.set_test_name("register")
    an.register_filter = "bicubic"
    lines = []
    an.status_update.connect(lines.append)
    results = an.analyze_videos(ref_path, dis_path)
    assert results and results["alignment"]["geometry"]["applied"] is True
    g = json.load(open(results["json_path"]))["alignment"]["geometry"]
    assert g["filter"] == "bicubic" and g["frames"] == N_FRAMES and abs(g["dx"] - GEOMETRY[0]) < 0.02
    assert len(results["raw_results"]["frames"]) == N_FRAMES
    assert any(s.startswith("Registration: capture displaced by (+0.3") for s in lines)
