"""The exact-integer resampler on the MI355X (csrc/resample.hip, pqa_resample / pqa_resample_device).  Every expected plane
is the numpy restatement's two integer passes (tests/resample_ref.py: apply) fed with the LIBRARY'S OWN tables
(pqa_debug_resample_table), so the comparison is equality, no tolerance.  Content is independent uniform noise over the full
sample range with a row of 0 and a row of 2^b - 1: a wrong tap at a tile seam or a missing clamp shows.  A workgroup's
destination tile is 64 columns by 32 rows; the shapes below span at least three tiles across and two down plus a partial one
(150 x 101: 2 + a 22-column tile across, 3 + a 5-row tile down)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import resample_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILTERS = ("bilinear", "bicubic", "lanczos")


def _engine(w, h, bpc=8, **kw):
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    return FeatureEngine(w, h, bit_depth=bpc, n_planes=kw.pop("n_planes", 1), features=kw.pop("features", N.FEAT_PSNR), **kw)


def _lib_dense(lib, filt, n_src, n_dst, x0=0.0, ext=None):
    first, coeff, taps = np.zeros(n_dst, np.int32), np.zeros((n_dst, 32), np.int16), C.c_int32()
    rc = lib.pqa_debug_resample_table(R.FILTERS[filt], n_src, n_dst, R.q16(x0), R.q16(n_src if ext is None else ext),
                                      first.ctypes.data, coeff.ctypes.data, 32, C.byref(taps))
    assert rc == 0
    return R.dense(first, coeff, n_src)


def _expected(lib, src, dst_shape, filt, b, window=None):
    h, w = src.shape
    x0, y0, ww, wh = window if window is not None else (0, 0, w, h)
    return R.apply(src, _lib_dense(lib, filt, w, dst_shape[1], x0, ww), _lib_dense(lib, filt, h, dst_shape[0], y0, wh), b)


@pytest.mark.parametrize("filt", FILTERS)
def test_upscale_8_bit_all_filters(filt):
    """47 x 33 -> 150 x 101 on a context larger than the source (200 x 120)"""
    src = [R.noise(1, 47, 33, 8), R.noise(2, 47, 33, 8)]
    with _engine(200, 120) as eng:
        got = eng.resample(src, (101, 150), filt)
        assert len(got) == 2 and got[0].dtype == np.uint8 and got[0].shape == (101, 150)
        for g, s in zip(got, src):
            assert np.array_equal(g, _expected(eng.lib, s, (101, 150), filt, 8))


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("dst", [(144, 176), (75, 117)])
def test_downscale_8_bit_from_a_source_larger_than_the_context(filt, dst):
    """352 x 288 on a 64 x 48 context -> 176 x 144 (2x) and -> 117 x 75 (3.0x / 3.84x: Lanczos needs 19 and 24 taps)"""
    src = R.noise(3, 352, 288, 8)
    with _engine(64, 48) as eng:
        got = eng.resample([src], dst, filt)[0]
        assert np.array_equal(got, _expected(eng.lib, src, dst, filt, 8))


@pytest.mark.parametrize("bpc,sw,sh,dw,dh", [(10, 200, 120, 320, 192), (12, 64, 48, 96, 80)])
@pytest.mark.parametrize("filt", FILTERS)
def test_deeper_samples(filt, bpc, sw, sh, dw, dh):
    src = R.noise(bpc, sw, sh, bpc)
    with _engine(sw, sh, bpc) as eng:
        got = eng.resample([src], (dh, dw), filt)[0]
        assert got.dtype == np.uint16 and np.array_equal(got, _expected(eng.lib, src, (dh, dw), filt, bpc))


@pytest.mark.parametrize("filt", FILTERS)
def test_windows_and_identity(filt):
    src = R.noise(5, 64, 48, 8)
    with _engine(64, 48) as eng:
        assert np.array_equal(eng.resample([src], (48, 64), filt)[0], src)
        sub = eng.resample([src], (48, 64), filt, window=(0.25, -0.5, 64, 48))[0]
        assert np.array_equal(sub, _expected(eng.lib, src, (48, 64), filt, 8, (0.25, -0.5, 64, 48)))
        assert not np.array_equal(sub, src)
        whole = eng.resample([src], (48, 64), filt, window=(3, 2, 64, 48))[0]
        assert np.array_equal(whole, R.replicated_crop(src, 3, 2))
        zoom = eng.resample([src], (101, 150), filt, window=(10.5, 7.25, 30, 20))[0]     # a window and a resize together
        assert np.array_equal(zoom, _expected(eng.lib, src, (101, 150), filt, 8, (10.5, 7.25, 30, 20)))
        flat = np.full((48, 64), 200, np.uint8)
        assert (eng.resample([flat], (101, 150), filt)[0] == 200).all()


@pytest.mark.parametrize("bpc", [8, 10])
def test_device_entry_with_odd_pitches_keeps_the_padding(bpc):
    """rows 3 (source) and 5 (destination) samples longer than a row, bases one sample in: the per-sample loads and stores;
    every byte of the destination buffer outside the rows keeps its sentinel.  Then 16-byte-aligned pitches: the 4-sample
    loads and stores, with a row tail (150 is no multiple of 4)."""
    import torch
    dt, es = (np.uint8, 1) if bpc == 8 else (np.uint16, 2)
    n, sw, sh, dw, dh = 3, 47, 33, 150, 101
    src = [R.noise(20 + f, sw, sh, bpc) for f in range(n)]
    with _engine(64, 48, bpc) as eng:
        want = [_expected(eng.lib, s, (dh, dw), "bicubic", bpc) for s in src]
        for spad, dpad, lead in ((3, 5, 1), (1, 10, 0)):
            sbuf = np.zeros((n, sh + 1, sw + spad), dt)
            for f in range(n):
                sbuf[f, :sh, lead:lead + sw] = src[f]
            dbuf = np.full((n, dh + 1, dw + dpad), 0xA5 if bpc == 8 else 0x3A5, dt)
            ts = torch.from_numpy(sbuf.view(np.uint8).reshape(-1)).cuda()
            td = torch.from_numpy(dbuf.view(np.uint8).reshape(-1)).cuda()
            torch.cuda.synchronize()
            eng.resample_resident(ts.data_ptr() + lead * es, sbuf.strides[1], sbuf.strides[0], (sh, sw), td.data_ptr() + lead * es,
                                  dbuf.strides[1], dbuf.strides[0], (dh, dw), n, "bicubic")
            out = td.cpu().numpy().view(dt).reshape(dbuf.shape)
            for f in range(n):
                assert np.array_equal(out[f, :dh, lead:lead + dw], want[f])
            keep = np.ones(dbuf.shape, bool)
            keep[:, :dh, lead:lead + dw] = False
            assert (out[keep] == dbuf[keep]).all()


def test_frame_counts_and_host_views():
    """0, 1 and 9 frames (9: more than one chunk of 8); frames that are views with a common odd stride"""
    src = [R.noise(30 + f, 47, 33, 8) for f in range(9)]
    with _engine(64, 48) as eng:
        want = [_expected(eng.lib, s, (40, 70), "lanczos", 8) for s in src]
        assert len({w.tobytes() for w in want}) == 9
        assert eng.resample([], (40, 70), "lanczos") == []
        eng.resample_resident(0, 47, 47 * 33, (33, 47), 0, 70, 70 * 40, (40, 70), 0)
        for n in (1, 9):
            got = eng.resample(src[:n], (40, 70), "lanczos")
            assert len(got) == n and all(np.array_equal(g, w) for g, w in zip(got, want))
        buf = np.zeros((9, 33, 52), np.uint8)
        buf[:, :, 1:48] = np.stack(src)
        got = eng.resample([buf[f, :, 1:48] for f in range(9)], (40, 70), "lanczos")
        assert all(np.array_equal(g, w) for g, w in zip(got, want))


def test_argument_rules():
    from pqa2_amd import _native as N
    src = R.noise(40, 64, 48, 8)
    with _engine(64, 48) as eng:
        good = eng.resample([src], (24, 32), "bicubic")[0]
        for call in (lambda: eng.resample([src], (24, 0), "bicubic"),
                     lambda: eng.resample([src], (24, 8193), "bicubic"),
                     lambda: eng.resample([src], (8, 32), "lanczos"),                        # 6x down: 36 taps
                     lambda: eng.resample([src], (24, 32), "bicubic", window=(0, 0, 0, 48)),
                     lambda: eng.resample([src], (24, 32), "bicubic", window=(0, 0, 64, -1)),
                     lambda: eng.resample_resident(0, 64, 64 * 48, (48, 64), 0, 32, 32 * 24, (24, 32), 1),       # null planes
                     lambda: eng.resample_resident(4096, 63, 64 * 48, (48, 64), 8192, 32, 32 * 24, (24, 32), 1),  # short rows
                     lambda: eng.resample_resident(4096, 64, 64 * 48, (48, 64), 8192, 31, 32 * 24, (24, 32), 1),
                     lambda: eng.resample_resident(4096, 64, 64 * 48, (48, 64), 8192, 32, 32 * 24, (24, 32), -1)):
            with pytest.raises(N.PqaError) as e:
                call()
            assert e.value.code == N.PQA_EINVAL
        with pytest.raises(ValueError):
            eng.resample([src], (24, 32), "nearest")
        sp = eng._resample_spec((48, 64), (24, 32), "bicubic", None)
        ptr = (C.c_void_p * 1)(src.ctypes.data)
        out = np.zeros((24, 32), np.uint8)
        optr = (C.c_void_p * 1)(out.ctypes.data)
        assert eng.lib.pqa_resample(eng._ctx, None, ptr, 64, optr, 32, 1) == N.PQA_EINVAL
        assert eng.lib.pqa_resample(eng._ctx, C.byref(sp), None, 64, optr, 32, 1) == N.PQA_EINVAL
        assert eng.lib.pqa_resample(eng._ctx, C.byref(sp), ptr, 64, (C.c_void_p * 1)(), 32, 1) == N.PQA_EINVAL
        sp.struct_size -= 8
        assert eng.lib.pqa_resample(eng._ctx, C.byref(sp), ptr, 64, optr, 32, 1) == N.PQA_EINVAL
        sp.struct_size += 8
        sp.filter = 3
        assert eng.lib.pqa_resample(eng._ctx, C.byref(sp), ptr, 64, optr, 32, 1) == N.PQA_EINVAL
        assert not out.any()
        assert np.array_equal(eng.resample([src], (24, 32), "bicubic")[0], good)     # a refused call leaves the context usable


def test_independent_of_the_scoring_chain():
    from pqa2_amd import _native as N
    rng = np.random.default_rng(7)
    ref = [rng.integers(0, 256, (48, 64)).astype(np.uint8) for _ in range(6)]
    dis = [np.clip(r.astype(int) + rng.integers(-9, 10, r.shape), 0, 255).astype(np.uint8) for r in ref]
    big = R.noise(50, 352, 288, 8)

    def run(with_call):
        with _engine(64, 48, features=N.FEAT_VMAF | N.FEAT_PSNR | N.FEAT_SSIM, max_batch=4) as eng:
            outs = []
            for i in range(6):
                eng.submit(i, [ref[i]], [dis[i]])
                if with_call and i in (0, 2, 4):    # inside a pending batch, and right after one was launched
                    outs.append(eng.resample([big], (144, 176), "bicubic")[0])
                    outs.append(eng.resample([dis[i]], (101, 150), "lanczos")[0])
            return eng.collect(0, 6), outs, eng.lib
    plain, _, _ = run(False)
    mixed, outs, lib = run(True)
    assert np.array_equal(plain.view(np.uint64), mixed.view(np.uint64))
    assert len(outs) == 6
    want = _expected(lib, big, (144, 176), "bicubic", 8)
    assert all(np.array_equal(o, want) for o in outs[0::2])
    assert all(np.array_equal(o, _expected(lib, dis[i], (101, 150), "lanczos", 8)) for o, i in zip(outs[1::2], (0, 2, 4)))


# ---- end to end -----------------------------------------------------------------------------------------------------------
def _write_clips(tmp_path):
    """the 64 x 48 golden reference; its distorted partner decimated by two in numpy (every second sample of every plane);
    and that small clip brought back to 64 x 48 by the restatement, bicubic"""
    import dataclasses
    from pqa2_amd.yuvio import open_video, write_y4m
    ref = os.path.join(ROOT, "tests", "golden", "clips", "c64x48_8_ref.y4m")
    rd = open_video(os.path.join(ROOT, "tests", "golden", "clips", "c64x48_8_dist.y4m"))
    info = rd.info
    small = [[np.ascontiguousarray(p[::2, ::2]) for p in rd.frame(i)] for i in range(len(rd))]
    small_info = dataclasses.replace(info, width=info.width // 2, height=info.height // 2)
    assert [p.shape for p in small[0]] == [(24, 32), (12, 16), (12, 16)]
    full = [[R.resize(p, shape, "bicubic", 8) for p, shape in zip(f, [(48, 64), (24, 32), (24, 32)])] for f in small]
    paths = {"ref": ref, "small": str(tmp_path / "small.y4m"), "full": str(tmp_path / "full.y4m")}
    write_y4m(paths["small"], small, small_info)
    write_y4m(paths["full"], full, info)
    return paths, len(small)


def test_end_to_end_resize_equals_a_prescaled_file(tmp_path):
    from pqa2_amd.pipeline import score_files
    p, n = _write_clips(tmp_path)
    with pytest.raises(ValueError, match="reference is 64x48 but distorted is 32x24"):
        score_files(p["ref"], p["small"], "vmaf_v0.6.1")
    got = score_files(p["ref"], p["small"], "vmaf_v0.6.1", resize="bicubic")
    want = score_files(p["ref"], p["full"], "vmaf_v0.6.1")
    assert got["resize"] == {"filter": "bicubic", "from": [32, 24], "to": [64, 48], "applied": True}
    assert got["records"].shape == want["records"].shape == (n, 24)
    assert np.array_equal(got["records"].view(np.uint64), want["records"].view(np.uint64))
    for k in want["metrics"]:
        assert np.array_equal(np.asarray(got["metrics"][k]), np.asarray(want["metrics"][k])), k
    same = score_files(p["ref"], p["full"], "vmaf_v0.6.1", resize="lanczos")      # equal sizes: the option changes nothing
    assert same["resize"] == {"filter": "lanczos", "from": [64, 48], "to": [64, 48], "applied": False}
    assert "resize" not in want and np.array_equal(same["records"].view(np.uint64), want["records"].view(np.uint64))
    with pytest.raises(ValueError):
        score_files(p["ref"], p["small"], "vmaf_v0.6.1", resize="nearest")
