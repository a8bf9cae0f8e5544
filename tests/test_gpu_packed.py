"""Packed capture formats on the GPU (UYVY, YUYV, v210; pqa2_amd/csrc/unpack.hip): the unpacked planes are the integers
tests/packed_ref.py packs, byte for byte, and every record from a packed clip is bit-identical to the planar submission of
the same samples -- through pqa_unpack[_device], pqa_submit_surfaces, pqa_submit_packed and score_files.  Every assertion
is an exact equality: the kernel only moves bits."""
import os

import numpy as np
import pytest

from tests import packed_ref as PR

pytestmark = pytest.mark.gpu

CONST = {"uyvy422": 3, "yuyv422": 4, "v210": 5}


def _round_up(v, m):
    return (v + m - 1) // m * m


def _clip422(w, h, n, bpc, t0=0):
    """the synthetic clip as 4:2:2: its 4:2:0 chroma rows doubled (any chroma does: the kernels are compared with themselves)"""
    from pqa2_amd import synth
    refs, diss = synth.make_clip(w, h, n, bpc, chroma=True, t0=t0)
    up = lambda f: [f[0]] + [np.ascontiguousarray(np.repeat(p, 2, axis=0)[:h]) for p in f[1:]]
    return [up(f) for f in refs], [up(f) for f in diss]


def _device_frames(torch, fmt, frames, w, pitch, gap_rows=1, seed=0):
    """n packed frames on the device: rows `pitch` bytes apart, frames (h + gap_rows) * pitch apart, and the allocation ends
    with the last used byte of the last row -> (byte tensor, frame pitch)"""
    h = frames[0][0].shape[0]
    fp = (h + gap_rows) * pitch
    flat = np.empty(len(frames) * fp, np.uint8)
    flat[:] = 0xC3
    for i, (y, u, v) in enumerate(frames):
        flat[i * fp:i * fp + h * pitch].reshape(h, pitch)[:] = PR.pack(fmt, y, u, v, stride=pitch, seed=seed + i, ones=i % 2 == 0)
    used = (len(frames) - 1) * fp + (h - 1) * pitch + PR.min_row_bytes(fmt, w)
    return torch.from_numpy(flat[:used].copy()).cuda(), fp


SIZES = [(16, 16), (19, 17), (48, 16), (50, 16), (52, 20), (96, 18), (642, 362), (1920, 1080)]


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("fmt", PR.FORMATS)
def test_unpacked_planes_are_the_packed_samples(fmt, w, h):
    import torch
    from pqa2_amd.engine import FeatureEngine
    n = 2 if w > 1000 else 3
    es = np.dtype(PR.DTYPE[fmt]).itemsize
    cw = PR.chroma_width(w)
    frames = [PR.random_planes(fmt, w, h, seed=7 * w + h + i) for i in range(n)]
    row = PR.min_row_bytes(fmt, w)
    with FeatureEngine(64, 64, bit_depth=PR.BIT_DEPTH[fmt]) as eng:   # the context's own size does not matter
        # device clips: aligned pitches (the 16-byte path) and pitches padded by an odd number of samples (sample by sample)
        for aligned in (True, False):
            spitch = _round_up(row, 16) + 16 if aligned else row + (4 if fmt == "v210" else 3)
            src, sfp = _device_frames(torch, fmt, frames, w, spitch, seed=w)
            dpitch = [(_round_up(k * es, 16) + 16) if aligned else (k + 3) * es for k in (w, cw, cw)]
            dfp = [(h + 1) * p for p in dpitch]
            for luma_only in (False, True):
                dst = [torch.full((n * dfp[p],), 0xA5, dtype=torch.uint8, device="cuda") for p in range(1 if luma_only else 3)]
                torch.cuda.synchronize()
                eng.unpack_resident(fmt, (h, w), src.data_ptr(), spitch, sfp, n, [d.data_ptr() for d in dst], dpitch, dfp)
                for p, d in enumerate(dst):
                    got = d.cpu().numpy().reshape(n, h + 1, dpitch[p])
                    k = (w, cw, cw)[p]
                    for i in range(n):
                        samples = np.ascontiguousarray(got[i, :h, :k * es]).view(PR.DTYPE[fmt])
                        assert np.array_equal(samples, frames[i][p]), (fmt, w, h, aligned, luma_only, p, i)
                    assert np.all(got[:, :h, k * es:] == 0xA5) and np.all(got[:, h:, :] == 0xA5), (fmt, w, h, aligned, luma_only, p)
        # host frames: file-stride rows, three planes and luma only
        stride = PR.file_stride(fmt, w)
        packed = [PR.pack(fmt, *f, stride=stride, seed=i, ones=False) for i, f in enumerate(frames)]
        for luma_only in (False, True):
            out = eng.unpack(packed, fmt, (h, w), luma_only=luma_only)
            assert len(out) == n and all(len(o) == (1 if luma_only else 3) for o in out)
            for i, o in enumerate(out):
                for p, plane in enumerate(o):
                    assert plane.dtype == PR.DTYPE[fmt] and np.array_equal(plane, frames[i][p]), (fmt, w, h, luma_only, p, i)
        # the numpy unpack of the reader is the same statement
        from pqa2_amd import yuvio
        for p, plane in enumerate(yuvio.unpack_packed(fmt, packed[0], w)):
            assert np.array_equal(plane, frames[0][p])


def _planar_records(w, h, bpc, refs, diss, first=0, **kw):
    from pqa2_amd.engine import FeatureEngine
    with FeatureEngine(w, h, bit_depth=bpc, **kw) as eng:
        for i in range(first, len(refs)):
            eng.submit(i, refs[i], diss[i])
        return eng.collect(first, len(refs) - first)


@pytest.mark.parametrize("fmt,w,h,pad", [("uyvy422", 52, 20, 0), ("yuyv422", 96, 18, 0), ("v210", 52, 20, 0), ("v210", 96, 18, 0),
                                         ("uyvy422", 642, 362, 5), ("yuyv422", 642, 362, 0), ("v210", 642, 362, 20)])
def test_packed_surfaces_give_the_planar_records(fmt, w, h, pad):
    import torch
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    n, bpc = 5, PR.BIT_DEPTH[fmt]
    refs, diss = _clip422(w, h, n, bpc)
    kw = dict(n_planes=3, chroma_shift=(1, 0), features=N.FEAT_ALL, max_batch=2)
    planar = _planar_records(w, h, bpc, refs, diss, **kw)
    pitch = _round_up(PR.min_row_bytes(fmt, w), 16) + pad
    R, rfp = _device_frames(torch, fmt, refs, w, pitch, seed=1)
    D, dfp = _device_frames(torch, fmt, diss, w, pitch, seed=2)
    torch.cuda.synchronize()
    mk = lambda T, fp, f0=0: FeatureEngine.surface_clip(CONST[fmt], T.data_ptr() + f0 * fp, pitch, fp)
    with FeatureEngine(w, h, bit_depth=bpc, **kw) as eng:
        eng.submit_surfaces(0, n, mk(R, rfp), mk(D, dfp))
        assert np.array_equal(eng.collect(0, n).view(np.uint64), planar.view(np.uint64))
    # a frame-sharded rank: frames 2.. with a packed frame 1 of the reference as the motion halo
    with FeatureEngine(w, h, bit_depth=bpc, **kw) as eng:
        eng.submit_surfaces(2, n - 2, mk(R, rfp, 2), mk(D, dfp, 2), prev_ref=mk(R, rfp, 1))
        assert np.array_equal(eng.collect(2, n - 2).view(np.uint64), planar[2:].view(np.uint64))
    # one context: host planes, then packed surfaces (motion continues across the switch), then host planes
    with FeatureEngine(w, h, bit_depth=bpc, **kw) as eng:
        for i in range(2):
            eng.submit(i, refs[i], diss[i])
        eng.submit_surfaces(2, 2, mk(R, rfp, 2), mk(D, dfp, 2))
        eng.submit(4, refs[4], diss[4])
        assert np.array_equal(eng.collect(0, n).view(np.uint64), planar.view(np.uint64))


def test_luma_only_context_mixes_nv12_and_uyvy():
    """the 4:2:0 master as NV12 against the 4:2:2 capture as UYVY in ONE call: no chroma is decoded on either side"""
    import torch
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    w, h, n = 96, 18, 5
    refs, diss = _clip422(w, h, n, 8)
    planar = _planar_records(w, h, 8, [f[:1] for f in refs], [f[:1] for f in diss], max_batch=4)
    lp = w + 3
    L = np.full((n, h, lp), 0xA5, np.uint8)
    for i, f in enumerate(refs):
        L[i, :, :w] = f[0]
    RL = torch.from_numpy(L).cuda()
    pitch = PR.min_row_bytes("uyvy422", w) + 3
    D, dfp = _device_frames(torch, "uyvy422", diss, w, pitch, seed=3)
    torch.cuda.synchronize()
    with FeatureEngine(w, h, max_batch=4) as eng:
        eng.submit_surfaces(0, n, FeatureEngine.surface_clip(N.SURFACE_NV12, RL.data_ptr(), lp, h * lp),
                            FeatureEngine.surface_clip(N.SURFACE_UYVY, D.data_ptr(), pitch, dfp))
        assert np.array_equal(eng.collect(0, n).view(np.uint64), planar.view(np.uint64))


@pytest.mark.parametrize("fmt", ["uyvy422", "v210"])
def test_packed_prev_ref_arms_every_history(fmt):
    """xpsnr + siti + integrity on a shard that starts at frame 2: the packed prev_ref is motion's halo and the one reference
    frame xpsnr and siti look back to, as set_ref_history([frame 1]) is for planar frames"""
    import torch
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    w, h, n, bpc = 322, 182, 5, PR.BIT_DEPTH[fmt]
    refs, diss = _clip422(w, h, n, bpc)
    kw = dict(bit_depth=bpc, n_planes=3, chroma_shift=(1, 0), max_batch=2,
              features=N.FEAT_ALL | N.FEAT_XPSNR | N.FEAT_SITI | N.FEAT_INTEGRITY)
    with FeatureEngine(w, h, **kw) as eng:
        eng.set_ref_history([refs[1][0]])
        for i in range(2, n):
            eng.submit(i, refs[i], diss[i])
        planar = eng.collect_ext5(2, n - 2)
    pitch = _round_up(PR.min_row_bytes(fmt, w), 16)
    R, rfp = _device_frames(torch, fmt, refs, w, pitch, seed=4)
    D, dfp = _device_frames(torch, fmt, diss, w, pitch, seed=5)
    torch.cuda.synchronize()
    mk = lambda T, fp, f0: FeatureEngine.surface_clip(CONST[fmt], T.data_ptr() + f0 * fp, pitch, fp)
    with FeatureEngine(w, h, **kw) as eng:
        eng.submit_surfaces(2, n - 2, mk(R, rfp, 2), mk(D, dfp, 2), prev_ref=mk(R, rfp, 1))
        packed = eng.collect_ext5(2, n - 2)
    assert len(packed) == len(planar) == 6
    for a, b in zip(packed, planar):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("fmt,w,h", [("uyvy422", 96, 18), ("yuyv422", 52, 20), ("v210", 96, 18), ("v210", 642, 362)])
def test_submit_packed_gives_the_planar_records(fmt, w, h):
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    n, bpc = 11, PR.BIT_DEPTH[fmt]   # chunks of 8 + 3
    refs, diss = _clip422(w, h, n, bpc)
    kw = dict(n_planes=3, chroma_shift=(1, 0), features=N.FEAT_ALL, max_batch=4)
    planar = _planar_records(w, h, bpc, refs, diss, **kw)
    stride = PR.file_stride(fmt, w)
    pk = lambda clip, seed: [PR.pack(fmt, *f, stride=stride, seed=seed + i) for i, f in enumerate(clip)]
    # reference planar, captured packed; the caller's buffers are overwritten right after the call returns
    with FeatureEngine(w, h, bit_depth=bpc, **kw) as eng:
        rp, dp = [[p.copy() for p in f] for f in refs], pk(diss, 10)
        eng.submit_packed(0, (rp, None), (dp, fmt))
        for f in rp:
            for p in f:
                p[:] = 0
        for a in dp:
            a[:] = 0xFF
        assert np.array_equal(eng.collect(0, n).view(np.uint64), planar.view(np.uint64))
    # both packed
    with FeatureEngine(w, h, bit_depth=bpc, **kw) as eng:
        rp, dp = pk(refs, 20), pk(diss, 30)
        eng.submit_packed(0, (rp, fmt), (dp, fmt))
        for a in rp + dp:
            a[:] = 0x11
        assert np.array_equal(eng.collect(0, n).view(np.uint64), planar.view(np.uint64))
    # interleaved with pqa_submit: motion continues across both switches
    with FeatureEngine(w, h, bit_depth=bpc, **kw) as eng:
        for i in range(3):
            eng.submit(i, refs[i], diss[i])
        eng.submit_packed(3, (pk(refs[3:8], 40), fmt), (pk(diss[3:8], 50), fmt))
        for i in range(8, n):
            eng.submit(i, refs[i], diss[i])
        assert np.array_equal(eng.collect(0, n).view(np.uint64), planar.view(np.uint64))


def test_submit_packed_large_frames():
    """frames of 4 MB and more are packed by the pack pool's threads instead of the caller alone: the same records"""
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    w, h, n, fmt = 1920, 1080, 3, "v210"
    rng = np.random.default_rng(3)
    refs = [PR.random_planes(fmt, w, h, seed=i) for i in range(n)]
    diss = [[np.clip(p.astype(np.int32) + rng.integers(-2, 3, p.shape), 0, 1023).astype(np.uint16) for p in f] for f in refs]
    kw = dict(n_planes=3, chroma_shift=(1, 0), features=N.FEAT_PSNR | N.FEAT_MOTION, max_batch=2)
    planar = _planar_records(w, h, 10, refs, diss, **kw)
    stride = PR.file_stride(fmt, w)
    with FeatureEngine(w, h, bit_depth=10, **kw) as eng:
        eng.submit_packed(0, (refs, None), ([PR.pack(fmt, *f, stride=stride, seed=i) for i, f in enumerate(diss)], fmt))
        assert np.array_equal(eng.collect(0, n).view(np.uint64), planar.view(np.uint64))


def test_packed_argument_errors():
    import ctypes as C
    import torch
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    w, h = 96, 18
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    clip = lambda fmt, pitch: FeatureEngine.surface_clip(fmt, p, pitch, h * pitch)
    r8, r10 = PR.min_row_bytes("uyvy422", w), PR.min_row_bytes("v210", w)

    def refused(eng, ref, dis, *words):
        with pytest.raises(N.PqaError) as e:
            eng.submit_surfaces(0, 1, ref, dis)
        assert e.value.code == N.PQA_EINVAL and all(wd in str(e.value) for wd in words), str(e.value)

    kw = dict(n_planes=3, chroma_shift=(1, 0), features=N.FEAT_ALL)
    with FeatureEngine(w, h, **kw) as eng:                      # 8 bit
        ok = clip(N.SURFACE_UYVY, r8)
        refused(eng, clip(N.SURFACE_V210, r10), ok, "format", "8-bit")
        refused(eng, ok, clip(N.SURFACE_YUYV, r8 - 1), "pitch")
        bad = clip(N.SURFACE_UYVY, r8)
        bad.struct_size -= 4
        refused(eng, bad, ok, "struct_size")
        eng.submit_surfaces(0, 1, ok, clip(N.SURFACE_YUYV, r8))   # and the context is still usable
        with pytest.raises(N.PqaError) as e:                     # frame 0's record is uncollected: nothing is copied or launched
            eng.submit_surfaces(16384, 1, ok, ok)
        assert e.value.code == N.PQA_ESTATE
        with pytest.raises(N.PqaError) as e:
            eng.submit_packed(16384, ([np.zeros((h, r8), np.uint8)], "uyvy422"), ([np.zeros((h, r8), np.uint8)], "uyvy422"))
        assert e.value.code == N.PQA_ESTATE
        assert np.all(np.isfinite(eng.collect(0, 1)))
        with pytest.raises(N.PqaError) as e:                     # the host entry: a short stride, a format of the wrong depth
            eng.submit_packed(1, ([np.zeros((h, r8 - 4), np.uint8)], "uyvy422"), ([np.zeros((h, r8), np.uint8)], "uyvy422"))
        assert e.value.code == N.PQA_EINVAL and "pitch" in str(e.value)
        with pytest.raises(N.PqaError) as e:
            eng.submit_packed(1, ([np.zeros((h, r10), np.uint8)], "v210"), ([np.zeros((h, r8), np.uint8)], "uyvy422"))
        assert e.value.code == N.PQA_EINVAL and "format" in str(e.value)
        hc = N.PqaHostClip()                                     # struct_size left 0
        with pytest.raises(N.PqaError) as e:
            eng._check(eng.lib.pqa_submit_packed(eng._ctx, 1, 0, C.byref(hc), C.byref(hc)))
        assert e.value.code == N.PQA_EINVAL and "struct_size" in str(e.value)
        sp = N.PqaUnpackSpec()                                   # pqa_unpack_device: struct_size, format, size, pitch
        d = N.PqaDeviceClip()
        d.plane[0], d.row_pitch[0], d.frame_pitch[0] = p, w, w * h
        for fill, word in ((lambda: None, "struct_size"),
                           (lambda: setattr(sp, "struct_size", C.sizeof(sp)) or setattr(sp, "format", 2), "format"),
                           (lambda: setattr(sp, "format", 3) or setattr(sp, "width", 0), "size"),
                           (lambda: setattr(sp, "width", w) or setattr(sp, "height", h), "pitch")):
            fill()
            with pytest.raises(N.PqaError) as e:
                eng._check(eng.lib.pqa_unpack_device(eng._ctx, C.byref(sp), p, r8 - 1, h * r8, 1, C.byref(d)))
            assert e.value.code == N.PQA_EINVAL and word in str(e.value), str(e.value)
        eng.unpack_resident("uyvy422", (h, w), p, r8, h * r8, 1, [p + 8192], [w], [w * h])   # usable afterwards
    with FeatureEngine(w, h, bit_depth=10, **kw) as eng:        # 10 bit
        ok = clip(N.SURFACE_V210, r10)
        refused(eng, clip(N.SURFACE_UYVY, r8), ok, "format", "10-bit")
        refused(eng, ok, clip(N.SURFACE_V210, r10 - 16), "pitch")
        refused(eng, ok, clip(N.SURFACE_V210, r10 + 2), "multiple", "4")
        eng.submit_surfaces(0, 1, ok, ok)
        assert np.all(np.isfinite(eng.collect(0, 1)))
    with FeatureEngine(w, h, bit_depth=12, **kw) as eng:        # 12 bit takes none of them
        p01x = FeatureEngine.surface_clip(N.SURFACE_P01X, p, 2 * w, 2 * w * h)
        for fmt, row in ((N.SURFACE_UYVY, r8), (N.SURFACE_YUYV, r8), (N.SURFACE_V210, r10)):
            refused(eng, clip(fmt, row), p01x, "format", "12-bit")
    for shift in ((1, 1), (0, 0)):                              # a three-plane 4:2:0 or 4:4:4 context with a packed side
        with FeatureEngine(w, h, n_planes=3, chroma_shift=shift, features=N.FEAT_ALL) as eng:
            refused(eng, clip(N.SURFACE_UYVY, r8), clip(N.SURFACE_UYVY, r8), "4:2:2")
            with pytest.raises(N.PqaError) as e:
                eng.submit_packed(0, ([np.zeros((h, r8), np.uint8)], "uyvy422"), ([np.zeros((h, r8), np.uint8)], "uyvy422"))
            assert e.value.code == N.PQA_EINVAL and "4:2:2" in str(e.value)


def _write_pair(tmp_path, w, h, n, bpc, chroma):
    """reference / distorted Y4M files of the synthetic clip: chroma "422" or "420" -> (paths, clips)"""
    from pqa2_amd import synth, yuvio
    if chroma == "422":
        refs, diss = _clip422(w, h, n, bpc)
    else:
        refs, diss = synth.make_clip(w, h, n, bpc, chroma=True)
    tag = chroma if bpc == 8 else f"{chroma}p{bpc}"
    info = yuvio.VideoInfo(w, h, bpc, 1, 0 if chroma == "422" else 1, False, 30, 1, 0, tag)
    paths = []
    for name, clip in (("ref", refs), ("dis", diss)):
        paths.append(str(tmp_path / f"{name}_{chroma}_{bpc}.y4m"))
        yuvio.write_y4m(paths[-1], clip, info)
    return paths, refs, diss


def _write_packed(path, fmt, clip, w):
    with open(path, "wb") as f:
        for i, (y, u, v) in enumerate(clip):
            f.write(PR.pack(fmt, y, u, v, stride=PR.file_stride(fmt, w), seed=i).tobytes())


def _same(a, b, where=""):
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), (where, list(a), list(b))
        for k in a:
            _same(a[k], b[k], f"{where}/{k}")
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), where
    else:
        assert a == b, where


def _same_result(got, want):
    skip = {"input", "fps", "info"}
    assert [k for k in got if k not in skip] == [k for k in want if k not in skip]
    for k in want:
        if k not in skip:
            _same(got[k], want[k], k)


@pytest.mark.parametrize("fmt,ext", [("uyvy422", ".uyvy"), ("v210", ".v210")])
@pytest.mark.parametrize("w,h", [(96, 18), (642, 362)])
def test_score_files_takes_packed_captures(tmp_path, fmt, ext, w, h):
    from pqa2_amd.pipeline import score_files
    n, bpc = 10, PR.BIT_DEPTH[fmt]
    (ref, dis), refs, diss = _write_pair(tmp_path, w, h, n, bpc, "422")
    want = score_files(ref, dis)
    assert "input" not in want
    cap = str(tmp_path / f"capture_{w}x{h}{ext}")
    _write_packed(cap, fmt, diss, w)
    got = score_files(ref, cap)
    _same_result(got, want)
    y4m_fmt = "yuv422p" if bpc == 8 else "yuv422p10le"
    assert got["input"] == {"reference": y4m_fmt, "distorted": fmt, "planes_scored": "yuv", "packed_upload": True}
    assert set(want["metrics"]) >= {"vmaf", "psnr_y", "psnr_cb", "psnr_cr", "ssim"}


@pytest.mark.parametrize("w,h", [(96, 18), (642, 362)])
def test_score_files_scores_the_luma_of_a_420_master_against_a_uyvy_capture(tmp_path, w, h):
    from pqa2_amd import yuvio
    from pqa2_amd.pipeline import score_files
    n = 10
    (ref, _), refs, diss = _write_pair(tmp_path, w, h, n, 8, "420")
    d422 = [[f[0]] + [np.ascontiguousarray(np.repeat(p, 2, axis=0)[:h]) for p in f[1:]] for f in diss]
    cap = str(tmp_path / f"capture_{w}x{h}.uyvy")
    _write_packed(cap, "uyvy422", d422, w)
    with pytest.raises(ValueError, match="reference and distorted clips differ in pixel format"):
        score_files(ref, cap)
    got = score_files(ref, cap, chroma_mismatch="luma")
    mono = yuvio.VideoInfo(w, h, 8, 0, 0, True, 30, 1, 0, "mono")
    mref, mdis = str(tmp_path / "ref_mono.y4m"), str(tmp_path / "dis_mono.y4m")
    yuvio.write_y4m(mref, [f[:1] for f in refs], mono)
    yuvio.write_y4m(mdis, [f[:1] for f in diss], mono)
    want = score_files(mref, mdis)
    _same_result(got, want)
    assert "psnr_cb" not in got["metrics"] and "psnr_y" in got["metrics"] and "vmaf" in got["metrics"]
    assert got["input"] == {"reference": "yuv420p", "distorted": "uyvy422", "planes_scored": "y", "packed_upload": True}


# ---- pqa_submit_packed's staging: halves that grow and alternate, a packed side larger than a slot, reset and mixing --------
GROW = [("uyvy422", 96, 18), ("v210", 52, 20)]   # with max_batch=2 a staging half holds two frames


def _grow_kw():
    from pqa2_amd import _native as N
    return dict(n_planes=3, chroma_shift=(1, 0), features=N.FEAT_ALL, max_batch=2)


_grow_cache = {}


def _grow_clip(fmt, w, h, t0=0):
    """eight 4:2:2 frames and their records, submitted one by one through pqa_submit: computed once, never written"""
    key = (fmt, w, h, t0)
    if key not in _grow_cache:
        refs, diss = _clip422(w, h, 8, PR.BIT_DEPTH[fmt], t0=t0)
        _grow_cache[key] = (refs, diss, _planar_records(w, h, PR.BIT_DEPTH[fmt], refs, diss, **_grow_kw()))
    return _grow_cache[key]


def _packed_side(fmt, clip, stride, seed):
    return [PR.pack(fmt, *f, stride=stride, seed=seed + i) for i, f in enumerate(clip)], fmt


def _planar_side(clip):
    return [[p.copy() for p in f] for f in clip], None


def _scribble(*sides):
    """the caller's arrays right after a call has returned: all of them overwritten"""
    for frames, fmt in sides:
        for f in frames:
            for a in ([f] if fmt else f):
                a[:] = 0x5A


@pytest.mark.parametrize("fmt,w,h", GROW)
@pytest.mark.parametrize("ref_packed", [False, True])
def test_submit_packed_halves_grow_and_alternate(fmt, w, h, ref_packed):
    """one frame reserves the smallest half; seven more run as chunks of 2, 2, 2, 1: both halves grow while the chunk before
    may still be read, and they alternate four times"""
    from pqa2_amd.engine import FeatureEngine
    refs, diss, planar = _grow_clip(fmt, w, h)
    row = PR.min_row_bytes(fmt, w)
    rstride, dstride = PR.file_stride(fmt, w) + 8, row + 4   # two different caller strides (v210: multiples of 4)
    side = lambda clip, f0, f1, stride, seed, packed: (_packed_side(fmt, clip[f0:f1], stride, seed) if packed
                                                       else _planar_side(clip[f0:f1]))
    with FeatureEngine(w, h, bit_depth=PR.BIT_DEPTH[fmt], **_grow_kw()) as eng:
        for f0, f1 in ((0, 1), (1, 8)):
            r, d = side(refs, f0, f1, rstride, 100, ref_packed), side(diss, f0, f1, dstride, 200, True)
            eng.submit_packed(f0, r, d)
            _scribble(r, d)
        assert np.array_equal(eng.collect(0, 8).view(np.uint64), planar.view(np.uint64))


def test_submit_packed_side_larger_than_a_planar_slot():
    """a luma-only context: a UYVY frame is two bytes a pixel against a slot of one"""
    from pqa2_amd.engine import FeatureEngine
    fmt, w, h, n = "uyvy422", 96, 18, 5
    refs, diss = _clip422(w, h, n, 8)
    kw = dict(n_planes=1, max_batch=2)
    planar = _planar_records(w, h, 8, [f[:1] for f in refs], [f[:1] for f in diss], **kw)
    with FeatureEngine(w, h, **kw) as eng:
        r, d = _planar_side([f[:1] for f in refs]), _packed_side(fmt, diss, PR.min_row_bytes(fmt, w) + 12, 7)
        eng.submit_packed(0, r, d)
        _scribble(r, d)
        assert np.array_equal(eng.collect(0, n).view(np.uint64), planar.view(np.uint64))


@pytest.mark.parametrize("fmt,w,h", GROW)
def test_submit_packed_after_pending_frames_and_after_reset(fmt, w, h):
    """pqa_submit leaves one frame pending when pqa_submit_packed enters; after pqa_reset the halves serve another clip"""
    from pqa2_amd.engine import FeatureEngine
    refs, diss, planar = _grow_clip(fmt, w, h)
    refs2, diss2, planar2 = _grow_clip(fmt, w, h, t0=5)
    row = PR.min_row_bytes(fmt, w)
    with FeatureEngine(w, h, bit_depth=PR.BIT_DEPTH[fmt], **_grow_kw()) as eng:
        for i in range(3):
            eng.submit(i, refs[i], diss[i])
        r, d = _planar_side(refs[3:6]), _packed_side(fmt, diss[3:6], row + 4, 300)
        eng.submit_packed(3, r, d)
        _scribble(r, d)
        eng.submit(6, refs[6], diss[6])
        assert np.array_equal(eng.collect(0, 7).view(np.uint64), planar[:7].view(np.uint64))
        eng.reset()
        r, d = _packed_side(fmt, refs2[:7], PR.file_stride(fmt, w) + 8, 400), _packed_side(fmt, diss2[:7], row + 4, 500)
        eng.submit_packed(0, r, d)
        _scribble(r, d)
        assert np.array_equal(eng.collect(0, 7).view(np.uint64), planar2[:7].view(np.uint64))
