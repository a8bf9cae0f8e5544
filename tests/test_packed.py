"""Packed capture formats without a GPU: the numpy restatement round-trips (tests/packed_ref.py), the reader of headerless
packed files (pqa2_amd/yuvio.PackedReader) against it, and score_files' chroma_mismatch option through tests/fake_engine.py.
The kernel and the entries: tests/test_gpu_packed.py."""
import os

import numpy as np
import pytest

from tests import packed_ref as PR

SHAPES = [(16, 16), (17, 16), (19, 17), (48, 16), (50, 16), (52, 20), (96, 18)]


@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("fmt", PR.FORMATS)
def test_pack_unpack_round_trip(fmt, w, h):
    y, u, v = PR.random_planes(fmt, w, h, seed=w * 100 + h)
    top = (1 << PR.BIT_DEPTH[fmt]) - 1
    assert y.min() == 0 and y.max() == top and u.max() == top and v.min() == 0      # the sample extremes are in
    for stride in (None, PR.file_stride(fmt, w), PR.min_row_bytes(fmt, w) + 20):
        packed = PR.pack(fmt, y, u, v, stride=stride)
        assert packed.dtype == np.uint8 and packed.shape == (h, stride or PR.min_row_bytes(fmt, w))
        for got, want in zip(PR.unpack(fmt, packed, w), (y, u, v)):
            assert got.dtype == PR.DTYPE[fmt] and np.array_equal(got, want)


@pytest.mark.parametrize("fmt", PR.FORMATS)
def test_padding_and_undefined_bits_change_nothing(fmt):
    w, h = 50, 16     # odd chroma width 25; the last v210 group holds 2 of 6 pixels
    planes = PR.random_planes(fmt, w, h, seed=5)
    a = PR.pack(fmt, *planes, stride=PR.min_row_bytes(fmt, w) + 12, seed=1, ones=True)
    b = PR.pack(fmt, *planes, stride=PR.min_row_bytes(fmt, w) + 12, seed=9, ones=False)
    assert not np.array_equal(a, b)                                   # the junk differs ...
    assert np.all(a[:, PR.min_row_bytes(fmt, w):] != 0)               # ... and is never zero
    for pa, pb, want in zip(PR.unpack(fmt, a, w), PR.unpack(fmt, b, w), planes):
        assert np.array_equal(pa, want) and np.array_equal(pb, want)
    if fmt == "v210":
        wa = np.ascontiguousarray(a[:, :PR.min_row_bytes(fmt, w)]).view("<u4")
        assert np.all(wa >> 30 == 3)


def test_v210_literal():
    """the twelve components of one group numbered 1 ... 12 in memory order"""
    y = np.array([[2, 4, 6, 8, 10, 12]], np.uint16)
    u = np.array([[1, 5, 9]], np.uint16)
    v = np.array([[3, 7, 11]], np.uint16)
    words = PR.pack("v210", y, u, v).view("<u4")[0] & 0x3FFFFFFF
    assert [int(x) for x in words] == [0x00300801, 0x00601404, 0x00902007, 0x00C02C0A]
    raw = np.array([0x00300801, 0x00601404, 0x00902007, 0x00C02C0A], "<u4").view(np.uint8).reshape(1, 16)
    for got, want in zip(PR.unpack("v210", raw, 6), (y, u, v)):
        assert np.array_equal(got, want)
    from pqa2_amd import yuvio
    for got, want in zip(yuvio.unpack_packed("v210", raw | np.uint8(0), 6), (y, u, v)):
        assert np.array_equal(got, want)


def test_stride_formulas():
    from pqa2_amd import yuvio
    for w, row8, row10, file10 in ((16, 32, 48, 128), (17, 36, 48, 128), (19, 40, 64, 128), (48, 96, 128, 128), (50, 100, 144, 256),
                                   (52, 104, 144, 256), (96, 192, 256, 256), (1920, 3840, 5120, 5120), (1280, 2560, 3424, 3456)):
        for fmt in ("uyvy422", "yuyv422"):
            assert PR.min_row_bytes(fmt, w) == PR.file_stride(fmt, w) == row8
            assert yuvio.packed_row_bytes(fmt, w) == yuvio.packed_file_stride(fmt, w) == row8
        assert PR.min_row_bytes("v210", w) == yuvio.packed_row_bytes("v210", w) == row10
        assert PR.file_stride("v210", w) == yuvio.packed_file_stride("v210", w) == file10


def _write(path, fmt, clip, w):
    with open(path, "wb") as f:
        for i, planes in enumerate(clip):
            f.write(PR.pack(fmt, *planes, stride=PR.file_stride(fmt, w), seed=i, ones=False).tobytes())


@pytest.mark.parametrize("fmt,ext", [("uyvy422", ".uyvy"), ("yuyv422", ".yuyv"), ("yuyv422", ".yuy2"), ("v210", ".v210")])
def test_packed_reader(tmp_path, fmt, ext):
    from pqa2_amd import yuvio
    w, h, n = 50, 16, 3
    clip = [PR.random_planes(fmt, w, h, seed=i) for i in range(n)]
    path = str(tmp_path / f"cap_{w}x{h}{ext}")
    _write(path, fmt, clip, w)
    rd = yuvio.open_video(path)                                # dispatch on the extension, geometry from the name
    assert isinstance(rd, yuvio.PackedReader) and len(rd) == n
    i = rd.info
    assert (i.width, i.height, i.bit_depth, i.hshift, i.vshift, i.mono, i.n_frames) == (w, h, PR.BIT_DEPTH[fmt], 1, 0, False, n)
    assert i.pix_fmt == fmt == i.packed and i.plane_shapes == [(h, w), (h, 25), (h, 25)]
    raw = np.fromfile(path, np.uint8)
    stride = PR.file_stride(fmt, w)
    for k in range(n):
        for got, want in zip(rd.frame(k), clip[k]):
            assert got.dtype == PR.DTYPE[fmt] and np.array_equal(got, want)
        pf = rd.packed_frame(k)
        assert pf.shape == (h, stride) and pf.base is not None and not pf.flags.owndata     # a view of the mapped file
        assert np.array_equal(pf.reshape(-1), raw[k * h * stride:(k + 1) * h * stride])
        assert np.shares_memory(pf, rd._mm)
    assert [len(f) for f in rd] == [3] * n
    # geometry from arguments where the name has none; the wrong depth is refused
    bare = str(tmp_path / f"capture{ext}")
    os.replace(path, bare)
    with pytest.raises(ValueError, match="geometry"):
        yuvio.open_video(bare)
    assert len(yuvio.open_video(bare, width=w, height=h)) == n
    with pytest.raises(ValueError, match="bit"):
        yuvio.PackedReader(bare, width=w, height=h, bit_depth=12)
    # a ragged tail is an error that names the sizes
    with open(bare, "ab") as f:
        f.write(b"\x01" * 7)
    with pytest.raises(ValueError) as e:
        yuvio.open_video(bare, width=w, height=h)
    assert str(n * h * stride + 7) in str(e.value) and str(h * stride) in str(e.value)


def test_metadata_reports_the_packed_pix_fmt(tmp_path):
    from pqa2_amd.vmaf_analyzer import VMAFAnalyzer
    w, h = 48, 16
    path = str(tmp_path / f"cap_{w}x{h}.v210")
    _write(path, "v210", [PR.random_planes("v210", w, h, seed=1)] * 2, w)
    an = VMAFAnalyzer()
    assert an.chroma_mismatch == "error"
    md = an.get_video_metadata(path)
    assert md["pix_fmt"] == "v210" and (md["width"], md["height"], md["nb_frames"]) == (w, h, 2)


def _y4m(path, clip, w, h, tag, hshift, vshift, mono=False, bpc=8):
    from pqa2_amd import yuvio
    yuvio.write_y4m(path, clip, yuvio.VideoInfo(w, h, bpc, hshift, vshift, mono, 30, 1, 0, tag))


def test_score_files_chroma_mismatch_option(tmp_path):
    """through the oracle stand-in (no submit_packed: the reader's numpy unpack feeds it)"""
    from pqa2_amd import synth
    from pqa2_amd.pipeline import score_files
    from tests.fake_engine import OracleEngine
    w, h, n = 64, 48, 2
    refs, diss = synth.make_clip(w, h, n, 8, chroma=True)
    ref = str(tmp_path / "ref.y4m")
    _y4m(ref, refs, w, h, "420jpeg", 1, 1)
    d422 = [[f[0]] + [np.ascontiguousarray(np.repeat(p, 2, axis=0)[:h]) for p in f[1:]] for f in diss]
    cap = str(tmp_path / f"cap_{w}x{h}.uyvy")
    _write(cap, "uyvy422", d422, w)
    make = lambda *a, **k: OracleEngine(*a, **k)
    with pytest.raises(ValueError, match='chroma_mismatch must be "error" or "luma"'):
        score_files(ref, cap, engine_factory=make, chroma_mismatch="chroma")
    with pytest.raises(ValueError, match="reference and distorted clips differ in pixel format"):
        score_files(ref, cap, engine_factory=make)
    with pytest.raises(ValueError, match="reference and distorted clips differ in pixel format"):
        score_files(ref, cap, engine_factory=make, chroma_mismatch="error")
    got = score_files(ref, cap, engine_factory=make, chroma_mismatch="luma", psnr=False, ssim=False)
    mref, mdis = str(tmp_path / "mref.y4m"), str(tmp_path / "mdis.y4m")
    _y4m(mref, [f[:1] for f in refs], w, h, "mono", 0, 0, True)
    _y4m(mdis, [f[:1] for f in diss], w, h, "mono", 0, 0, True)
    want = score_files(mref, mdis, engine_factory=make, psnr=False, ssim=False)
    assert "input" not in want
    assert list(got["metrics"]) == list(want["metrics"])
    for k in want["metrics"]:
        assert np.array_equal(got["metrics"][k], want["metrics"][k]), k
    assert got["input"] == {"reference": "yuv420p", "distorted": "uyvy422", "planes_scored": "y", "packed_upload": False}
    # a bit-depth difference stays an error under "luma"
    r10, d10 = synth.make_clip(w, h, n, 10, chroma=True)
    ref10 = str(tmp_path / "ref10.y4m")
    _y4m(ref10, r10, w, h, "420p10", 1, 1, bpc=10)
    with pytest.raises(ValueError, match="reference and distorted clips differ in pixel format"):
        score_files(ref10, cap, engine_factory=make, chroma_mismatch="luma")
