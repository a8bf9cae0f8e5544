"""The host side of packed RGB captures without a GPU: the reader of headerless files (yuvio.RgbReader), open_video's dispatch,
and the way through score_files on a stand-in engine whose rgb_convert is the numpy restatement."""
import numpy as np
import pytest

from pqa2_amd import rgb, yuvio
from tests import rgb_ref as R


def _write(path, fmt, w, h, n, seed=0):
    rng = np.random.default_rng(seed)
    frames = [R.pack(fmt, *rng.integers(0, 1 << R.BIT_DEPTH[fmt], (3, h, w)), stride=R.file_stride(fmt, w), seed=seed + i) for i in range(n)]
    with open(path, "wb") as f:
        for fr in frames:
            f.write(fr.tobytes())
    return frames


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_reader_geometry_strides_and_frame_count(tmp_path, fmt):
    w, h, n = 70, 12, 3
    path = str(tmp_path / f"cap_{w}x{h}.{fmt}")
    frames = _write(path, fmt, w, h, n)
    rd = yuvio.open_video(path)
    assert isinstance(rd, yuvio.RgbReader) and len(rd) == n and rd.format == fmt
    info = rd.info
    assert (info.width, info.height, info.hshift, info.vshift, info.mono, info.packed, info.n_frames) == (w, h, 0, 0, False, fmt, n)
    assert info.bit_depth == (10 if fmt == "r210" else 8) and info.pix_fmt == fmt
    assert rd.row_stride == (512 if fmt == "r210" else 280)          # r210: 256 bytes per 64 pixels
    for i in range(n):
        got = rd.packed_frame(i)
        assert got.shape == (h, rd.row_stride) and np.array_equal(got, frames[i])
        for mine, want in zip(rgb.unpack_rgb(fmt, got, w), R.unpack(frames[i], fmt, w)):
            assert np.array_equal(mine, want)
    with pytest.raises(IndexError):
        rd.packed_frame(n)
    with pytest.raises(TypeError, match="_RgbReader"):
        rd.frame(0)


def test_reader_errors(tmp_path):
    w, h = 70, 12
    path = str(tmp_path / f"cap_{w}x{h}.r210")
    _write(path, "r210", w, h, 2)
    with open(path, "ab") as f:
        f.write(b"\0" * 7)
    with pytest.raises(ValueError, match=r"is not a whole number of r210 frames of 70x12 \(6144 bytes each, rows 512 bytes apart\)"):
        yuvio.open_video(path)
    empty = str(tmp_path / "empty_70x12.bgra")
    open(empty, "wb").close()
    with pytest.raises(ValueError, match="is not a whole number of bgra frames"):
        yuvio.open_video(empty)
    bare = str(tmp_path / "cap.bgra")
    _write(bare, "bgra", w, h, 1)
    with pytest.raises(ValueError, match="needs a geometry"):
        yuvio.open_video(bare)
    assert len(yuvio.open_video(bare, width=w, height=h)) == 1
    with pytest.raises(ValueError, match="bgra is 8 bit, not 10"):
        yuvio.open_video(bare, width=w, height=h, bit_depth=10)
    with pytest.raises(ValueError, match="not a packed RGB file"):
        yuvio.RgbReader(str(tmp_path / "cap_70x12.uyvy"))
    assert yuvio.RGB_EXTENSIONS == {".bgra", ".argb", ".rgba", ".abgr", ".r210"}


def _rgb_engine():
    from tests.fake_engine import OracleEngine

    class RgbEngine(OracleEngine):
        """the oracle stand-in with FeatureEngine.rgb_convert stated by the restatement; `calls` records every call"""
        calls = []

        def rgb_convert(self, frames, fmt, shape, dst, m, luma_only=False, generic=False):
            type(self).calls.append((len(frames), fmt, tuple(shape), tuple(dst), list(m)))
            return [R.convert(np.asarray(f), fmt, shape[1], shape[0], m, dst, luma_only=luma_only) for f in frames]
    RgbEngine.calls = []
    return RgbEngine


def test_score_files_on_a_stand_in_engine(tmp_path):
    from pqa2_amd import synth
    from pqa2_amd.pipeline import score_files
    w, h, n = 64, 48, 3
    refs, _ = synth.make_clip(w, h, n, 8, chroma=True)
    ref = str(tmp_path / "ref.y4m")
    master = yuvio.VideoInfo(w, h, 8, 1, 1, False, 30, 1, 0, "420mpeg2")
    yuvio.write_y4m(ref, refs, master)
    cap = str(tmp_path / f"cap_{w}x{h}.abgr")
    packed = _write(cap, "abgr", w, h, n, seed=9)
    E = _rgb_engine()
    make = lambda *a, **k: E(*a, **k)
    for kw, word in (({"rgb_matrix": "bt470"}, "rgb_matrix must be"), ({"rgb_range": "video"}, "rgb_range must be"),
                     ({"chroma_siting": "middle"}, "chroma_siting must be")):
        with pytest.raises(ValueError, match=word):
            score_files(ref, cap, engine_factory=make, **kw)
    assert E.calls == []
    got = score_files(ref, cap, engine_factory=make, psnr=True, ssim=False)       # chroma_mismatch stays "error": nothing to refuse
    m = rgb.conversion_matrix("bt601", 8, True, 8, False)
    assert E.calls == [(n, "abgr", (h, w), (1, 1, 0, 1, 8), m)]                    # one call for the run of frames
    assert got["input"] == {"reference": "yuv420p", "distorted": "abgr", "planes_scored": "yuv", "packed_upload": False,
                            "conversion": {"side": "distorted", "from": "abgr", "to": "yuv420p", "matrix": "bt601", "rgb_range": "full",
                                           "yuv_range": "limited", "bit_depth": [8, 8], "siting": {"to": [0, 1]}, "coefficients": m}}
    pre = str(tmp_path / "pre.y4m")
    yuvio.write_y4m(pre, [R.convert(p, "abgr", w, h, m, (1, 1, 0, 1, 8)) for p in packed], master)
    want = score_files(ref, pre, engine_factory=make, psnr=True, ssim=False)
    assert list(got["metrics"]) == list(want["metrics"]) and "psnr_cb" in got["metrics"]
    for k in want["metrics"]:
        assert np.array_equal(got["metrics"][k], want["metrics"][k]), k
    # a full-range master, the options, and the RGB clip on the reference side
    full = str(tmp_path / "full.y4m")
    yuvio.write_y4m(full, refs, yuvio.VideoInfo(w, h, 8, 1, 1, False, 30, 1, 0, "420jpeg", color_range="full"))
    E.calls.clear()
    res = score_files(cap, full, engine_factory=make, psnr=False, ssim=False, rgb_matrix="bt2020", rgb_range="limited")
    m2 = rgb.conversion_matrix("bt2020", 8, False, 8, True)
    assert E.calls == [(n, "abgr", (h, w), (1, 1, 1, 1, 8), m2)]
    conv = res["input"]["conversion"]
    assert (conv["side"], conv["matrix"], conv["rgb_range"], conv["yuv_range"], conv["siting"]) == ("reference", "bt2020", "limited", "full", {"to": [1, 1]})
    # a 12-bit partner is refused in words
    deep = str(tmp_path / "deep.y4m")
    yuvio.write_y4m(deep, [[p.astype(np.uint16) * 16 for p in f] for f in refs], yuvio.VideoInfo(w, h, 12, 1, 1, False, 30, 1, 0, "420p12"))
    with pytest.raises(ValueError, match="8 or 10 bit, not to the 12-bit"):
        score_files(deep, cap, engine_factory=make)
    # two RGB clips: both to 4:4:4 at the reference's depth
    cap10 = str(tmp_path / f"cap_{w}x{h}.r210")
    _write(cap10, "r210", w, h, n, seed=11)
    E.calls.clear()
    res = score_files(cap10, cap, engine_factory=make, psnr=True, ssim=False)
    assert [(c[1], c[3]) for c in E.calls] == [("r210", (0, 0, 0, 0, 10)), ("abgr", (0, 0, 0, 0, 10))]
    assert [c["to"] for c in res["input"]["conversion"]] == ["yuv444p10le", "yuv444p10le"]
    assert E.calls[0][4] == rgb.conversion_matrix("bt601", 10, False, 10, False) and E.calls[1][4] == rgb.conversion_matrix("bt601", 8, True, 10, False)
