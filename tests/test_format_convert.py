"""The premises of the pixel-format conversion (include/pqa_vmaf.h, pqa_format_convert), on the numpy restatement
tests/format_convert_ref.py, and its way through yuvio, score_files (on a stand-in engine), the CLI and VMAFAnalyzer.
No GPU: tests/test_gpu_format_convert.py holds the kernel against the same restatement."""
import io
import itertools
import os

import numpy as np
import pytest

from tests import format_convert_ref as FR

SHIFTS = (0, 1, 2)
SITES = (FR.COSITED, FR.CENTRE)


def test_weights_sum_to_a_power_of_two():
    for ss, ds, s_site, d_site in itertools.product(SHIFTS, SHIFTS, SITES, SITES):
        want = 2 * max(1 << ss, 1 << ds) ** 2 // (1 << ss)
        assert want == FR.weight_sum(ss, ds) and want & (want - 1) == 0 and want <= 32
        for luma in (1, 2, 3, 5, 13, 64):
            rows = FR.taps(luma, ss, ds, s_site, d_site)
            assert len(rows) == FR.plane_size(luma, ds)
            for row in rows:
                assert sum(w for _, w in row) == want, (ss, ds, s_site, d_site, luma)
                assert 1 <= len(row) <= 8
                assert [j for j, _ in row] == list(range(row[0][0], row[0][0] + len(row)))   # consecutive candidates
            m = FR.axis_matrix(luma, ss, ds, s_site, d_site)
            assert (m.sum(axis=1) == want).all()


def test_example_tap_sets():
    # 4:2:2 -> 4:2:0 vertically, centred: [1 3 3 1] / 8 at rows 2i - 1 ... 2i + 2
    for i, row in enumerate(FR.taps(64, 0, 1, FR.COSITED, FR.CENTRE)):
        assert row == [(2 * i - 1, 1), (2 * i, 3), (2 * i + 1, 3), (2 * i + 2, 1)]
    # ... co-sited: [1 2 1] / 4 (as [2 4 2] / 8)
    for i, row in enumerate(FR.taps(64, 0, 1, FR.COSITED, FR.COSITED)):
        assert row == [(2 * i - 1, 2), (2 * i, 4), (2 * i + 1, 2)]
    # 4:2:0 centred -> 4:2:2: [1 3] / 4 and [3 1] / 4 alternating
    rows = FR.taps(64, 1, 0, FR.CENTRE, FR.COSITED)
    for k in range(32):
        assert rows[2 * k] == [(k - 1, 1), (k, 3)] and rows[2 * k + 1] == [(k, 3), (k + 1, 1)]
    # identity: [2] / 2 (a plane of shift s: one tap that carries the whole sum 2 F)
    for s, site in itertools.product(SHIFTS, SITES):
        assert FR.taps(13, s, s, site, site) == [[(i, 2 << s)] for i in range(FR.plane_size(13, s))]


def test_identity_returns_the_source():
    rng = np.random.default_rng(1)
    for hs, vs, site, bits in itertools.product(SHIFTS, SHIFTS, SITES, (8, 10, 12)):
        shape = (FR.plane_size(11, vs), FR.plane_size(13, hs))
        p = rng.integers(0, 1 << bits, shape).astype(np.uint8 if bits == 8 else np.uint16)
        lay = (hs, vs, site, site, bits)
        assert np.array_equal(FR.convert(p, (11, 13), lay, lay), p)
    # siting is void where the shift is 0
    p = rng.integers(0, 256, (11, 13)).astype(np.uint8)
    assert np.array_equal(FR.convert(p, (11, 13), (0, 0, 0, 0, 8), (0, 0, 1, 1, 8)), p)


@pytest.mark.parametrize("sbits,dbits", list(itertools.product((8, 10, 12), repeat=2)))
def test_constant_plane_and_extremes(sbits, dbits):
    d, top = dbits - sbits, (1 << dbits) - 1
    for c in (0, 1, 77, (1 << sbits) - 2, (1 << sbits) - 1):
        want = c << d if d >= 0 else min((c + (1 << (-d - 1))) >> -d, top)
        for src, dst in (((1, 0, 0, 0), (1, 1, 0, 1)), ((1, 1, 1, 1), (0, 0, 0, 0)), ((0, 0, 0, 0), (2, 2, 1, 0)), ((0, 0, 0, 0), (0, 0, 0, 0))):
            shape = (FR.plane_size(7, src[1]), FR.plane_size(9, src[0]))
            p = np.full(shape, c, np.uint8 if sbits == 8 else np.uint16)
            out = FR.convert(p, (7, 9), src + (sbits,), dst + (dbits,))
            assert out.dtype == (np.uint8 if dbits == 8 else np.uint16) and (out == want).all(), (c, src, dst)
    if sbits > 8:   # a container value above the depth's maximum is read as the maximum
        p = np.full((7, 9), 0xFFFF, np.uint16)
        want = ((1 << sbits) - 1) << d if d >= 0 else min(((1 << sbits) - 1 + (1 << (-d - 1))) >> -d, top)
        assert (FR.convert(p, (7, 9), (0, 0, 0, 0, sbits), (0, 0, 0, 0, dbits)) == want).all()
        assert (FR.convert(p, (7, 9), (0, 0, 0, 0, sbits), (1, 1, 1, 1, dbits)) == want).all()


def test_ten_bit_white_is_eight_bit_white():
    p = np.array([[1023, 1022, 1021, 1020, 2, 1, 0]], np.uint16)
    assert FR.convert(p, (1, 7), (0, 0, 0, 0, 10), (0, 0, 0, 0, 8)).tolist() == [[255, 255, 255, 255, 1, 0, 0]]


def _interior(luma, ss, ds, s_site, d_site):
    n_src = FR.plane_size(luma, ss)
    return [i for i, row in enumerate(FR.taps(luma, ss, ds, s_site, d_site)) if row[0][0] >= 0 and row[-1][0] <= n_src - 1]


def test_a_linear_plane_stays_linear_in_the_interior():
    """v = 2 Px + 3 Py + 10 with P the position in half luma samples: every siting offset, in the wrong direction or of the
    wrong size, would show.  The triangle reproduces a linear function exactly, so nothing is rounded."""
    lh, lw = 20, 24
    checked = 0
    for (shs, svs), (dhs, dvs), s_site, d_site in itertools.product(itertools.product(SHIFTS, SHIFTS), itertools.product(SHIFTS, SHIFTS),
                                                                    SITES, SITES):
        px = np.array([FR.position(k, shs, s_site) for k in range(FR.plane_size(lw, shs))])
        py = np.array([FR.position(k, svs, s_site) for k in range(FR.plane_size(lh, svs))])
        src = (2 * px[None, :] + 3 * py[:, None] + 10).astype(np.uint8)
        out = FR.convert(src, (lh, lw), (shs, svs, s_site, s_site, 8), (dhs, dvs, d_site, d_site, 8))
        ix, iy = _interior(lw, shs, dhs, s_site, d_site), _interior(lh, svs, dvs, s_site, d_site)
        assert ix and iy
        qx = np.array([FR.position(k, dhs, d_site) for k in ix])
        qy = np.array([FR.position(k, dvs, d_site) for k in iy])
        assert np.array_equal(out[np.ix_(iy, ix)], 2 * qx[None, :] + 3 * qy[:, None] + 10), ((shs, svs), (dhs, dvs), s_site, d_site)
        checked += 1
    assert checked == 81 * 4


def test_round_trip_stays_within_the_bound_of_the_taps():
    """4:2:0 -> 4:2:2 -> 4:2:0 (vertically centred).  The bound comes from the taps: with U the up and D the down matrix (sums
    Su, Sd) the exact round trip is D U c / (Sd Su); the first rounding is off by at most 1/2, D's weights carry that with
    sum 1, the second rounding adds 1/2: |out - D U c / (Sd Su)| <= 1.  D U is [3 10 3] / 16 in the interior, so on a smooth
    plane the round trip moves a sample by at most 3/16 of its second difference, plus 1."""
    lh, lw = 48, 32
    a420, a422 = (1, 1, 0, 1, 8), (1, 0, 0, 0, 8)
    y, x = np.mgrid[0:lh // 2, 0:lw // 2]
    c = np.rint(128 + 90 * np.sin(y / 5.0) * np.cos(x / 7.0)).astype(np.uint8)
    up = FR.convert(c, (lh, lw), a420, a422)
    back = FR.convert(up, (lh, lw), a422, a420)
    U, D = FR.axis_matrix(lh, 1, 0, FR.CENTRE, FR.COSITED), FR.axis_matrix(lh, 0, 1, FR.COSITED, FR.CENTRE)
    su, sd = FR.weight_sum(1, 0), FR.weight_sum(0, 1)
    M = D @ U
    assert (M[5, 4:7] * 16 == np.array([3, 10, 3]) * su * sd).all() and M[5].sum() == su * sd
    exact = M @ c.astype(np.int64)                       # times su * sd
    assert (np.abs(back.astype(np.int64) * su * sd - exact) <= su * sd).all()
    d2 = np.abs(c[:-2].astype(np.int64) - 2 * c[1:-1] + c[2:])
    assert (16 * np.abs(back[1:-1].astype(np.int64) - c[1:-1]) <= 3 * d2 + 16).all()


def test_video_info_chroma_siting():
    from pqa2_amd import yuvio
    want = {"420jpeg": (1, 1), "420mpeg2": (0, 1), "420": (0, 1), "420paldv": (0, 0), "420p10": (0, 1), "420p12": (0, 1),
            "420p16": (0, 1), "422": (0, 0), "422p10": (0, 0), "422p12": (0, 0), "422p16": (0, 0), "444": (0, 0), "444p10": (0, 0),
            "444p12": (0, 0), "444p16": (0, 0), "mono": (0, 0), "mono10": (0, 0), "mono12": (0, 0), "mono16": (0, 0)}
    assert set(want) == set(yuvio._Y4M_CHROMA)
    for tag, (hs, vs, bits, mono) in yuvio._Y4M_CHROMA.items():
        assert yuvio.VideoInfo(64, 48, bits, hs, vs, mono, chroma_tag=tag).chroma_siting == want[tag], tag
    for fmt, bits in (("uyvy422", 8), ("yuyv422", 8), ("v210", 10)):
        assert yuvio.VideoInfo(64, 48, bits, 1, 0, False, chroma_tag="422" if bits == 8 else "422p10", packed=fmt).chroma_siting == (0, 0)


# ---- score_files on a stand-in engine ------------------------------------------------------------------------------------

def _convert_engine():
    from tests.fake_engine import OracleEngine

    class ConvertEngine(OracleEngine):
        """the oracle stand-in with FeatureEngine.format_convert stated by the restatement; `calls` records every call"""
        calls = []

        def format_convert(self, frames, luma_shape, src, dst, generic=False):
            type(self).calls.append((len(frames), tuple(luma_shape), tuple(src), tuple(dst)))
            return [FR.convert(np.asarray(f), luma_shape, src, dst) for f in frames]
    ConvertEngine.calls = []
    return ConvertEngine


def _clips(tmp_path, w=64, h=48, n=3):
    from pqa2_amd import synth, yuvio
    from tests import packed_ref as PR
    refs, diss = synth.make_clip(w, h, n, 8, chroma=True)
    ref = str(tmp_path / "ref.y4m")
    yuvio.write_y4m(ref, refs, yuvio.VideoInfo(w, h, 8, 1, 1, False, 30, 1, 0, "420mpeg2"))
    rng = np.random.default_rng(5)
    d422 = [[f[0]] + [np.clip(np.repeat(p, 2, axis=0)[:h].astype(np.int64) + rng.integers(-3, 4, (h, p.shape[1])), 0, 255).astype(np.uint8)
                      for p in f[1:]] for f in diss]
    cap = str(tmp_path / f"cap_{w}x{h}.uyvy")
    with open(cap, "wb") as f:
        for fr in d422:
            f.write(PR.pack("uyvy422", *fr, stride=yuvio.packed_file_stride("uyvy422", w)).tobytes())
    return ref, cap, refs, d422


def test_score_files_convert_on_a_stand_in_engine(tmp_path):
    from pqa2_amd import yuvio
    from pqa2_amd.pipeline import score_files
    w, h, n = 64, 48, 3
    ref, cap, refs, d422 = _clips(tmp_path, w, h, n)
    E = _convert_engine()
    make = lambda *a, **k: E(*a, **k)
    with pytest.raises(ValueError, match="reference and distorted clips differ in pixel format"):
        score_files(ref, cap, engine_factory=make, chroma_mismatch="error")
    assert E.calls == []
    got_luma = score_files(ref, cap, engine_factory=make, chroma_mismatch="luma", psnr=False, ssim=False)
    assert E.calls == [] and got_luma["input"]["planes_scored"] == "y" and "conversion" not in got_luma["input"]
    got = score_files(ref, cap, engine_factory=make, chroma_mismatch="convert", psnr=True, ssim=True)
    src, dst = (1, 0, 0, 0, 8), (1, 1, 0, 1, 8)
    assert E.calls == [(2 * n, (h, w), src, dst)]          # the distorted side only: U and V of its n frames in one call, no luma call
    assert got["input"] == {"reference": "yuv420p", "distorted": "uyvy422", "planes_scored": "yuv", "packed_upload": False,
                            "conversion": {"side": "distorted", "from": "uyvy422", "to": "yuv420p", "bit_depth": [8, 8],
                                           "siting": {"from": [0, 0], "to": [0, 1]}}}
    pre = str(tmp_path / "pre.y4m")
    yuvio.write_y4m(pre, [FR.convert_frame(f, src, dst, (h, w)) for f in d422], yuvio.VideoInfo(w, h, 8, 1, 1, False, 30, 1, 0, "420mpeg2"))
    want = score_files(ref, pre, engine_factory=make, psnr=True, ssim=True)
    assert list(got["metrics"]) == list(want["metrics"]) and "psnr_cb" in got["metrics"] and "psnr_cr" in got["metrics"]
    for k in want["metrics"]:
        assert np.array_equal(got["metrics"][k], want["metrics"][k]), k
    # chroma_siting overrides both clips' siting on their subsampled axes
    E.calls.clear()
    res = score_files(ref, cap, engine_factory=make, chroma_mismatch="convert", chroma_siting="center", psnr=False, ssim=False)
    assert E.calls == [(2 * n, (h, w), (1, 0, 1, 0, 8), (1, 1, 1, 1, 8))]
    assert res["input"]["conversion"]["siting"] == {"from": [1, 0], "to": [1, 1]}
    with pytest.raises(ValueError, match="chroma_siting must be"):
        score_files(ref, cap, engine_factory=make, chroma_mismatch="convert", chroma_siting="middle")
    with pytest.raises(ValueError, match="chroma_mismatch must be"):
        score_files(ref, cap, engine_factory=make, chroma_mismatch="swscale")
    # clips of one pixel format are not wrapped
    E.calls.clear()
    same = score_files(ref, pre, engine_factory=make, chroma_mismatch="convert", psnr=False, ssim=False)
    assert E.calls == [] and "input" not in same
    # a monochrome clip against a colour clip stays an error
    mono = str(tmp_path / "mono.y4m")
    yuvio.write_y4m(mono, [f[:1] for f in refs], yuvio.VideoInfo(w, h, 8, 0, 0, True, 30, 1, 0, "mono"))
    with pytest.raises(ValueError, match="reference and distorted clips differ in pixel format"):
        score_files(mono, cap, engine_factory=make, chroma_mismatch="convert")
    assert E.calls == []


def test_score_files_convert_carries_the_bit_depth(tmp_path):
    """a 10-bit 4:2:2 clip against the 8-bit 4:2:0 master: the luma goes through a depth-only call, the chroma through one call"""
    from pqa2_amd import yuvio
    from pqa2_amd.pipeline import score_files
    w, h, n = 64, 48, 2
    ref, _, _, d422 = _clips(tmp_path, w, h, n)
    d10 = [[(p.astype(np.uint16) << 2) | 1 for p in f] for f in d422]
    cap10 = str(tmp_path / "cap10.y4m")
    yuvio.write_y4m(cap10, d10, yuvio.VideoInfo(w, h, 10, 1, 0, False, 30, 1, 0, "422p10"))
    E = _convert_engine()
    got = score_files(ref, cap10, engine_factory=lambda *a, **k: E(*a, **k), chroma_mismatch="convert", psnr=True, ssim=False)
    assert E.calls == [(n, (h, w), (0, 0, 0, 0, 10), (0, 0, 0, 0, 8)), (2 * n, (h, w), (1, 0, 0, 0, 10), (1, 1, 0, 1, 8))]
    assert got["input"]["conversion"]["bit_depth"] == [10, 8] and got["input"]["conversion"]["from"] == "yuv422p10le"
    assert got["input"]["conversion"]["to"] == "yuv420p"


# ---- the CLI and VMAFAnalyzer hand the two options through --------------------------------------------------------------------

def test_cli_hands_the_options_through(tmp_path, monkeypatch):
    from pqa2_amd import pipeline, score
    seen = []

    def fake(*args, **kw):
        seen.append(kw)
        raise RuntimeError("stop here")
    monkeypatch.setattr(pipeline, "score_files", fake)
    js = str(tmp_path / "o.json")
    assert score.main(["a.y4m", "b.y4m", "--json", js]) == 1
    assert score.main(["a.y4m", "b.y4m", "--json", js, "--chroma-mismatch", "convert", "--chroma-siting", "topleft"]) == 1
    assert "chroma_mismatch" not in seen[0] and "chroma_siting" not in seen[0]
    assert seen[1]["chroma_mismatch"] == "convert" and seen[1]["chroma_siting"] == "topleft"
    with pytest.raises(SystemExit):
        score.main(["a.y4m", "b.y4m", "--json", js, "--chroma-siting", "middle"])


def test_analyzer_hands_the_options_through(tmp_path, monkeypatch):
    from pqa2_amd import vmaf_analyzer as V
    ref, cap, _, _ = _clips(tmp_path)
    a = V.VMAFAnalyzer()
    assert a.chroma_mismatch == "error" and a.chroma_siting is None
    kw = a._ssim_family_kwargs()
    assert "chroma_mismatch" not in kw and "chroma_siting" not in kw
    a.chroma_mismatch, a.chroma_siting = "convert", "left"
    kw = a._ssim_family_kwargs()
    assert kw["chroma_mismatch"] == "convert" and kw["chroma_siting"] == "left"
    cmds = []

    class FakePopen:
        def __init__(self, cmd, **kw):
            cmds.append(cmd)
            self.stderr = io.StringIO("")
            self.pid = os.getpid()

        def wait(self, timeout=None):
            return 1

        def poll(self):
            return 1

    monkeypatch.setattr(V.subprocess, "Popen", FakePopen)
    b = V.VMAFAnalyzer()
    b.gpus = 2
    b._run_child_job(ref, cap, "vmaf_v0.6.1", "j.json", None, None, 3)
    b.chroma_mismatch, b.chroma_siting = "convert", "center"
    b._run_child_job(ref, cap, "vmaf_v0.6.1", "j.json", None, None, 3)
    for c in cmds:
        c[c.index("--master-port") + 1] = "PORT"
    extra = ["--chroma-mismatch", "convert", "--chroma-siting", "center"]
    assert "--chroma-mismatch" not in cmds[0] and "--chroma-siting" not in cmds[0]
    i = cmds[1].index("--chroma-mismatch")
    assert cmds[1][i:i + 4] == extra and cmds[1][:i] + cmds[1][i + 4:] == cmds[0]
