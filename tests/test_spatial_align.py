"""Spatial alignment on the host (no GPU): align.best_shift on constructed arrays -- the tie key, confidence with its 0 / 0
and x / 0 cases, at_edge, agreement, the parabola -- the numpy restatement against a per-pixel loop, the argument rules of
score_files(spatial_align=), and the crop arithmetic of the reader wrapper (4:2:0 with odd shifts included) through
tests/fake_engine.py: the records of a displaced pair equal those of the clips cut by hand."""
import numpy as np
import pytest

from tests import spatial_align_ref as R


def _S(R_, fill=100, n=1):
    return np.full((n, 2 * R_ + 1, 2 * R_ + 1), fill, np.uint64)


def test_restatement_against_a_pixel_loop():
    ref, dis = R.random_pair(5, 1, 9, 7)
    S = R.shift_sse(ref, dis, 2)
    for j in range(5):
        for i in range(5):
            want = sum((int(ref[0][y, x]) - int(dis[0][y + j - 2, x + i - 2])) ** 2 for y in range(2, 5) for x in range(2, 7))
            assert int(S[0, j, i]) == want
    moved = R.shift_plane(ref[0], 1, -2, np.random.default_rng(0), 255)
    assert moved[0, 1] == ref[0][2, 0] and R.shift_sse(ref, [moved], 2)[0, 0, 3] == 0    # dx = +1: right; dy = -2: up


def test_best_shift_minimum_and_fields():
    from pqa2_amd.align import best_shift
    S = _S(3, 1000, n=2)
    S[:, 3 + 1, 3 - 2] = 10        # (dx, dy) = (-2, +1)
    S[0, 0, 0] = 30
    b = best_shift(S, 3, n_pixels=5)
    assert (b["dx"], b["dy"], b["searched"], b["at_edge"]) == (-2, 1, 3, False)
    assert b["mse"] == 20 / (2 * 5) and b["agreement"] == 1.0
    assert b["confidence"] == (30 + 1000) / 20    # the smallest pooled value outside the 3 x 3 neighbourhood
    assert b["subpixel_dx"] == 0.0 and b["subpixel_dy"] == 0.0
    with pytest.raises(ValueError):
        best_shift(S, 2)
    with pytest.raises(ValueError):
        best_shift(S[0], 3)


def test_best_shift_tie_key():
    from pqa2_amd.align import best_shift
    flat = best_shift(_S(2), 2)         # everything ties: the zero shift
    assert (flat["dx"], flat["dy"], flat["confidence"]) == (0, 0, 1.0)
    S = _S(2)
    for dx, dy in ((1, 0), (0, 1), (-1, 0), (0, -1)):     # equal length: the smaller |dy|, then the smaller dx
        S[0, 2 + dy, 2 + dx] = 5
    assert (best_shift(S, 2)["dx"], best_shift(S, 2)["dy"]) == (-1, 0)
    S = _S(2)
    S[0, 2 + 1, 2] = S[0, 2 - 1, 2] = 5                   # |dy| ties: the negative dy
    assert (best_shift(S, 2)["dx"], best_shift(S, 2)["dy"]) == (0, -1)
    S = _S(2)
    S[0, 2 + 1, 2 + 1] = S[0, 2, 2 + 2] = 5               # the shorter shift wins over the smaller |dy|
    assert (best_shift(S, 2)["dx"], best_shift(S, 2)["dy"]) == (1, 1)
    S[0, 2, 2 + 2] = 4                                    # ... but not over a smaller error
    assert (best_shift(S, 2)["dx"], best_shift(S, 2)["dy"]) == (2, 0)


def test_best_shift_confidence_cases():
    from pqa2_amd.align import best_shift
    S = _S(3, 7)
    S[0, 3, 3] = 0
    assert best_shift(S, 3)["confidence"] == float("inf")                 # x / 0
    assert best_shift(_S(3, 0), 3)["confidence"] == 1.0                   # 0 / 0
    S = _S(3, 0)
    S[0, 2:5, 2:5] = 9
    S[0, 3, 3] = 0
    assert best_shift(S, 3)["confidence"] == 1.0                          # zeros outside the neighbourhood too
    S = _S(3, 50)
    S[0, 3, 3], S[0, 3, 4] = 10, 11                                       # a neighbour does not count
    assert best_shift(S, 3)["confidence"] == 5.0
    assert best_shift(_S(1, 3), 1)["confidence"] == 1.0                   # nothing outside the neighbourhood
    assert best_shift(_S(0, 3), 0) == {"dx": 0, "dy": 0, "mse": 3.0, "confidence": 1.0, "agreement": 1.0, "at_edge": True,
                                       "subpixel_dx": None, "subpixel_dy": None, "searched": 0}


def test_best_shift_edge_agreement_and_parabola():
    from pqa2_amd.align import best_shift
    S = _S(2, 100)
    S[0, 2, 4] = 1
    b = best_shift(S, 2)
    assert (b["dx"], b["dy"], b["at_edge"], b["subpixel_dx"], b["subpixel_dy"]) == (2, 0, True, None, None)
    S[0, 2, 4], S[0, 0, 1] = 100, 1
    assert best_shift(S, 2)["at_edge"] is True and best_shift(S, 2)["dy"] == -2
    S = _S(2, 100, n=4)
    S[0:3, 2, 3] = 10           # three frames say (1, 0)
    S[3, 1, 2] = 20             # one says (0, -1), and loses the pooled vote: 3 * 10 + 100 < 3 * 100 + 20
    b = best_shift(S, 2)
    assert (b["dx"], b["dy"], b["agreement"]) == (1, 0, 0.75)
    S = _S(3, 1000)
    S[0, 3, 2:5] = (40, 10, 20)      # along x: vertex at (40 - 20) / (2 (40 - 20 + 20)) = 0.25
    S[0, 2:5, 3] = (10, 10, 30)      # along y: (10 - 30) / (2 (10 - 20 + 30)) = -0.5
    b = best_shift(S, 3)
    assert (b["dx"], b["dy"]) == (0, 0) and b["subpixel_dx"] == 0.25 and b["subpixel_dy"] == -0.5
    S = _S(3, 10)
    S[0, 3, 3] = 10                  # flat: the three points have no minimum
    assert best_shift(S, 3)["subpixel_dx"] is None


def test_report_lines_and_analyzer_options():
    from pqa2_amd import report
    from pqa2_amd.vmaf_analyzer import VMAFAnalyzer
    sp = {"dx": 3, "dy": -1, "mse": 4.5, "confidence": float("inf"), "agreement": 1.0, "at_edge": False, "subpixel_dx": 0.0,
          "subpixel_dy": 0.0, "searched": 4, "frames": 8, "applied": True, "chroma_exact": False}
    line = report.spatial_summary_line(sp)
    assert "displaced by (+3, -1) px" in line and "exact match" in line and "chroma half a sample off" in line
    assert "not applied" in report.spatial_summary_line(dict(sp, at_edge=True, applied=False))
    keys = report.alignment_log_keys({"spatial": sp})
    assert keys["alignment"]["spatial"]["confidence"] is None and "confidence" not in keys["alignment"]
    both = report.alignment_log_keys({"offset_frames": 1, "confidence": float("inf"), "spatial": dict(sp, confidence=2.0)})
    assert both["alignment"]["confidence"] is None and both["alignment"]["spatial"]["confidence"] == 2.0
    an = VMAFAnalyzer()
    assert an.spatial_align_enabled is False and an.spatial_align_radius == 8
    an.set_advanced_options(spatial_align_enabled=True, spatial_align_radius=40)
    assert an.spatial_align_enabled and an.spatial_align_radius == 16
    assert an._ssim_family_kwargs()["spatial_align"] == 16


# ---- score_files: argument rules and the crop arithmetic --------------------------------------------------------------------
def _shift_engine():
    from tests.fake_engine import OracleEngine

    class ShiftEngine(OracleEngine):
        """the oracle stand-in plus the restated shifted-window SSE"""

        def shift_sse(self, ref_frames, dis_frames, radius):
            return R.shift_sse(ref_frames, dis_frames, radius)
    return ShiftEngine


def _info(w, h, mono):
    from pqa2_amd.yuvio import VideoInfo
    return VideoInfo(width=w, height=h, fps_num=24, fps_den=1, bit_depth=8, mono=mono, hshift=0 if mono else 1,
                     vshift=0 if mono else 1, chroma_tag="mono" if mono else "420")


def _write(tmp_path, dx, dy, cdx, cdy, mono, w=48, h=40, n=2):
    """a clip, its capture displaced by (dx, dy) in luma and (cdx, cdy) in chroma, and both cut by hand: the reference at
    (max(0, -dx), max(0, -dy)), the capture at that origin plus (dx, dy), chroma at origin >> 1 with the window's size"""
    from pqa2_amd.yuvio import write_y4m
    frames = R.natural_planes(51, n, w, h, 0 if mono else 1, 0 if mono else 1, mono)
    rng = np.random.default_rng(52)
    cap = [[R.shift_plane(pl, *((dx, dy) if p == 0 else (cdx, cdy)), rng, 255) for p, pl in enumerate(planes)] for planes in frames]
    wc, hc, x0, y0 = w - abs(dx), h - abs(dy), max(0, -dx), max(0, -dy)
    cw, ch = -(-wc >> 1), -(-hc >> 1)

    def cut(planes, ox, oy):
        return [planes[0][oy:oy + hc, ox:ox + wc]] + [c[oy >> 1:(oy >> 1) + ch, ox >> 1:(ox >> 1) + cw] for c in planes[1:]]
    paths = {}
    for key, clip, info in (("ref", frames, _info(w, h, mono)), ("dis", cap, _info(w, h, mono)),
                            ("ref_cut", [cut(f, x0, y0) for f in frames], _info(wc, hc, mono)),
                            ("dis_cut", [cut(f, x0 + dx, y0 + dy) for f in cap], _info(wc, hc, mono))):
        paths[key] = str(tmp_path / (key + ".y4m"))
        write_y4m(paths[key], clip, info)
    return paths


def test_score_files_argument_rules(tmp_path):
    from pqa2_amd.pipeline import score_files
    p = _write(tmp_path, 1, 0, 0, 0, True, w=32, h=24, n=1)
    kw = dict(psnr=False, ssim=False, engine_factory=_shift_engine())
    for bad in (-1, 17):
        with pytest.raises(ValueError, match="spatial_align must be"):
            score_files(p["ref"], p["dis"], None, spatial_align=bad, **kw)
    with pytest.raises(ValueError, match="spatial_frames"):
        score_files(p["ref"], p["dis"], None, spatial_align=2, spatial_frames=0, **kw)
    with pytest.raises(ValueError, match="larger than"):
        score_files(p["ref"], p["dis"], None, spatial_align=12, **kw)     # 24 rows are not more than 2 * 12
    assert "alignment" not in score_files(p["ref"], p["dis"], None, **kw)


def test_spatial_sample_and_crop_windows():
    from pqa2_amd.pipeline import _CroppedReader, crop_readers, spatial_sample
    assert spatial_sample(80, 8) == [5, 15, 25, 35, 45, 55, 65, 75]
    assert spatial_sample(3, 8) == [0, 1, 2] and spatial_sample(1, 8) == [0] and spatial_sample(0, 8) == []

    class Clip:
        def __init__(self, mono):
            self.info = _info(48, 40, mono)

        def __len__(self):
            return 5

        def frame(self, i):
            planes = [np.arange(40 * 48, dtype=np.uint8).reshape(40, 48)]
            return planes if self.info.mono else planes + [np.arange(20 * 24, dtype=np.uint8).reshape(20, 24)] * 2
    r, d = crop_readers(Clip(False), Clip(False), 3, -1)
    assert (r.info.width, r.info.height, r.info.chroma_w, r.info.chroma_h, len(r)) == (45, 39, 23, 20, 5)
    assert r.windows() == [(1, 0, 39, 45), (0, 0, 20, 23), (0, 0, 20, 23)]       # the reference starts one row down
    assert d.windows() == [(0, 3, 39, 45), (0, 1, 20, 23), (0, 1, 20, 23)]       # the capture three samples right
    fr, fd = r.frame(0), d.frame(0)
    assert [p.shape for p in fr] == [p.shape for p in fd] == [(39, 45), (20, 23), (20, 23)]
    assert fr[0][0, 0] == (1 * 48 + 0) % 256 and fd[0][0, 0] == 3 and fd[1][0, 0] == 1
    assert fr[0].base is not None       # a view: nothing was copied
    r, d = crop_readers(Clip(True), Clip(True), -2, 4)
    assert r.windows() == [(0, 2, 36, 46)] and d.windows() == [(4, 0, 36, 46)]
    with pytest.raises(ValueError):
        _CroppedReader(Clip(True), 4, 0, 46, 40)


@pytest.mark.parametrize("mono,dx,dy,cdx,cdy,exact", [(True, 3, -1, 0, 0, True), (False, 2, -2, 1, -1, True),
                                                      (False, 3, -1, 1, 0, False)])
def test_score_files_crops_like_by_hand(tmp_path, mono, dx, dy, cdx, cdy, exact):
    """the records of score_files(spatial_align=) on a displaced pair are those of the clips cut by hand; 4:2:0 with the odd
    shift (3, -1): chroma origins (0, 0) and (1, 0), window 45 x 39 -> 23 x 20 chroma samples, chroma_exact false"""
    from pqa2_amd.pipeline import score_files
    p = _write(tmp_path, dx, dy, cdx, cdy, mono)
    kw = dict(engine_factory=_shift_engine())
    res = score_files(p["ref"], p["dis"], "vmaf_v0.6.1", spatial_align=4, spatial_frames=2, **kw)
    sp = res["alignment"]["spatial"]
    assert (sp["dx"], sp["dy"], sp["applied"], sp["at_edge"], sp["chroma_exact"], sp["frames"], sp["searched"]) == \
           (dx, dy, True, False, exact, 2, 4)
    assert sp["mse"] == 0.0 and sp["confidence"] == float("inf") and sp["agreement"] == 1.0
    assert set(sp) == {"dx", "dy", "mse", "confidence", "agreement", "at_edge", "subpixel_dx", "subpixel_dy", "searched",
                       "frames", "applied", "chroma_exact"}
    by_hand = score_files(p["ref_cut"], p["dis_cut"], "vmaf_v0.6.1", **kw)
    assert res["records"].shape == by_hand["records"].shape
    assert np.array_equal(res["records"].view(np.uint64), by_hand["records"].view(np.uint64))
    assert res["psnr_lines"] == by_hand["psnr_lines"]
    if not mono and exact:     # the chroma planes line up exactly: their error is zero
        from pqa2_amd import _native as N
        assert not res["records"][:, N.REC_SSE:N.REC_SSE + 3].view(np.uint64).any()


def test_score_files_not_applied_is_the_plain_path(tmp_path):
    from pqa2_amd.pipeline import score_files
    p = _write(tmp_path, 4, 0, 0, 0, True)
    kw = dict(engine_factory=_shift_engine())
    edge = score_files(p["ref"], p["dis"], "vmaf_v0.6.1", spatial_align=4, spatial_frames=2, **kw)
    sp = edge["alignment"]["spatial"]
    assert (sp["dx"], sp["dy"], sp["at_edge"], sp["applied"]) == (4, 0, True, False)
    plain = score_files(p["ref"], p["dis"], "vmaf_v0.6.1", **kw)
    assert np.array_equal(edge["records"].view(np.uint64), plain["records"].view(np.uint64))
    same = score_files(p["ref"], p["ref"], "vmaf_v0.6.1", spatial_align=4, spatial_frames=2, **kw)
    sp = same["alignment"]["spatial"]
    assert (sp["dx"], sp["dy"], sp["applied"]) == (0, 0, False) and same["records"].shape == (2, 24)
