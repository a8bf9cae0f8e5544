"""The overlay step of score_files on the CPU: detection -> regions -> node grid on numpy tile sums, and the step itself through
an oracle stand-in that blends with tests/mask_ref.py.  The clips are synth.make_pair with a checkerboard burnt into the
captured luma (mask_ref.checker_logo)."""
import numpy as np
import pytest

from tests import mask_ref as MR


def _lumas(w, h, n, strength=1.0):
    from pqa2_amd import synth
    pairs = [synth.make_pair(w, h, t, 8, chroma=False, strength=strength) for t in range(n)]
    return [p[0][0] for p in pairs], [p[1][0] for p in pairs]


# ---- detection -> regions -> nodes, on numpy tile sums -------------------------------------------------------------------------
def test_logo_is_one_persistent_region_and_its_mask():
    from pqa2_amd import distortion as D
    w, h, n, T = 320, 180, 8, 16
    refs, clean = _lumas(w, h, n)
    logo = [MR.checker_logo(d) for d in clean]
    counts = D.tile_counts(w, h, T)
    found = {}
    for name, dis in (("clean", clean), ("logo", logo)):
        S = D.tile_sse(MR.tile_moments(refs, dis, T))
        hot = D.hot_tiles(S, counts, tile=T, bit_depth=8)
        found[name] = (D.persistent_regions(hot, S, counts, tile=T, bit_depth=8, width=w, height=h), D.persistent_tiles(hot, 0.9))
    assert found["clean"][0]["regions"] == [] and not found["clean"][1].any()
    regions, tiles = found["logo"][0]["regions"], found["logo"][1]
    assert len(regions) == 1 and regions[0]["box"] == [208, 112, 288, 160] and regions[0]["tiles"] == 15 and tiles.sum() == 15
    m = D.overlay_mask(tiles, w, h, T, grow=1, feather=16, node=8, chroma_shift=(1, 1))
    assert m["boxes"] == [[192, 96, 304, 176]] and m["step_log2"] == 3 and m["bounds"] == [177, 81, 320, 180]
    assert round(m["share"], 3) == 0.246
    a = MR.alpha(m["nodes"], w, h, 3, 3)
    x0, y0, x1, y1 = MR.LOGO_BOX
    assert (a[y0:y1, x0:x1] == 256).all() and (a[96:176, 192:304] == 256).all() and a[:81].max() == 0 and a[:, :177].max() == 0
    # nothing persistent: an empty mask, which the pipeline does not apply
    none = D.overlay_mask(found["clean"][1], w, h, T)
    assert not none["nodes"].any() and none["bounds"] is None and none["share"] == 0 and none["boxes"] == []


# ---- score_files through the oracle stand-in ---------------------------------------------------------------------------------
W, H, N_FRAMES = 96, 64, 4
BOX = (37, 19, 69, 35)


def _engine():
    from tests.fake_engine import OracleEngine

    class OverlayEngine(OracleEngine):
        """the oracle stand-in plus the restated tile moments and mask blend"""
        calls = []

        def __init__(self, width, height, **kw):
            super().__init__(width, height, **kw)
            self.bits = kw.get("bit_depth", 8)

        def tile_moments(self, ref_frames, dis_frames, tile=32):
            OverlayEngine.calls.append(("tile_moments", len(ref_frames), tile))
            return MR.tile_moments(ref_frames, dis_frames, tile)

        def mask_blend(self, frames, nodes, steps, fill, plane=0):
            OverlayEngine.calls.append(("mask_blend", len(frames), tuple(steps), plane, fill if isinstance(fill, int) else "planes"))
            return [MR.blend(np.asarray(f), nodes, *steps, fill if isinstance(fill, int) else np.asarray(fill[k]), self.bits)
                    for k, f in enumerate(frames)]
    return OverlayEngine


@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    from pqa2_amd import synth
    from pqa2_amd.yuvio import write_y4m
    d = tmp_path_factory.mktemp("overlay")
    info = synth.clip_info(W, H)
    refs, clean = synth.make_clip(W, H, N_FRAMES)
    logo = [[MR.checker_logo(f[0], BOX), f[1], f[2]] for f in clean]
    paths = {}
    for key, clip in (("ref", refs), ("clean", clean), ("logo", logo)):
        paths[key] = str(d / (key + ".y4m"))
        write_y4m(paths[key], clip, info)
    return paths


def _bits(res):
    return res["records"].view(np.uint64)


def _vmaf(res):
    return float(np.mean(res["metrics"]["vmaf"]))


def test_off_leaves_score_files_untouched(clips):
    from pqa2_amd.pipeline import score_files
    Eng = _engine()
    plain = score_files(clips["ref"], clips["logo"], "vmaf_v0.6.1", engine_factory=Eng)
    off = score_files(clips["ref"], clips["logo"], "vmaf_v0.6.1", engine_factory=Eng, overlay_mask=None, overlay_frames=3, overlay_tile=8,
                      overlay_grow=4, overlay_feather=64, overlay_share=0.5)
    assert not Eng.calls and "overlay" not in plain and "overlay" not in off and set(plain) == set(off)
    assert np.array_equal(_bits(plain), _bits(off)) and plain["metrics"].keys() == off["metrics"].keys()


def test_report_finds_and_applies_nothing(clips):
    from pqa2_amd.pipeline import score_files
    Eng = _engine()
    plain = score_files(clips["ref"], clips["logo"], "vmaf_v0.6.1", engine_factory=Eng)
    rep = score_files(clips["ref"], clips["logo"], "vmaf_v0.6.1", engine_factory=Eng, overlay_mask="report")
    ov = rep["overlay"]
    assert set(ov) == {"mode", "detected", "regions", "boxes", "share", "fill", "tile", "grow", "feather", "frames_sampled", "applied"}
    assert (ov["mode"], ov["detected"], ov["applied"], ov["tile"], ov["grow"], ov["feather"], ov["frames_sampled"]) == ("report", True, False, 16, 1, 16, N_FRAMES)
    assert len(ov["regions"]) == 1 and ov["regions"][0]["box"] == [32, 16, 80, 48] and ov["boxes"] == [[16, 0, 96, 64]]
    assert 0 < ov["share"] <= 1 and len(ov["fill"]) == 3 and ov["fill"][1:] == [128, 128] and 16 <= ov["fill"][0] <= 235
    assert Eng.calls == [("tile_moments", N_FRAMES, 16)] and np.array_equal(_bits(rep), _bits(plain))
    # the clean clip: no persistent tile, nothing applied under any mode
    Eng.calls.clear()
    none = score_files(clips["ref"], clips["clean"], "vmaf_v0.6.1", engine_factory=Eng, overlay_mask="neutral")
    assert none["overlay"]["regions"] == [] and none["overlay"]["boxes"] == [] and not none["overlay"]["applied"] and none["overlay"]["share"] == 0
    assert [c[0] for c in Eng.calls] == ["tile_moments"]


def test_neutral_with_a_box_makes_logo_and_clean_clip_equal(clips):
    """every logo sample has alpha = 256: both runs submit the same integers"""
    from pqa2_amd.pipeline import score_files
    Eng = _engine()
    kw = dict(engine_factory=Eng, overlay_mask="neutral", overlay_boxes=[[32, 16, 80, 40]])
    with_logo = score_files(clips["ref"], clips["logo"], "vmaf_v0.6.1", **kw)
    clean = score_files(clips["ref"], clips["clean"], "vmaf_v0.6.1", **kw)
    plain = score_files(clips["ref"], clips["logo"], "vmaf_v0.6.1", engine_factory=Eng)
    assert np.array_equal(_bits(with_logo), _bits(clean)) and not np.array_equal(_bits(with_logo), _bits(plain))
    ov = with_logo["overlay"]
    assert (ov["mode"], ov["detected"], ov["applied"], ov["regions"], ov["boxes"]) == ("neutral", False, True, [], [[32, 16, 80, 40]])
    assert ov == clean["overlay"] and not any(c[0] == "tile_moments" for c in Eng.calls)
    blends = [c for c in Eng.calls if c[0] == "mask_blend"]
    assert {c[2:4] for c in blends} == {((3, 3), 0), ((2, 2), 1), ((2, 2), 2)} and {c[4] for c in blends} == set(ov["fill"])
    detected = score_files(clips["ref"], clips["logo"], "vmaf_v0.6.1", engine_factory=Eng, overlay_mask="neutral")
    assert detected["overlay"]["applied"] and _vmaf(detected) > _vmaf(plain)


def test_reference_mode_blends_the_capture_towards_the_reference(clips):
    from pqa2_amd.pipeline import score_files
    Eng = _engine()
    same = score_files(clips["ref"], clips["ref"], "vmaf_v0.6.1", engine_factory=Eng)
    masked = score_files(clips["ref"], clips["ref"], "vmaf_v0.6.1", engine_factory=Eng, overlay_mask="reference",
                         overlay_boxes=[list(BOX)])
    assert masked["overlay"]["fill"] == "reference" and masked["overlay"]["applied"] and np.array_equal(_bits(masked), _bits(same))
    assert {c[4] for c in Eng.calls if c[0] == "mask_blend"} == {"planes"}
    plain = score_files(clips["ref"], clips["logo"], "vmaf_v0.6.1", engine_factory=Eng)
    fixed = score_files(clips["ref"], clips["logo"], "vmaf_v0.6.1", engine_factory=Eng, overlay_mask="reference")
    assert _vmaf(fixed) > _vmaf(plain)


def test_argument_errors(clips):
    from pqa2_amd.pipeline import score_files
    Eng = _engine()
    for kw in (dict(overlay_mask="blur"), dict(overlay_boxes=[[0, 0, 8, 8]]), dict(overlay_mask="report", overlay_frames=0),
               dict(overlay_mask="report", overlay_tile=12), dict(overlay_mask="report", overlay_grow=-1),
               dict(overlay_mask="report", overlay_feather=12), dict(overlay_mask="report", overlay_share=0),
               dict(overlay_mask="report", overlay_share=1.5), dict(overlay_mask="neutral", overlay_boxes=[[0, 0, 200, 8]]),
               dict(overlay_mask="neutral", overlay_boxes=[[8, 8, 8, 16]])):
        with pytest.raises(ValueError):
            score_files(clips["ref"], clips["logo"], "vmaf_v0.6.1", engine_factory=Eng, **kw)


def test_report_lines():
    from pqa2_amd import report
    ov = {"mode": "neutral", "detected": True, "regions": [{"box": [32, 16, 80, 48], "tiles": 6, "frames_hot_min": 4}],
          "boxes": [[16, 0, 96, 64]], "share": 0.25, "fill": [120, 128, 128], "tile": 16, "grow": 1, "feather": 16, "frames_sampled": 4,
          "applied": True}
    assert report.overlay_log_keys(None) == {} and report.overlay_log_keys(ov) == {"overlay": ov}
    line = report.overlay_summary_line(ov)
    assert "neutral" in line and "[16, 0, 96, 64]" in line and "25.0 %" in line and "[120, 128, 128]" in line
    assert "nothing masked" in report.overlay_summary_line(dict(ov, boxes=[], applied=False))
    assert "the reference" in report.overlay_summary_line(dict(ov, mode="reference", fill="reference"))
