"""Overlay masking end to end on the MI355X: Y4M files in a tmp dir through score_files(overlay_mask=).  The clips are
synth.make_clip at 320 x 180, 8 frames, 4:2:0, 8 bit, with a 64 x 32 checkerboard burnt into the captured luma at
mask_ref.LOGO_BOX; tests/test_overlay.py takes the same step through an oracle stand-in on the CPU.  On the parent commit
score_files has no overlay_mask."""
import numpy as np
import pytest

from tests import mask_ref as MR

pytestmark = pytest.mark.gpu

W, H, N_FRAMES = 320, 180, 8
GROWN = [192, 96, 304, 176]      # the logo's tiles [208, 112, 288, 160] grown by one tile of 16


@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    from pqa2_amd import synth
    from pqa2_amd.yuvio import write_y4m
    d = tmp_path_factory.mktemp("overlay")
    info = synth.clip_info(W, H)
    refs, clean = synth.make_clip(W, H, N_FRAMES)
    logo = [[MR.checker_logo(f[0]), f[1], f[2]] for f in clean]
    paths = {}
    for key, clip in (("ref", refs), ("clean", clean), ("logo", logo)):
        paths[key] = str(d / (key + ".y4m"))
        write_y4m(paths[key], clip, info)
    return paths


@pytest.fixture(scope="module")
def plain(clips):
    """the unmasked runs, computed once"""
    from pqa2_amd.pipeline import score_files
    return {k: score_files(clips["ref"], clips[k], "vmaf_v0.6.1") for k in ("clean", "logo", "ref")}


def _bits(res):
    return res["records"].view(np.uint64)


def _vmaf(res):
    return float(np.mean(res["metrics"]["vmaf"]))


def test_report_finds_the_logo_and_changes_no_score(clips, plain):
    from pqa2_amd.pipeline import score_files
    rep = score_files(clips["ref"], clips["logo"], "vmaf_v0.6.1", overlay_mask="report")
    ov = rep["overlay"]
    assert ov["regions"][0]["box"] == [208, 112, 288, 160] and len(ov["regions"]) == 1 and ov["regions"][0]["tiles"] == 15
    assert ov["boxes"] == [GROWN] and not ov["applied"] and ov["detected"] and ov["frames_sampled"] == N_FRAMES
    assert round(ov["share"], 3) == 0.246
    assert np.array_equal(_bits(rep), _bits(plain["logo"])) and rep["metrics"].keys() == plain["logo"]["metrics"].keys()
    for k, v in plain["logo"]["metrics"].items():
        assert np.array_equal(np.asarray(v), np.asarray(rep["metrics"][k]), equal_nan=True), k
    off = score_files(clips["ref"], clips["logo"], "vmaf_v0.6.1", overlay_mask=None)
    assert "overlay" not in off and "overlay" not in plain["logo"] and np.array_equal(_bits(off), _bits(plain["logo"]))
    none = score_files(clips["ref"], clips["clean"], "vmaf_v0.6.1", overlay_mask="neutral")     # no persistent tile: nothing applied
    assert none["overlay"]["regions"] == [] and not none["overlay"]["applied"] and np.array_equal(_bits(none), _bits(plain["clean"]))


def test_neutral_box_makes_logo_and_clean_clip_bit_identical(clips, plain):
    """every logo sample has alpha = 256: both runs submit the same integers"""
    from pqa2_amd.pipeline import score_files
    kw = dict(overlay_mask="neutral", overlay_boxes=[GROWN])
    with_logo = score_files(clips["ref"], clips["logo"], "vmaf_v0.6.1", **kw)
    clean = score_files(clips["ref"], clips["clean"], "vmaf_v0.6.1", **kw)
    assert np.array_equal(_bits(with_logo), _bits(clean))
    assert not np.array_equal(_bits(with_logo), _bits(plain["logo"])) and not np.array_equal(_bits(clean), _bits(plain["clean"]))
    ov = with_logo["overlay"]
    assert ov == clean["overlay"] and ov["applied"] and not ov["detected"] and ov["boxes"] == [GROWN] and ov["fill"][1:] == [128, 128]
    # the second pass sees the masked clips too: the distortion map of the logo clip finds no persistent region any more
    kw = dict(kw, distortion_map=16)
    a, b = (score_files(clips["ref"], clips[k], "vmaf_v0.6.1", **kw) for k in ("logo", "clean"))
    assert a["distortion"]["planes"]["y"]["persistent"] == [] and a["distortion"]["planes"]["y"]["psnr_all"] == b["distortion"]["planes"]["y"]["psnr_all"]


def test_detected_neutral_mask_gives_most_of_the_score_back(clips, plain):
    """|masked - clean| < 1/2 |logo - clean|: a sanity bound, not a tolerance (the f64 oracle gives 0.266 of it).  On the
    MI355X, one run: clean 83.4712, logo 75.2614 and masked 80.7871 (ratio 0.327), as printed below (DESIGN.md section 5 quotes them)."""
    from pqa2_amd.pipeline import score_files
    masked = score_files(clips["ref"], clips["logo"], "vmaf_v0.6.1", overlay_mask="neutral")
    v_clean, v_logo, v_masked = _vmaf(plain["clean"]), _vmaf(plain["logo"]), _vmaf(masked)
    print(f"overlay vmaf: clean {v_clean:.4f} logo {v_logo:.4f} masked {v_masked:.4f} "
          f"ratio {abs(v_masked - v_clean) / abs(v_logo - v_clean):.4f} fill {masked['overlay']['fill']}")
    assert masked["overlay"]["applied"] and masked["overlay"]["boxes"] == [GROWN]
    assert abs(v_masked - v_clean) < 0.5 * abs(v_logo - v_clean)


def test_reference_mode(clips, plain):
    from pqa2_amd.pipeline import score_files
    same = score_files(clips["ref"], clips["ref"], "vmaf_v0.6.1", overlay_mask="reference", overlay_boxes=[list(MR.LOGO_BOX)])
    assert same["overlay"]["applied"] and same["overlay"]["fill"] == "reference"
    assert np.array_equal(_bits(same), _bits(plain["ref"]))      # an identical pair stays one, plane for plane
    fixed = score_files(clips["ref"], clips["logo"], "vmaf_v0.6.1", overlay_mask="reference")
    print(f"overlay vmaf: reference mode {_vmaf(fixed):.4f} against clean {_vmaf(plain['clean']):.4f}")
    assert _vmaf(fixed) > _vmaf(plain["logo"]) and fixed["overlay"]["boxes"] == [GROWN]


def test_ten_bit_422_goes_through_all_three_planes(tmp_path):
    from pqa2_amd import distortion as D
    from pqa2_amd import pipeline as P
    from pqa2_amd.engine import FeatureEngine
    from pqa2_amd.yuvio import VideoInfo, open_video, write_y4m
    w, h, n = 98, 54, 3
    info = VideoInfo(w, h, 10, 1, 0, False, 25, 1, 0, "422p10")
    rng = np.random.default_rng(3)
    frames = [[rng.integers(0, 1024, s).astype(np.uint16) for s in ((h, w), (h, 49), (h, 49))] for _ in range(2 * n)]
    ref, dis = str(tmp_path / "ref.y4m"), str(tmp_path / "dis.y4m")
    write_y4m(ref, frames[:n], info)
    write_y4m(dis, frames[n:], info)
    box = [[33, 10, 71, 40]]
    res = P.score_files(ref, dis, "vmaf_v0.6.1", overlay_mask="neutral", overlay_boxes=box)
    assert res["overlay"]["applied"] and res["overlay"]["boxes"] == [[32, 8, 72, 40]] and res["overlay"]["fill"][1:] == [512, 512]
    res = P.score_files(ref, dis, "vmaf_v0.6.1", overlay_mask="reference", overlay_boxes=box)
    assert res["overlay"]["applied"]
    mask = D.overlay_mask_from_boxes(box, w, h, chroma_shift=(1, 0))
    fills = res["overlay"]["fill"] if res["overlay"]["fill"] != "reference" else [300, 512, 512]
    rd = open_video(dis)
    steps = ((3, 3), (2, 3), (2, 3))
    masked = P._MaskedReader(rd, mask, fills, None, 0, FeatureEngine)
    towards = P._MaskedReader(rd, mask, None, open_video(ref), 0, FeatureEngine)
    try:
        for i in range(n):
            for p in range(3):
                assert np.array_equal(masked.frame(i)[p], MR.blend(frames[n + i][p], mask["nodes"], *steps[p], fills[p], 10)), (i, p)
                assert np.array_equal(towards.frame(i)[p], MR.blend(frames[n + i][p], mask["nodes"], *steps[p], frames[i][p], 10)), (i, p)
    finally:
        masked.close()
        towards.close()
