"""score_files(coding_grid=True) on the MI355X, end to end through the real engine, on the committed c352x288_8 clips (their
distortion includes an 8 x 8 DC quantisation of the luma): the result equals the solver run on the restatement's profiles
(tests/edge_ref.py), the luma has an aligned 8-grid and the chroma none, every other metric and record is that of a run without
the option, and the pass shared with the distortion map, the spectrum and the temporal distortion gives the same."""
import os

import numpy as np
import pytest

from tests import edge_ref as R

pytestmark = pytest.mark.gpu

CLIPS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clips")
REF, DIS = os.path.join(CLIPS, "c352x288_8_ref.y4m"), os.path.join(CLIPS, "c352x288_8_dist.y4m")
COLUMNS = {"blockiness_x", "blockiness_y"}
_RES = {}


def _frames(path):
    from pqa2_amd.yuvio import open_video
    rd = open_video(path)
    try:
        return [[np.array(p) for p in rd.frame(i)] for i in range(len(rd))]
    finally:
        rd.close()


def results():
    """(plain, on): one run without the option and one with it, shared by the tests"""
    if not _RES:
        from pqa2_amd.pipeline import score_files
        _RES["plain"] = score_files(REF, DIS, "vmaf_v0.6.1", psnr=True)
        _RES["on"] = score_files(REF, DIS, "vmaf_v0.6.1", psnr=True, coding_grid=True, grid_planes="all")
    return _RES["plain"], _RES["on"]


def test_the_result_is_the_solver_on_the_restatements_profiles():
    from pqa2_amd import grid as G
    plain, on = results()
    ref, dis = _frames(REF), _frames(DIS)
    want = {}
    for p, name in enumerate(("y", "cb", "cr")):
        h, w = ref[0][p].shape
        rows, cols = R.edge_profiles([f[p] for f in ref], [f[p] for f in dis], 8)
        want[name] = G.analyse(rows, cols, w, h, 8)
    assert on["coding_grid"] == {"planes": want}
    y = on["coding_grid"]["planes"]["y"]["summary"]
    assert y["kind"] == "grid" and y["block"] == [8, 8] and y["phase"] == [0, 0] and y["aligned"] is True
    assert (y["x"]["period"], y["x"]["phase"], y["y"]["period"], y["y"]["phase"]) == (8, 0, 8, 0)
    assert on["coding_grid"]["planes"]["cb"]["summary"]["kind"] == "none"
    assert on["coding_grid"]["planes"]["cr"]["summary"]["kind"] == "none"
    cols = G.frame_columns(want["y"]["frames"])
    assert all(np.array_equal(on["metrics"][k], cols[k]) for k in COLUMNS)


def test_everything_else_is_untouched():
    plain, on = results()
    assert "coding_grid" not in plain
    assert np.array_equal(on["records"].view(np.uint64), plain["records"].view(np.uint64))
    assert all(np.array_equal(on["metrics"][k], plain["metrics"][k]) for k in plain["metrics"])
    assert set(on["metrics"]) - set(plain["metrics"]) == COLUMNS


def test_one_shared_pass_gives_the_same():
    from pqa2_amd.pipeline import score_files
    plain, on = results()
    both = score_files(REF, DIS, "vmaf_v0.6.1", psnr=True, coding_grid=True, grid_planes="all", distortion_map=32, spectrum=3,
                       temporal=32)
    assert both["coding_grid"] == on["coding_grid"]
    assert {"distortion", "spectrum", "temporal"} <= set(both)
    assert np.array_equal(both["records"].view(np.uint64), plain["records"].view(np.uint64))
    assert all(np.array_equal(both["metrics"][k], on["metrics"][k]) for k in on["metrics"])
