"""score_files(distortion_map=) on the MI355X, end to end through the real engine: a 96 x 64, 10-frame Y4M pair with one
planted patch; the patch is reported as a defect event, the measurement equals the restatement (tests/tile_ref.py), and the
records of the scoring chain are those of a run without the option."""
import json

import numpy as np
import pytest

from tests import tile_ref as R

pytestmark = pytest.mark.gpu

W, H, T, FRAMES = 96, 64, 16, 10
PATCH = (24, 12, 40, 24)      # x0, y0, width, height: tiles 1 ... 3 by 0 ... 2


def _write(tmp_path):
    from pqa2_amd.yuvio import VideoInfo, write_y4m
    info = VideoInfo(width=W, height=H, fps_num=24, fps_den=1, bit_depth=8, mono=False, hshift=1, vshift=1, chroma_tag="420")
    rng = np.random.default_rng(3)
    ref = [rng.integers(16, 236, (H, W)).astype(np.uint8) for _ in range(FRAMES)]
    dis = [np.clip(np.rint(r + rng.normal(0.0, 2.0, r.shape)), 0, 255).astype(np.uint8) for r in ref]
    x0, y0, pw, ph = PATCH
    for f in (5, 6, 7):
        dis[f][y0:y0 + ph, x0:x0 + pw] = 255 - dis[f][y0:y0 + ph, x0:x0 + pw]
    grey = np.full((H // 2, W // 2), 128, np.uint8)
    rp, dp = str(tmp_path / "ref.y4m"), str(tmp_path / "dis.y4m")
    write_y4m(rp, [[f, grey, grey] for f in ref], info)
    write_y4m(dp, [[f, grey, grey] for f in dis], info)
    return rp, dp, ref, dis


def test_the_planted_patch_is_reported_and_the_records_are_untouched(tmp_path):
    from pqa2_amd import distortion as DM
    from pqa2_amd import report
    from pqa2_amd.engine import sse_from_records
    from pqa2_amd.pipeline import score_files
    rp, dp, ref, dis = _write(tmp_path)
    plain = score_files(rp, dp, "vmaf_v0.6.1", psnr=True)
    off = score_files(rp, dp, "vmaf_v0.6.1", psnr=True, distortion_map=0)
    on = score_files(rp, dp, "vmaf_v0.6.1", psnr=True, distortion_map=T, distortion_planes="all", distortion_dir=str(tmp_path / "maps"))
    assert "distortion" not in plain and "distortion" not in off and list(off["metrics"]) == list(plain["metrics"])
    for other in (off, on):
        assert np.array_equal(other["records"].view(np.uint64), plain["records"].view(np.uint64))
        assert all(np.array_equal(other["metrics"][k], plain["metrics"][k]) for k in plain["metrics"])
    d = on["distortion"]
    assert (d["tile"], d["grid"], d["frames"], list(d["planes"])) == (T, [6, 4], FRAMES, ["y", "cb", "cr"])
    y = d["planes"]["y"]
    assert len(y["defects"]) == 1
    ev = y["defects"][0]
    assert (ev["first"], ev["last"], ev["frames"], ev["box"]) == (5, 7, 3, [16, 0, 64, 48]) and ev["share"] > 0.99
    assert y["persistent"] == [] and y["worst_frame"]["frame"] in (5, 6, 7)
    assert d["planes"]["cb"]["defects"] == [] and d["planes"]["cb"]["psnr_all"] == 60.0
    # the measurement is the restatement's, and the solver's clip PSNR is the one of the PSNR feature's exact SSE
    M = R.tile_moments(ref, dis, T)
    assert np.array_equal(np.load(tmp_path / "maps" / "distortion_y.npy"), M.sum(axis=0, dtype=np.uint64))
    cols = DM.frame_summary(M, W, H, T, 8)
    assert np.array_equal(on["metrics"]["tile_psnr_min"], cols["tile_psnr_min"])
    assert np.array_equal(on["metrics"]["distortion_concentration"], cols["concentration"])
    total = sum(int(v) for v in sse_from_records(on["records"])[:, 0])
    assert y["psnr_all"] == float(R.psnr_of(np.array([total / (W * H * FRAMES)]), 8)[0])
    data = open(tmp_path / "maps" / "distortion_y.pgm", "rb").read()
    assert data.startswith(b"P5\n6 4\n255\n") and len(data) == 11 + 24
    json.dumps(report.distortion_log_keys(d))
