"""score_files(temporal=) on the MI355X, end to end through the real engine: a 64 x 48, 12-frame Y4M pair whose capture is the
reference blended half and half with its previous frame comes out as a blend of weight 1/2; the measurement equals the
restatement (tests/temporal_ref.py), the JSON carries the object and the per-frame columns, the pass shared with the
distortion map and the spectrum gives what three separate runs give, and the records of the scoring chain are those of a run
without the option."""
import json

import numpy as np
import pytest

from tests import temporal_ref as R

pytestmark = pytest.mark.gpu

W, H, T, FRAMES, PAN = 64, 48, 32, 12, 3
COLUMNS = {"temporal_gain", "temporal_noise_mse", "blend_weight"}


def _write(tmp_path):
    """the reference: white noise through a Gaussian of sigma 4 px, stretched over the code range, panned 3 px a frame"""
    from pqa2_amd.yuvio import VideoInfo, write_y4m
    info = VideoInfo(width=W, height=H, fps_num=24, fps_den=1, bit_depth=8, mono=False, hshift=1, vshift=1, chroma_tag="420")
    rng = np.random.default_rng(3)
    x = rng.standard_normal((H + 32, W + PAN * FRAMES + 32))
    k = np.exp(-0.5 * (np.arange(-16, 17) / 4.0) ** 2)
    k /= k.sum()
    x = np.apply_along_axis(lambda v: np.convolve(v, k, "valid"), 1, x)
    x = np.apply_along_axis(lambda v: np.convolve(v, k, "valid"), 0, x)
    x = np.rint(255.0 * (x - x.min()) / (x.max() - x.min())).astype(np.int64)
    ref = [x[:, PAN * t:PAN * t + W].astype(np.uint8) for t in range(FRAMES)]
    dis = [ref[0]] + [((ref[t].astype(np.int64) + ref[t - 1] + 1) >> 1).astype(np.uint8) for t in range(1, FRAMES)]
    grey = np.full((H // 2, W // 2), 128, np.uint8)
    rp, dp = str(tmp_path / "ref.y4m"), str(tmp_path / "dis.y4m")
    write_y4m(rp, [[f, grey, grey] for f in ref], info)
    write_y4m(dp, [[f, grey, grey] for f in dis], info)
    return rp, dp, ref, dis


def test_a_blended_capture_is_a_blend_and_the_records_are_untouched(tmp_path):
    from pqa2_amd import report
    from pqa2_amd import temporal as TP
    from pqa2_amd.pipeline import score_files
    rp, dp, ref, dis = _write(tmp_path)
    plain = score_files(rp, dp, "vmaf_v0.6.1", psnr=True)
    on = score_files(rp, dp, "vmaf_v0.6.1", psnr=True, temporal=T, temporal_planes="all")
    assert "temporal" not in plain
    assert np.array_equal(on["records"].view(np.uint64), plain["records"].view(np.uint64))      # the VMAF records
    assert all(np.array_equal(on["metrics"][k], plain["metrics"][k]) for k in plain["metrics"])
    assert set(on["metrics"]) - set(plain["metrics"]) == COLUMNS
    tp = on["temporal"]
    assert set(tp) == {"tile", "planes", "frames"}
    assert (tp["tile"], tp["frames"], list(tp["planes"])) == (T, FRAMES, ["y", "cb", "cr"])
    M = R.temporal_moments(ref, dis, T)
    assert tp["planes"]["y"] == TP.analyse(M, W, H, T, 8)      # the measurement is the restatement's
    s = tp["planes"]["y"]["summary"]
    assert s["kind"] == "blend" and abs(s["blend_weight"] - 0.5) < 0.01
    assert {"kind", "transitions", "motion_mse", "temporal_mse", "loss_mse", "noise_mse", "gain", "blend_weight", "pops",
            "pop_period", "still_noise_mse", "level_step_max"} <= set(s)
    assert len(tp["planes"]["y"]["frames"]) == FRAMES - 1
    assert {"frame", "motion_mse", "temporal_mse", "gain", "blend_weight", "level_step", "loss_mse", "noise_mse"} == set(
        tp["planes"]["y"]["frames"][0])
    assert tp["planes"]["cb"]["summary"]["kind"] == "identical"
    cols = TP.frame_columns(M, W, H, 8)
    assert all(np.array_equal(on["metrics"][k], cols[k]) for k in COLUMNS)
    assert abs(on["metrics"]["blend_weight"][5] - 0.5) < 0.02 and on["metrics"]["blend_weight"][0] == 0.0
    log = report.build_vmaf_log(on["metrics"], 0.0, on["frame_indices"], {"model": on["model_name"], **report.temporal_log_keys(tp)})
    report.write_vmaf_json(str(tmp_path / "on.json"), log)
    logged = json.load(open(tmp_path / "on.json"))
    assert logged["temporal"] == json.loads(json.dumps(tp)) and COLUMNS <= set(logged["frames"][3]["metrics"])
    assert report.temporal_summary_line(tp).startswith("Temporal distortion: 32 px tiles on 12 frames, blend (weight 0.5")


def test_one_shared_pass_equals_three_separate_runs(tmp_path):
    from pqa2_amd.pipeline import score_files
    rp, dp, _, _ = _write(tmp_path)
    both = score_files(rp, dp, "vmaf_v0.6.1", temporal=T, distortion_map=32, spectrum=3)
    assert both["temporal"] == score_files(rp, dp, "vmaf_v0.6.1", temporal=T)["temporal"]
    assert both["distortion"] == score_files(rp, dp, "vmaf_v0.6.1", distortion_map=32)["distortion"]
    assert both["spectrum"] == score_files(rp, dp, "vmaf_v0.6.1", spectrum=3)["spectrum"]
    plain = score_files(rp, dp, "vmaf_v0.6.1")
    assert np.array_equal(both["records"].view(np.uint64), plain["records"].view(np.uint64))
