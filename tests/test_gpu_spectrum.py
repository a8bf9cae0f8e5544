"""score_files(spectrum=) on the MI355X, end to end through the real engine: a 96 x 64, 10-frame Y4M pair whose capture is the
horizontally blurred reference comes out as a horizontal detail loss from score_files and from python -m pqa2_amd.score, a
pair with added noise as noise; the measurement equals the restatement (tests/spectrum_ref.py), the records of the scoring
chain are those of a run without the option, and two ranks that share the GPU report the same object."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from tests import spectrum_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, L, FRAMES = 96, 64, 4, 10


def _write(tmp_path, kind):
    from pqa2_amd.yuvio import VideoInfo, write_y4m
    info = VideoInfo(width=W, height=H, fps_num=24, fps_den=1, bit_depth=8, mono=False, hshift=1, vshift=1, chroma_tag="420")
    ref = [R.noise_plane(20 + t, W, H) for t in range(FRAMES)]
    dis = [R.h_blur(r) if kind == "blur" else R.add_noise(r, 40 + t, 8) for t, r in enumerate(ref)]
    grey = np.full((H // 2, W // 2), 128, np.uint8)
    rp, dp = str(tmp_path / f"ref_{kind}.y4m"), str(tmp_path / f"dis_{kind}.y4m")
    write_y4m(rp, [[f, grey, grey] for f in ref], info)
    write_y4m(dp, [[f, grey, grey] for f in dis], info)
    return rp, dp, ref, dis


def test_a_blurred_capture_is_a_horizontal_loss_and_the_records_are_untouched(tmp_path):
    from pqa2_amd import report
    from pqa2_amd import spectrum as SP
    from pqa2_amd.pipeline import score_files
    rp, dp, ref, dis = _write(tmp_path, "blur")
    plain = score_files(rp, dp, "vmaf_v0.6.1", psnr=True)
    on = score_files(rp, dp, "vmaf_v0.6.1", psnr=True, spectrum=L, spectrum_planes="all", distortion_map=16)
    assert "spectrum" not in plain
    assert np.array_equal(on["records"].view(np.uint64), plain["records"].view(np.uint64))
    assert all(np.array_equal(on["metrics"][k], plain["metrics"][k]) for k in plain["metrics"])
    sp = on["spectrum"]
    assert (sp["levels"], sp["frames"], list(sp["planes"])) == (L, FRAMES, ["y", "cb", "cr"])
    M = R.band_moments(ref, dis, L)
    assert sp["planes"]["y"] == SP.analyse(M, W, H, 8)      # the measurement is the restatement's
    s = sp["planes"]["y"]["summary"]
    assert (s["kind"], s["axis"], s["bandwidth_h"]["level"], s["bandwidth_v"]["level"]) == ("loss", "horizontal", 2, 1)
    assert sp["planes"]["cb"]["summary"]["kind"] == "identical"
    cols = SP.frame_columns(M, W, H, 8)
    assert all(np.array_equal(on["metrics"][k], cols[k]) for k in cols)
    assert on["distortion"] == score_files(rp, dp, "vmaf_v0.6.1", distortion_map=16)["distortion"]      # the shared pass
    json.dumps(report.spectrum_log_keys(sp))


def test_added_noise_is_noise(tmp_path):
    from pqa2_amd.pipeline import score_files
    rp, dp, _, _ = _write(tmp_path, "noise")
    s = score_files(rp, dp, "vmaf_v0.6.1", spectrum=L)["spectrum"]["planes"]["y"]["summary"]
    assert s["kind"] == "noise" and s["noise_share"] > 0.99 and s["bandwidth_h"]["level"] == 1


def test_the_cli_and_two_ranks_report_the_same_object(tmp_path):
    """python -m pqa2_amd.score --spectrum 4, plain and as a 2-rank gloo job on one GPU: the same JSON, a horizontal loss"""
    rp, dp, _, _ = _write(tmp_path, "blur")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, PYTHONPATH=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0")
    outs = {}
    for tag, launcher in (("one", []), ("two", ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                                                 "--master-addr", "127.0.0.1", "--master-port", str(port)])):
        j = str(tmp_path / f"{tag}.json")
        cmd = [sys.executable] + launcher + ["-m", "pqa2_amd.score", rp, dp, "--json", j, "--batch", "2", "--spectrum", str(L)]
        if launcher:
            cmd += ["--backend", "gloo", "--share-device"]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        if not launcher:
            assert "Distortion spectrum: 4 octaves on 10 frames, loss (horizontal)" in r.stderr
        d = json.load(open(j))
        d.pop("fps", None)
        outs[tag] = d
    assert outs["one"] == outs["two"]
    y = outs["one"]["spectrum"]["planes"]["y"]["summary"]
    assert (y["kind"], y["axis"]) == ("loss", "horizontal") and "detail_gain_h" in outs["one"]["frames"][5]["metrics"]
