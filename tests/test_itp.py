"""Delta E ITP (ITU-R BT.2124) without a GPU: the restatement (tests/itp_ref.py) against published values, pqa2_amd/itp.py's
matrices and verdicts, and the plumbing through score_files, the command line and the analyzer on a stand-in engine."""
import json
import os
import re

import numpy as np
import pytest

from tests import itp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the definition ---------------------------------------------------------------------------------------------------
def test_pq_pins():
    assert abs(R.pq_inverse(100 / 10000) - 0.508078) <= 5e-7
    assert abs(R.pq_inverse(203 / 10000) - 0.5807) <= 1e-4          # BT.2408 reference white
    assert R.pq_inverse(1.0) == 1.0
    y = np.concatenate([[0.0], np.logspace(-7, 0, 200)])
    assert np.abs(R.pq_eotf(R.pq_inverse(y)) - y).max() <= 1e-12
    e = np.linspace(0, 1, 1025)[1:]      # not 0: ST 2084 maps black to c1^m2 = 7.3e-7, not to 0
    assert np.abs(R.pq_inverse(R.pq_eotf(e)) - e).max() <= 1e-12
    assert abs(R.pq_inverse(0.0) - R.C1 ** R.M2) <= 1e-18


def test_hlg_reference_white():
    f = R.display_light(np.array([0.75, 0.75, 0.75]), "hlg", 1000.0)
    assert np.abs(f - 203.0).max() <= 0.5
    assert abs(R.hlg_gamma(1000.0) - 1.2) <= 1e-15
    assert np.abs(R.display_light(np.array([1.0, 1.0, 1.0]), "hlg", 1000.0) - 1000.0).max() <= 1e-3   # (e^((1-c)/a) + b) / 12 = 1
    assert (R.display_light(np.zeros(3), "hlg", 400.0) == 0.0).all()       # gamma < 1: black stays black


def test_matrix_row_sums_and_greys():
    assert np.abs(R.RGB_TO_LMS.sum(axis=1) - 1).max() <= 1e-15
    assert np.abs((R.RGB_TO_LMS @ R.BT709_TO_BT2020).sum(axis=1) - 1).max() <= 1e-12
    s = R.LMS_TO_ICTCP.sum(axis=1)
    assert s[0] == 1.0 and s[1] == 0.0 and s[2] == 0.0
    for transfer, bpc in (("pq", 10), ("hlg", 10), ("bt1886", 8), ("pq", 12)):
        sp = R.make_spec(transfer, bit_depth=bpc)
        mid = 1 << (bpc - 1)
        y = np.arange(16 << (bpc - 8), 236 << (bpc - 8), 3, dtype=np.float64)
        c = R.ictcp(np.column_stack([y, np.full_like(y, mid), np.full_like(y, mid)]), sp)
        assert np.abs(c[:, 1:]).max() <= 1e-9, transfer
        rgb = (y - (16 << (bpc - 8))) / (219 << (bpc - 8))
        lum = R.display_light(np.column_stack([rgb] * 3), transfer, sp["peak"])[:, 0]
        assert np.abs(c[:, 0] - 720 * R.pq_inverse(lum / 10000)).max() <= 1e-9, transfer


def test_one_jnd_and_the_grey_pair():
    sp = R.make_spec("pq")
    # two PQ greys whose I differs by 1 / 720: code values through the decode matrix, fractional
    ya = 64 + 876 * 0.5
    yb = 64 + 876 * (0.5 + 1 / 720)
    de, di, dt, dp = R.delta_e(np.array([ya, 512, 512]), np.array([yb, 512, 512]), sp)
    assert abs(de - 1.0) <= 1e-9 and abs(abs(di) - 1.0) <= 1e-9 and abs(dt) <= 1e-9 and abs(dp) <= 1e-9
    de, _, _, _ = R.delta_e(np.array([502.0, 512, 512]), np.array([503.0, 512, 512]), sp)
    assert abs(de - 0.82192) <= 5e-6


def test_identity_symmetry_and_the_split():
    rng = np.random.default_rng(2)
    a = rng.integers(0, 1024, (500, 3)).astype(np.float64)
    b = rng.integers(0, 1024, (500, 3)).astype(np.float64)
    for transfer in ("pq", "hlg", "bt1886"):
        sp = R.make_spec(transfer)
        assert (R.delta_e(a, a, sp)[0] == 0.0).all()
        de, di, dt, dp = R.delta_e(a, b, sp)
        assert np.array_equal(de, R.delta_e(b, a, sp)[0])
        assert abs((de ** 2).sum() - ((di ** 2).sum() + (dt ** 2).sum() + (dp ** 2).sum())) <= 1e-9 * (de ** 2).sum()
        assert np.isfinite(de).all() and de.max() > 1


def test_frame_sums_layout():
    rng = np.random.default_rng(4)
    w, h = 10, 6
    ref = [rng.integers(64, 940, (h, w)), rng.integers(64, 960, (h // 2, w // 2)), rng.integers(64, 960, (h // 2, w // 2))]
    dis = [ref[0] + 3, ref[1], ref[2] + 5]
    sp = R.make_spec("pq")
    s = R.frame_sums(ref, dis, sp, 1, 1)
    de, d, i_ref = R.frame_de(ref, dis, sp, 1, 1)
    assert s[6] == w * h and s[4] == de.max() and s[5] == (de > 1).sum()
    assert abs(s[0] - de.sum()) <= 1e-9 and abs((s[1] + s[2] + s[3]) - (de ** 2).sum()) <= 1e-8
    assert np.array_equal(R.upsample(ref, 1, 1)[1, 3], [ref[0][1, 3], ref[1][0, 1], ref[2][0, 1]])


# ---- pqa2_amd/itp.py ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transfer,matrix,full,bpc", [("pq", "bt2020", False, 10), ("hlg", "bt2020", False, 10), ("pq", "bt2020", True, 12),
                                                       ("bt1886", "bt709", False, 8), ("bt1886", "bt601", True, 8),
                                                       ("bt1886", "bt709", False, 10)])
def test_spec_agrees_with_the_restatement(transfer, matrix, full, bpc):
    from pqa2_amd import itp
    sp = itp.spec(transfer, matrix, full, bpc)
    ref = R.make_spec(transfer, matrix, full, bpc)
    assert np.abs(np.array(sp["yuv_to_rgb"]) - ref["yuv_to_rgb"].ravel()).max() <= 1e-7
    assert np.abs(np.array(sp["rgb_to_lms"]) * 1e4 - ref["rgb_to_lms"].ravel() * 1e4).max() <= 1e-7
    assert sp["peak"] == ref["peak"] and sp["threshold"] == 1.0
    assert sp["range"] == ("full" if full else "limited") and sp["bit_depth"] == bpc


def test_spec_defaults_primaries_and_errors():
    from pqa2_amd import itp, _native as N
    assert itp.spec("pq")["matrix"] == "bt2020" and itp.spec("hlg")["peak"] == 1000.0 and itp.spec("bt1886")["peak"] == 100.0
    assert itp.spec("bt1886", height=480)["matrix"] == "bt601" and itp.spec("bt1886", height=1080)["matrix"] == "bt709"
    sdr = itp.spec("bt1886", "bt709", bit_depth=8)
    assert sdr["primaries"] == "bt709"
    want = (R.RGB_TO_LMS @ R.BT709_TO_BT2020) / 1e4
    assert np.abs(np.array(sdr["rgb_to_lms"]) - want.ravel()).max() <= 1e-11
    assert np.abs(np.array(sdr["rgb_to_lms"]) - (R.RGB_TO_LMS / 1e4).ravel()).max() > 1e-6       # not the 2020 matrix
    assert itp.spec("pq", "bt2020")["primaries"] == "bt2020"
    for kw in (dict(transfer="srgb"), dict(transfer="pq", matrix="xyz"), dict(transfer="hlg", peak=0), dict(transfer="pq", threshold=-1),
               dict(transfer="pq", bit_depth=7)):
        with pytest.raises(ValueError):
            itp.spec(**kw)
    ns = itp.native_spec(itp.spec("hlg", peak=600, threshold=2.5))
    assert (ns.transfer, ns.peak, ns.threshold) == (N.ITP_HLG, 600.0, 2.5) and len(ns.yuv_to_rgb) == 12 and len(ns.rgb_to_lms) == 9


def _row(px, mean, di2, dt2, dp2, mx, above, i=0.5):
    return [mean * px, di2 * px, dt2 * px, dp2 * px, mx, above, px, i * px]


def test_summary_decisions():
    from pqa2_amd import itp
    px = 1000
    s = itp.summary([_row(px, 0, 0, 0, 0, 0, 0)] * 2)
    assert s["kind"] == "identical" and s["mean"] == 0 and s["above_jnd"] == 0 and s["frames"] == 2
    s = itp.summary([_row(px, 0.3, 0.1, 0.01, 0.01, 0.9, 0)])
    assert s["kind"] == "below_jnd"
    s = itp.summary([_row(px, 2.0, 4.0, 0.5, 0.5, 6.0, 700), _row(px, 1.0, 1.0, 0.1, 0.1, 3.0, 300)])
    assert s["kind"] == "luminance" and s["worst_frame"] == 0 and abs(s["mean"] - 1.5) <= 1e-12 and abs(s["above_jnd"] - 0.5) <= 1e-12
    assert abs(s["luminance_share"] - 5.0 / 6.2) <= 1e-12 and abs(s["luminance_share"] + s["chroma_share"] - 1) <= 1e-12
    assert s["max"] == 6.0 and abs(s["rms"] - np.sqrt(6.2 / 2)) <= 1e-12
    assert s["per_frame"]["delta_e_itp"] == [2.0, 1.0] and s["per_frame"]["itp_above_jnd"] == [0.7, 0.3]
    assert itp.summary([_row(px, 2.0, 0.5, 3.0, 1.0, 6.0, 700)])["kind"] == "chroma"
    assert itp.summary([_row(px, 2.0, 2.0, 1.0, 1.0, 6.0, 700)])["kind"] == "mixed"
    assert itp.summary([_row(px, 2.0, 3.0, 0.5, 0.5, 6.0, 700)])["kind"] == "luminance"      # exactly 3/4
    assert itp.summary([_row(px, 0.3, 0.1, 0.01, 0.01, 2.5, 1)], threshold=3.0)["kind"] == "below_jnd"
    with pytest.raises(ValueError):
        itp.summary(np.zeros((0, 8)))
    cols = itp.frame_columns([_row(px, 2.0, 4.0, 0.5, 0.5, 6.0, 700)])
    assert sorted(cols) == ["delta_e_itp", "delta_e_itp_max", "itp_above_jnd"]


# ---- score_files, the command line and the analyzer through a stand-in engine -----------------------------------------------
CALLS = []


def _itp_engine():
    from tests.fake_engine import OracleEngine

    class ItpEngine(OracleEngine):
        """the oracle stand-in plus the restated Delta E ITP"""

        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.hs, self.vs = kw.get("chroma_shift", (1, 1))

        def delta_itp(self, ref_frames, dis_frames, spec):
            from pqa2_amd import _native as N
            assert self.n_planes == 3 and isinstance(spec, N.PqaItpSpec)
            CALLS.append(len(ref_frames))
            sp = {"transfer": {0: "pq", 1: "hlg", 2: "bt1886"}[spec.transfer], "yuv_to_rgb": np.array(list(spec.yuv_to_rgb), np.float64),
                  "rgb_to_lms": np.array(list(spec.rgb_to_lms), np.float64), "peak": float(spec.peak), "threshold": float(spec.threshold)}
            return np.stack([R.frame_sums(r, d, sp, self.hs, self.vs) for r, d in zip(ref_frames, dis_frames)])
    return ItpEngine


def _write(tmp_path, n=11, w=48, h=32, mono=False, bpc=10, full=False):
    from pqa2_amd.yuvio import VideoInfo, write_y4m
    rng = np.random.default_rng(8)
    info = VideoInfo(width=w, height=h, fps_num=24, fps_den=1, bit_depth=bpc, mono=mono, hshift=1, vshift=1,
                     chroma_tag="mono" if mono else ("420p10" if bpc == 10 else "420"), **({"color_range": "full"} if full else {}))
    dt = np.uint16 if bpc > 8 else np.uint8
    s = 1 << (bpc - 8)
    ref = [[rng.integers(16 * s, 235 * s, (h, w)).astype(dt), rng.integers(100 * s, 156 * s, (h // 2, w // 2)).astype(dt),
            rng.integers(100 * s, 156 * s, (h // 2, w // 2)).astype(dt)] for _ in range(n)]
    dis = [[(f[0] + 2 * s).astype(dt), f[1], (f[2] + (i % 3) * s).astype(dt)] for i, f in enumerate(ref)]
    rp, dp = str(tmp_path / "r.y4m"), str(tmp_path / "d.y4m")
    write_y4m(rp, [f[:1] for f in ref] if mono else ref, info)
    write_y4m(dp, [f[:1] for f in dis] if mono else dis, info)
    return rp, dp, ref, dis


def test_score_files_columns_object_and_defaults(tmp_path):
    from pqa2_amd import report
    from pqa2_amd.pipeline import score_files
    rp, dp, ref, dis = _write(tmp_path)
    kw = dict(engine_factory=_itp_engine())
    del CALLS[:]
    plain = score_files(rp, dp, "vmaf_v0.6.1", **kw)
    assert CALLS == [] and "delta_itp" not in plain and "delta_e_itp" not in plain["metrics"]
    res = score_files(rp, dp, "vmaf_v0.6.1", delta_itp="pq", **kw)
    assert CALLS == [8, 3]                                       # 8 pairs a call
    assert np.array_equal(res["records"].view(np.uint64), plain["records"].view(np.uint64))
    sp = res["delta_itp"]["spec"]
    assert (sp["transfer"], sp["matrix"], sp["range"], sp["bit_depth"], sp["threshold"]) == ("pq", "bt2020", "limited", 10, 1.0)
    assert len(sp["yuv_to_rgb"]) == 12 and len(sp["rgb_to_lms"]) == 9
    ref_spec = R.make_spec("pq")
    for i in range(len(ref)):
        de, _, _ = R.frame_de(ref[i], dis[i], ref_spec, 1, 1)
        assert abs(res["metrics"]["delta_e_itp"][i] - de.mean()) <= 1e-4          # f32 coefficients against f64 ones
        assert abs(res["metrics"]["delta_e_itp_max"][i] - de.max()) <= 1e-4
        assert abs(res["metrics"]["itp_above_jnd"][i] - (de > 1).mean()) <= 0.01
    summ = res["delta_itp"]["summary"]
    assert summ["frames"] == len(ref) and summ["kind"] in ("luminance", "mixed", "chroma")
    assert abs(summ["mean"] - np.mean(res["metrics"]["delta_e_itp"])) <= 1e-12
    log = report.build_vmaf_log(res["metrics"], res["fps"], res["frame_indices"], report.itp_log_keys(res["delta_itp"]))
    log = json.loads(json.dumps(log))
    assert "delta_e_itp" in log["pooled_metrics"] and "itp_above_jnd" in log["frames"][3]["metrics"]
    assert log["delta_itp"]["summary"]["kind"] == summ["kind"] and report.itp_log_keys(None) == {}
    assert report.itp_summary_line(res["delta_itp"]).startswith("Delta E ITP (pq, bt2020, limited range): ")
    sub = score_files(rp, dp, "vmaf_v0.6.1", delta_itp="pq", n_subsample=2, **kw)
    assert len(sub["metrics"]["delta_e_itp"]) == len(sub["frame_indices"]) and sub["delta_itp"]["summary"]["frames"] == len(ref)
    hlg = score_files(rp, dp, "vmaf_v0.6.1", delta_itp="hlg", itp_peak=600, itp_threshold=2, itp_range="full", **kw)
    sp = hlg["delta_itp"]["spec"]
    assert (sp["transfer"], sp["matrix"], sp["range"], sp["peak"], sp["threshold"]) == ("hlg", "bt2020", "full", 600.0, 2.0)
    sdr = score_files(rp, dp, "vmaf_v0.6.1", delta_itp="bt1886", **kw)
    assert (sdr["delta_itp"]["spec"]["matrix"], sdr["delta_itp"]["spec"]["peak"]) == ("bt601", 100.0)     # 32 lines: by the height
    assert score_files(rp, dp, "vmaf_v0.6.1", delta_itp="bt1886", itp_matrix="bt709", **kw)["delta_itp"]["spec"]["primaries"] == "bt709"
    for bad in (dict(delta_itp="srgb"), dict(delta_itp="pq", itp_range="tv"), dict(delta_itp="pq", itp_matrix="xyz"),
                dict(delta_itp="hlg", itp_peak=-5), dict(delta_itp="pq", itp_threshold=-1)):
        with pytest.raises(ValueError):
            score_files(rp, dp, "vmaf_v0.6.1", **bad, **kw)


def test_range_follows_the_header_and_monochrome_is_refused(tmp_path):
    from pqa2_amd.pipeline import score_files
    (tmp_path / "f").mkdir()
    rp, dp, _, _ = _write(tmp_path / "f", n=2, full=True)
    res = score_files(rp, dp, "vmaf_v0.6.1", delta_itp="pq", engine_factory=_itp_engine())
    assert res["delta_itp"]["spec"]["range"] == "full"
    (tmp_path / "m").mkdir()
    rp, dp, _, _ = _write(tmp_path / "m", n=2, mono=True)
    with pytest.raises(ValueError, match="monochrome"):
        score_files(rp, dp, "vmaf_v0.6.1", delta_itp="pq", engine_factory=_itp_engine())


def test_command_line_passes_the_options_on(tmp_path, monkeypatch):
    from pqa2_amd import pipeline, score
    seen = []

    def fake(*a, **kw):
        seen.append(kw)
        raise RuntimeError("stop")

    monkeypatch.setattr(pipeline, "score_files", fake)
    monkeypatch.setattr(score, "_die_with_parent", lambda *a, **k: None)
    base = ["r.y4m", "d.y4m", "--json", str(tmp_path / "x.json")]
    score.main(base)
    score.main(base + ["--delta-itp", "pq"])
    score.main(base + ["--delta-itp", "hlg", "--itp-matrix", "bt2020", "--itp-range", "full", "--itp-peak", "600", "--itp-threshold", "2"])
    score.main(base + ["--itp-peak", "600"])      # without --delta-itp nothing is passed on

    def ours(kw):
        return {k: v for k, v in kw.items() if k.startswith("itp") or k == "delta_itp"}
    assert not ours(seen[0]) and not ours(seen[3])
    assert ours(seen[1]) == {"delta_itp": "pq", "itp_matrix": None, "itp_range": None, "itp_peak": None, "itp_threshold": 1.0}
    assert ours(seen[2]) == {"delta_itp": "hlg", "itp_matrix": "bt2020", "itp_range": "full", "itp_peak": 600.0, "itp_threshold": 2.0}
    with pytest.raises(SystemExit):
        score.main(base + ["--delta-itp", "srgb"])


def test_analyzer_attributes_results_and_child_argv(tmp_path, monkeypatch):
    from pqa2_amd import vmaf_analyzer as V
    rp, dp, _, _ = _write(tmp_path, n=3)
    a = V.VMAFAnalyzer()
    assert a.delta_itp is None and a.itp_matrix is None and a.itp_peak is None
    a.set_output_directory(str(tmp_path))
    a._engine_factory = _itp_engine()
    res = a.analyze_videos(rp, dp)
    assert res is not None and "delta_itp" not in res
    a.delta_itp, a.itp_peak = "hlg", 800
    lines = []
    a.status_update.connect(lines.append)
    res = a.analyze_videos(rp, dp)
    assert res is not None and res["delta_itp"]["spec"]["transfer"] == "hlg" and res["delta_itp"]["spec"]["peak"] == 800.0
    assert any(line.startswith("Delta E ITP (hlg") for line in lines)
    log = json.load(open(res["json_path"]))
    assert "delta_e_itp" in log["frames"][0]["metrics"] and "delta_itp" in log
    cmds = []

    class FakePopen:
        def __init__(self, cmd, **kw):
            cmds.append(list(cmd))
            self.stderr, self.returncode, self.pid = iter(()), 1, 0

        def wait(self, timeout=None):
            return 1

        def poll(self):
            return 1

    monkeypatch.setattr(V.subprocess, "Popen", FakePopen)
    b = V.VMAFAnalyzer()
    b.gpus = 2
    b._run_child_job(rp, dp, "vmaf_v0.6.1", "j.json", None, None, 3)
    b.delta_itp, b.itp_matrix, b.itp_peak = "bt1886", "bt709", 120
    b._run_child_job(rp, dp, "vmaf_v0.6.1", "j.json", None, None, 3)
    assert "--delta-itp" not in cmds[0]
    i = cmds[1].index("--delta-itp")
    assert cmds[1][i:i + 6] == ["--delta-itp", "bt1886", "--itp-matrix", "bt709", "--itp-peak", "120.0"]


# ---- the C ABI --------------------------------------------------------------------------------------------------------
def test_header_and_exports():
    from pqa2_amd import _native as N
    hdr = open(os.path.join(ROOT, "include", "pqa_vmaf.h")).read()
    for sym in ("pqa_itp_sums", "pqa_delta_itp", "pqa_delta_itp_device", "pqa_debug_itp"):
        assert re.search(r"PQA_API\s+int\s+" + sym + r"\s*\(", hdr) and sym in N.EXPORTS
    for name, val in (("PQA_ITP_PQ", N.ITP_PQ), ("PQA_ITP_HLG", N.ITP_HLG), ("PQA_ITP_BT1886", N.ITP_BT1886)):
        assert int(re.search(name + r"\s*=\s*(\d+)", hdr).group(1)) == val
    struct = hdr[hdr.index("typedef struct pqa_itp_spec {"):hdr.index("} pqa_itp_spec;")]
    fields = re.findall(r"^\s*(?:uint32_t|float)\s+(\w+)", struct, re.M)
    assert fields == [n for n, _ in N.PqaItpSpec._fields_]
    import ctypes as C
    assert C.sizeof(N.PqaItpSpec) == 4 * (1 + 12 + 9 + 2)
    lib = N.load()
    assert lib.pqa_itp_sums() == N.ITP_SUMS == 8
    assert lib.pqa_debug_itp(None, None, 0, None) == N.PQA_EINVAL
    bad = N.PqaItpSpec()
    bad.transfer = 7
    assert lib.pqa_debug_itp(C.byref(bad), None, 0, None) == N.PQA_EINVAL and b"unknown transfer" in lib.pqa_last_error(None)
