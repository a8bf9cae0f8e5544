"""BASELINE.json configs at FULL size under the driver's `-m gpu` run (VERDICT r1 "configs not exercised"):

  configs[2]  2160p 8-bit  vmaf_4k_v0.6.1          -> one frame pair against the oracle
  configs[4]  2160p 10-bit vmaf_v0.6.1neg + PSNR + SSIM on all planes (4:2:0)
              -> size-independent properties + one frame pair against the oracle (u16 kernels at 4K)

plus the C-ABI call-sequence promises of include/pqa_vmaf.h (PQA_ESTATE) and piecewise collection
while later batches are still running.  Tolerances as in test_gpu_parity.py: features 5e-5 relative
(f32 kernels vs the f32 restatement), SSE bit-exact, SSIM 1e-9, VMAF 0.01.
"""
import numpy as np
import pytest

from pqa2_amd import model as M

pytestmark = pytest.mark.gpu

REL_TOL = 5e-5
VMAF_TOL = 0.01
W4K, H4K = 3840, 2160


def _planes_host(clip, key, i, bpc):
    out = []
    for t in clip[key]:
        a = t[i].cpu().numpy()
        out.append(a.view(np.uint16) if bpc > 8 else a)
    return out


def _resident_args(clip, key, es):
    ts = clip[key]
    return ([t.data_ptr() for t in ts], [t.shape[2] * es for t in ts], [t.shape[1] * t.shape[2] * es for t in ts])


def test_config_2160p_8bit_frame_pair_against_oracle(oracle32):
    """BASELINE configs[2]: 3840x2160 8-bit, vmaf_4k_v0.6.1 (integer border), two frames vs the oracle."""
    import torch
    from pqa2_amd import synth_torch
    from pqa2_amd.engine import FeatureEngine
    mdl = M.load_model("vmaf_4k_v0.6.1")
    n = 2
    clip = synth_torch.make_clip_cuda(W4K, H4K, n, 8, device="cuda")
    torch.cuda.synchronize()
    rp, rpitch, fpitch = _resident_args(clip, "ref", 1)
    dp, _, _ = _resident_args(clip, "dis", 1)
    with FeatureEngine(W4K, H4K, vif_border=mdl.vif_border, vif_enhn_gain_limit=mdl.vif_enhn_gain_limit,
                       adm_enhn_gain_limit=mdl.adm_enhn_gain_limit) as eng:
        eng.submit_resident(0, n, rp, dp, rpitch, fpitch)
        got = eng.collect(0, n)
    refs = [_planes_host(clip, "ref", i, 8)[0] for i in range(n)]
    diss = [_planes_host(clip, "dis", i, 8)[0] for i in range(n)]
    exp = oracle32.clip_features_mt(refs, diss, 8, 2, vif_border101=bool(mdl.vif_border))
    rel = np.abs(got[:, :16] - exp[:, :16]) / np.maximum(np.abs(exp[:, :16]), 1e-12)
    assert rel.max() < REL_TOL, rel.max()
    assert abs(got[1, 16] - exp[1, 16]) < 5e-6 * exp[1, 16] + 2e-5 and got[0, 16] == 0.0
    rec = np.zeros((n, 24)); rec[:, :17] = exp
    v_exp = M.score_frames(mdl, M.metrics_from_records(rec, W4K, H4K, "integer_"))["vmaf"]
    v_got = M.score_frames(mdl, M.metrics_from_records(got, W4K, H4K, "integer_"))["vmaf"]
    assert np.abs(v_exp - v_got).max() <= VMAF_TOL


def test_config_2160p_10bit_neg_psnr_ssim_all_planes(oracle32):
    """BASELINE configs[4]: 3840x2160 10-bit 4:2:0, vmaf_v0.6.1neg (both gain limits 1.0, models/vmaf_v0.6.1neg.json
    :34-51), PSNR + SSIM on Y, U, V.  Properties at full size, then two frames against the oracle."""
    import torch
    from pqa2_amd import _native as N
    from pqa2_amd import synth_torch
    from pqa2_amd.engine import FeatureEngine, sse_from_records
    mdl = M.load_model("vmaf_v0.6.1neg")
    assert mdl.vif_enhn_gain_limit == 1.0 and mdl.adm_enhn_gain_limit == 1.0
    bpc, es, n = 10, 2, 3
    w, h = W4K, H4K
    cw, ch = w // 2, h // 2
    clip = synth_torch.make_clip_cuda(w, h, n, bpc, device="cuda", chroma=True)
    torch.cuda.synchronize()
    rp, rpitch, fpitch = _resident_args(clip, "ref", es)
    dp, _, _ = _resident_args(clip, "dis", es)
    kw = dict(bit_depth=bpc, n_planes=3, features=N.FEAT_ALL, vif_border=mdl.vif_border,
              vif_enhn_gain_limit=1.0, adm_enhn_gain_limit=1.0)
    with FeatureEngine(w, h, max_batch=2, **kw) as eng:
        eng.submit_resident(0, n, rp, rp, rpitch, fpitch)                      # identical
        ident = eng.collect(0, n)
        eng.reset()
        eng.submit_resident(0, n, rp, dp, rpitch, fpitch)                      # the real pair
        pair = eng.collect(0, n)
        static = [t[:1].expand(n, *t.shape[1:]).contiguous() for t in clip["ref"]]
        sp = [t.data_ptr() for t in static]
        torch.cuda.synchronize()   # the context runs on its own stream: torch's copies must have landed
        eng.reset()
        eng.submit_resident(0, n, sp, sp, rpitch, fpitch)                      # static
        stat = eng.collect(0, n)
        c = 5
        lo = [t.to(torch.int32).clamp(0, 1023 - c).to(torch.int16) for t in clip["ref"]]
        hi = [(t.to(torch.int32) + c).to(torch.int16) for t in lo]
        torch.cuda.synchronize()
        eng.reset()
        eng.submit_resident(0, n, [t.data_ptr() for t in lo], [t.data_ptr() for t in hi], rpitch, fpitch)
        off = eng.collect(0, n)
    np.testing.assert_allclose(ident[:, 0:4] / ident[:, 4:8], 1.0, atol=2e-5)
    np.testing.assert_allclose(ident[:, 8:12] / ident[:, 12:16], 1.0, atol=1e-6)
    assert np.all(sse_from_records(ident) == 0) and np.allclose(ident[:, 17:20], 1.0)
    assert np.all(stat[:, 16] == 0.0) and pair[0, 16] == 0.0 and np.all(pair[1:, 16] > 0)
    want_sse = np.array([c * c * w * h, c * c * cw * ch, c * c * cw * ch], np.uint64)
    assert np.all(sse_from_records(off) == want_sse[None, :])
    # the neg model's gain limit: a contrast-enhanced copy may not score above the reference itself
    assert np.all(pair[:, 0:4] <= pair[:, 4:8] * (1 + 1e-6))
    # host path over the same bytes == resident path, bit for bit (u16 staging, three planes, 2160p)
    with FeatureEngine(w, h, max_batch=3, **kw) as eng:
        for i in range(n):
            eng.submit(i, _planes_host(clip, "ref", i, bpc), _planes_host(clip, "dis", i, bpc))
        host = eng.collect(0, n)
    assert np.array_equal(host.view(np.uint64), pair.view(np.uint64))
    # two frames against the oracle: u16 VIF / ADM / motion at 4K, SSE exact, SSIM of all planes
    m = 2
    refs = [_planes_host(clip, "ref", i, bpc) for i in range(m)]
    diss = [_planes_host(clip, "dis", i, bpc) for i in range(m)]
    exp = oracle32.clip_features_mt([r[0] for r in refs], [d[0] for d in diss], bpc, 2, vif_gain_limit=1.0,
                                    adm_gain_limit=1.0, vif_border101=bool(mdl.vif_border))
    rel = np.abs(pair[:m, :16] - exp[:, :16]) / np.maximum(np.abs(exp[:, :16]), 1e-12)
    assert rel.max() < REL_TOL, rel.max()
    assert abs(pair[1, 16] - exp[1, 16]) < 5e-6 * exp[1, 16] + 2e-5
    sse = sse_from_records(pair)
    for i in range(m):
        for p in range(3):
            assert int(sse[i, p]) == oracle32.sse_plane(diss[i][p], refs[i][p], bpc)
            assert abs(pair[i, 17 + p] - oracle32.ssim_plane(diss[i][p], refs[i][p], bpc)) < 1e-9
    rec = np.zeros((m, 24)); rec[:, :17] = exp
    v_exp = M.score_frames(mdl, M.metrics_from_records(rec, w, h, "integer_"))["vmaf"]
    v_got = M.score_frames(mdl, M.metrics_from_records(pair[:m], w, h, "integer_"))["vmaf"]
    assert np.abs(v_exp - v_got).max() <= VMAF_TOL


# ---- C-ABI call-sequence promises (include/pqa_vmaf.h: PQA_ESTATE) ---------------------------------------------
def _small_clip(n, w=96, h=64):
    from pqa2_amd import synth
    return synth.make_clip(w, h, n, 8, chroma=False)


def test_collect_of_a_never_submitted_frame_is_estate():
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    refs, diss = _small_clip(3)
    with FeatureEngine(96, 64, max_batch=2, result_capacity=8) as eng:
        with pytest.raises(N.PqaError) as e:
            eng.collect(0, 1)                       # nothing submitted at all
        assert e.value.code == N.PQA_ESTATE and "never submitted" in str(e.value)
        for i in range(3):
            eng.submit(i, refs[i], diss[i])
        with pytest.raises(N.PqaError) as e:
            eng.collect(2, 2)                       # frame 3 was never submitted
        assert e.value.code == N.PQA_ESTATE
        assert eng.collect(0, 3).shape == (3, 24)   # the context is still usable
        eng.reset()
        with pytest.raises(N.PqaError) as e:        # reset starts a new clip: old records are gone
            eng.collect(0, 1)
        assert e.value.code == N.PQA_ESTATE


def test_overwriting_an_uncollected_record_is_estate():
    import torch
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    n, w, h = 6, 96, 64
    refs, diss = _small_clip(n, w, h)
    with FeatureEngine(w, h, max_batch=2, result_capacity=4) as eng:    # ring of 4 records
        for i in range(4):
            eng.submit(i, refs[i], diss[i])
        with pytest.raises(N.PqaError) as e:
            eng.submit(4, refs[4], diss[4])         # slot 0 still holds the uncollected record of frame 0
        assert e.value.code == N.PQA_ESTATE and "uncollected" in str(e.value)
        first = eng.collect(0, 2)                   # frees slots 0 and 1
        eng.submit(4, refs[4], diss[4])
        eng.submit(5, refs[5], diss[5])
        rest = eng.collect(2, 4)
        with pytest.raises(N.PqaError) as e:        # frame 0's record has been replaced by frame 4's
            eng.collect(0, 1)
        assert e.value.code == N.PQA_ESTATE
        eng.submit(1, refs[1], diss[1])             # the SAME index again (a re-run) is not an overwrite
    with FeatureEngine(w, h, max_batch=4, result_capacity=16) as eng:
        for i in range(n):
            eng.submit(i, refs[i], diss[i])
        full = eng.collect(0, n)
    assert np.array_equal(np.concatenate([first, rest]).view(np.uint64), full.view(np.uint64))
    # device-resident submit: the same rule, checked per batch before anything is launched
    R = torch.from_numpy(np.stack([r[0] for r in refs])).cuda()
    D = torch.from_numpy(np.stack([d[0] for d in diss])).cuda()
    torch.cuda.synchronize()
    with FeatureEngine(w, h, max_batch=2, result_capacity=4) as eng:
        eng.submit_resident(0, 4, [R.data_ptr()], [D.data_ptr()], [w], [w * h])
        with pytest.raises(N.PqaError) as e:
            eng.submit_resident(4, 2, [R[4:].data_ptr()], [D[4:].data_ptr()], [w], [w * h], R[3].data_ptr(), w)
        assert e.value.code == N.PQA_ESTATE
        got = eng.collect(0, 4)
        eng.submit_resident(4, 2, [R[4:].data_ptr()], [D[4:].data_ptr()], [w], [w * h], R[3].data_ptr(), w)
        got = np.concatenate([got, eng.collect(4, 2)])
    assert np.array_equal(got.view(np.uint64), full.view(np.uint64))


def test_estate_launches_and_loses_nothing():
    """`PQA_ESTATE: nothing is launched or overwritten` on the two paths that did not keep it.
    (1) pqa_submit_device with more frames than one batch: a collision in a LATER batch must be found before the first
    batch is launched.  (2) pqa_submit of a non-consecutive index while earlier frames are still pending: the pending
    frames are flushed (claim their slots) first, so the check sees them, and they are not dropped."""
    import torch
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    n, w, h = 9, 96, 64
    refs, diss = _small_clip(n, w, h)
    R = torch.from_numpy(np.stack([r[0] for r in refs])).cuda()
    D = torch.from_numpy(np.stack([d[0] for d in diss])).cuda()
    torch.cuda.synchronize()
    with FeatureEngine(w, h, max_batch=n, result_capacity=16) as eng:
        eng.submit_resident(0, n, [R.data_ptr()], [D.data_ptr()], [w], [w * h])
        full = eng.collect(0, n)
    with FeatureEngine(w, h, max_batch=2, result_capacity=6) as eng:
        eng.submit_resident(0, 2, [R.data_ptr()], [D.data_ptr()], [w], [w * h])
        with pytest.raises(N.PqaError) as e:   # frames 4, 5 fit; 6, 7 would land on the uncollected records of 0, 1
            eng.submit_resident(4, 4, [R[4:].data_ptr()], [D[4:].data_ptr()], [w], [w * h], R[3].data_ptr(), w)
        assert e.value.code == N.PQA_ESTATE
        with pytest.raises(N.PqaError) as e:   # ... and the first batch of that call was NOT launched
            eng.collect(4, 2)
        assert e.value.code == N.PQA_ESTATE and "never submitted" in str(e.value)
        assert np.array_equal(eng.collect(0, 2).view(np.uint64), full[:2].view(np.uint64))
    with FeatureEngine(w, h, max_batch=8, result_capacity=8) as eng:     # host path: 8 frames per staging half
        for i in range(4):
            eng.submit(i, refs[i], diss[i])                              # pending, not yet launched
        with pytest.raises(N.PqaError) as e:
            eng.submit(8, refs[8], diss[8])                              # slot 0 = frame 0, pending and uncollected
        assert e.value.code == N.PQA_ESTATE and "uncollected" in str(e.value)
        assert np.array_equal(eng.collect(0, 4).view(np.uint64), full[:4].view(np.uint64))   # nothing was dropped
        eng.submit(8, refs[8], diss[8])                                  # and now it fits
        got8 = eng.collect(8, 1)
    # frame 8 after a gap: its motion has no predecessor in this context (0), everything else is frame 8's own
    assert np.array_equal(got8[:, :16].view(np.uint64), full[8:9, :16].view(np.uint64))


def test_piecewise_collect_while_later_batches_run():
    """pqa_collect(first, count) waits for the batch that produced those records only (per-batch events): collecting
    batch by batch while the rest of a 1080p clip is still in flight returns exactly the records of one final collect."""
    import torch
    from pqa2_amd import synth_torch
    from pqa2_amd.engine import FeatureEngine
    w, h, n, B = 1920, 1080, 24, 4
    clip = synth_torch.make_clip_cuda(w, h, n, 8, device="cuda")
    torch.cuda.synchronize()
    rp, rpitch, fpitch = _resident_args(clip, "ref", 1)
    dp, _, _ = _resident_args(clip, "dis", 1)
    with FeatureEngine(w, h, max_batch=B) as eng:
        eng.submit_resident(0, n, rp, dp, rpitch, fpitch)
        whole = eng.collect(0, n)
        eng.reset()
        eng.submit_resident(0, n, rp, dp, rpitch, fpitch)
        parts = [eng.collect(i, B) for i in range(0, n, B)]          # in order, each waits for its own batch
        eng.reset()
        eng.submit_resident(0, n, rp, dp, rpitch, fpitch)
        back = [eng.collect(i, B) for i in range(n - B, -1, -B)][::-1]  # youngest first: waits for everything at once
    assert np.array_equal(np.concatenate(parts).view(np.uint64), whole.view(np.uint64))
    assert np.array_equal(np.concatenate(back).view(np.uint64), whole.view(np.uint64))


# ---- the N > 1 path with the REAL engine -------------------------------------------------------
def _write_pair(tmp_path, w, h, n, bpc=8):
    from pqa2_amd import synth, yuvio
    refs, diss = synth.make_clip(w, h, n, bpc, chroma=True)
    info = synth.clip_info(w, h, bpc)
    rp, dp = str(tmp_path / "ref.y4m"), str(tmp_path / "dist.y4m")
    yuvio.write_y4m(rp, refs, info)
    yuvio.write_y4m(dp, diss, info)
    return rp, dp


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _strip_fps(path):
    import json
    d = json.load(open(path))
    d.pop("fps", None)       # wall-clock: the only field that legitimately differs between runs
    return json.dumps(d, sort_keys=True)


@pytest.mark.parametrize("ranks,n", [(2, 11), (3, 11), (4, 3)])
def test_torchrun_ranks_share_the_gpu_and_match_single_process(tmp_path, ranks, n):
    """python -m torch.distributed.run --nproc-per-node N -m pqa2_amd.score: N fresh processes, each with its own
    pqa_ctx on the HIP engine (frame shard + one-frame motion halo through pqa_set_motion_halo), records all-gathered
    (gloo here: the ranks share this box's single GPU; RCCL needs one GPU per rank), rank 0 writes JSON + stats files.
    Everything but the wall-clock `fps` field must equal the single-process run byte for byte."""
    import os
    import subprocess
    import sys
    w, h = 320, 180               # 11 frames over 2 / 3 ranks: uneven shards, seams at odd positions; 3 frames over 4
                                  # ranks: one rank's shard is empty
    rp, dp = _write_pair(tmp_path, w, h, n)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root, HSA_ENABLE_IPC_MODE_LEGACY="0")
    outs = {}
    for tag, launcher in (("one", []), ("many", ["-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={ranks}",
                                                  "--master-addr", "127.0.0.1", "--master-port", str(_free_port())])):
        j, ps, ss = (str(tmp_path / f"{tag}.{x}") for x in ("json", "psnr", "ssim"))
        cmd = [sys.executable] + launcher + ["-m", "pqa2_amd.score", rp, dp, "--json", j, "--psnr-log", ps, "--ssim-log", ss,
                                            "--model", "vmaf_v0.6.1", "--batch", "2"]
        if launcher:
            cmd += ["--backend", "gloo", "--share-device"]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[tag] = (j, ps, ss)
    assert _strip_fps(outs["one"][0]) == _strip_fps(outs["many"][0])
    for k in (1, 2):
        assert open(outs["one"][k]).read() == open(outs["many"][k]).read()


def _n_gpus():
    import torch
    return torch.cuda.device_count()     # counting devices does not initialise HIP


@pytest.mark.skipif(_n_gpus() < 2, reason="needs two GPUs: arms itself on a multi-GPU box (the 1-GPU lease skips it)")
def test_two_ranks_on_rccl_one_gpu_each_match_single_process(tmp_path):
    """The real N > 1 transport: torchrun, 2 ranks, --backend nccl (= RCCL), one GPU per
    rank, records all-gathered device to device; JSON (wall-clock `fps` aside), psnr and ssim files byte-equal to the
    single-process run.  Has never run on the builder's one-GPU lease: it skips there and runs wherever two GPUs exist."""
    import os
    import subprocess
    import sys
    rp, dp = _write_pair(tmp_path, 320, 180, 11)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root, HSA_ENABLE_IPC_MODE_LEGACY="0")
    outs = {}
    for tag, launcher in (("one", []), ("two", ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                                                 "--master-addr", "127.0.0.1", "--master-port", str(_free_port())])):
        j, ps, ss = (str(tmp_path / f"{tag}.{x}") for x in ("json", "psnr", "ssim"))
        cmd = [sys.executable] + launcher + ["-m", "pqa2_amd.score", rp, dp, "--json", j, "--psnr-log", ps, "--ssim-log", ss,
                                            "--model", "vmaf_v0.6.1", "--batch", "2"]
        if launcher:
            cmd += ["--backend", "nccl"]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[tag] = (j, ps, ss)
    assert _strip_fps(outs["one"][0]) == _strip_fps(outs["two"][0])
    for k in (1, 2):
        assert open(outs["one"][k]).read() == open(outs["two"][k]).read()


def test_bench_ranks_sharing_the_gpu_score_the_clip_like_one_rank():
    """bench.py's N > 1 step on the one-GPU box (gloo + --share-device; the driver's launch line otherwise): every rank scores
    its own frames batch by batch under its kernels, the last frame of a chunk after the record gather (its motion2 needs the
    next rank's first motion), the scores are gathered.  The pooled score of the 2 x 48- and 3 x 32-frame jobs must equal the
    one-rank run over the same 96-frame clip, and the line must say what the driver reads (n_gpus, weak, frames_total)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root, HSA_ENABLE_IPC_MODE_LEGACY="0")
    common = ["--steps", "2", "--warmup", "1", "--workload", "1080p", "--batch", "20", "--no-cpu-baseline", "--no-other-configs",
              "--no-e2e"]
    lines = {}
    for ranks in (1, 2, 3):
        launcher = [] if ranks == 1 else ["-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={ranks}", "--master-addr",
                                          "127.0.0.1", "--master-port", str(_free_port())]
        cmd = [sys.executable] + launcher + [os.path.join(root, "bench.py"), "--gpus", str(ranks), "--frames", str(96 // ranks)] + common
        if ranks > 1:
            cmd += ["--backend", "gloo", "--share-device"]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines[ranks] = json.loads(r.stdout.strip().splitlines()[-1])
    for ranks in (2, 3):
        d = lines[ranks]
        assert d["n_gpus"] == ranks and d["scaling"] == "weak" and d["config"]["frames_total"] == 96 and d["value"] > 0
        assert d["pooled_vmaf_mean"] == lines[1]["pooled_vmaf_mean"], (ranks, d["pooled_vmaf_mean"], lines[1]["pooled_vmaf_mean"])


def test_bench_plain_line_full_legs_and_dumped_outputs(tmp_path):
    """A plain bench.py run prints the headline alone (no roofline, per-kernel or CPU legs); --full adds the roofline and
    per-kernel times; --dump-outputs writes the last timed step's records and scores, the same in both runs (seeded clip)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root, HSA_ENABLE_IPC_MODE_LEGACY="0")
    common = ["--steps", "3", "--warmup", "1", "--workload", "1080p", "--frames", "40", "--batch", "20"]
    lines = {}
    for tag, extra in (("plain", []), ("full", ["--full", "--no-cpu-baseline"])):
        cmd = [sys.executable, os.path.join(root, "bench.py"), "--dump-outputs", str(tmp_path / tag)] + common + extra
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines[tag] = json.loads(r.stdout.strip().splitlines()[-1])
    plain, full = lines["plain"], lines["full"]
    for d in (plain, full):
        assert d["steps"] == 3 and d["unit"] == "frames/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
        assert d["ms_per_step"] > 0 and abs(d["value"] - 40 * 1e3 / d["ms_per_step"]) <= 1e-2 * d["value"]   # ms rounded to 1 us
    assert not {"roofline", "kernel_ms_per_frame", "cpu_baseline", "libvmaf_side_by_side"} & set(plain)
    assert "roofline" in full and "kernel_ms_per_frame" in full and "libvmaf_side_by_side" in full
    shapes = {"features": (40, 20), "sse": (40, 3), "vmaf": (40,), "pooled": (4,)}
    for name, shape in shapes.items():
        a, b = (np.load(tmp_path / tag / f"{name}.npy") for tag in ("plain", "full"))
        assert a.dtype == np.float64 and a.shape == shape, (name, a.dtype, a.shape)
        np.testing.assert_array_equal(a, b, err_msg=name)
    vmaf = np.load(tmp_path / "plain" / "vmaf.npy")
    assert np.all(np.isfinite(vmaf)) and round(float(vmaf.mean()), 6) == plain["pooled_vmaf_mean"]


@pytest.mark.skipif(_n_gpus() < 2, reason="needs two GPUs: arms itself on a multi-GPU box (the 1-GPU lease skips it)")
def test_bench_two_gpus_on_rccl_prints_a_line():
    """bench.py --gpus 2 exactly as the driver launches it (torch.distributed.run, one rank per GPU, RCCL): one JSON line
    with n_gpus 2, weak scaling, a whole-job value, and the pooled score of the 2 x F-frame clip equal on repeat runs."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--workload", "1080p", "--frames", "64"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["config"]["frames_total"] == 128 and d["value"] > 0
    assert 0.0 < d["pooled_vmaf_mean"] <= 100.0


def test_analyzer_gpus2_child_job_on_one_gpu(tmp_path):
    """VMAFAnalyzer.gpus = 2 end to end (torchrun child with two ranks, progress lines, result dict), rehearsed on this
    one-GPU box with child_backend = gloo + child_share_device; same numbers as the in-process run."""
    from pqa2_amd import VMAFAnalyzer
    rp, dp = _write_pair(tmp_path, 256, 144, 9)
    a = VMAFAnalyzer()
    a.set_output_directory(str(tmp_path / "single"))
    (tmp_path / "single").mkdir()
    a.set_test_name("t")
    errs = []
    a.error_occurred.connect(errs.append)
    one = a.analyze_videos(rp, dp, "vmaf_v0.6.1")
    assert one is not None and errs == []
    b = VMAFAnalyzer()
    (tmp_path / "double").mkdir()
    b.set_output_directory(str(tmp_path / "double"))
    b.set_test_name("t")
    b.gpus, b.child_backend, b.child_share_device = 2, "gloo", True
    b.error_occurred.connect(errs.append)
    two = b.analyze_videos(rp, dp, "vmaf_v0.6.1")
    assert two is not None and errs == [], errs
    assert two["vmaf_score"] == one["vmaf_score"]
    assert [f["metrics"] for f in two["raw_results"]["frames"]] == [f["metrics"] for f in one["raw_results"]["frames"]]
    assert open(two["psnr_log"]).read() == open(one["psnr_log"]).read()
    assert open(two["ssim_log"]).read() == open(one["ssim_log"]).read()


_RCCL_ONE_RANK = r"""
import os, sys
import numpy as np
import torch, torch.distributed as dist
from pqa2_amd import shard, synth
from pqa2_amd.engine import FeatureEngine
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{sys.argv[1]}", world_size=1, rank=0, device_id=dev)
w, h, n = 192, 108, 5
refs, diss = synth.make_clip(w, h, n, 8, chroma=False)
with FeatureEngine(w, h, max_batch=2) as eng:
    for i in range(n):
        eng.submit(i, refs[i], diss[i])
    local = eng.collect(0, n)
local[:, 20] = np.array([2**63 + 12345, 1, 0, 2**64 - 1, 7], np.uint64).view(np.float64)   # NaN-pattern payloads
full = shard.gather_records(local, n, 1, 0, dev, force_collective=True)      # all_gather_into_tensor on the GPU: RCCL
t = torch.tensor([1.5], dtype=torch.float64, device=dev)
dist.all_reduce(t, op=dist.ReduceOp.MAX)                                      # bench.py's max-over-ranks timing call
dist.barrier()
dist.destroy_process_group()
assert np.array_equal(full.view(np.uint64), local.view(np.uint64)), "records changed in the RCCL gather"
assert float(t.item()) == 1.5
print("rccl-one-rank ok")
"""


def test_rccl_gather_of_device_records_with_one_rank(tmp_path):
    """init_process_group("nccl") (= RCCL), the int64 all_gather_into_tensor of shard.gather_records on a DEVICE tensor,
    bench.py's all_reduce(MAX) and barrier -- with the one rank this box can host.  More ranks need more GPUs: the
    driver's 8-GPU SCALE run is the only place RCCL carries data between devices."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-c", _RCCL_ONE_RANK, str(_free_port())], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "rccl-one-rank ok" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])


# ---- VIF scale 0 on the matrix cores (vif_s0_march_kernel) vs the VALU kernel and the oracle -----------------------
@pytest.mark.parametrize("w,h,bpc", [(488, 40, 8), (489, 41, 8), (736, 48, 8), (1000, 200, 8), (1281, 721, 8), (1920, 1080, 8),
                                     (64, 48, 10), (489, 41, 10), (1000, 200, 10), (1920, 1080, 10),
                                     (64, 48, 12), (489, 41, 12), (1000, 200, 12), (1920, 1080, 12)])
def test_vif_mfma_path_matches_valu_path_and_oracle(oracle32, w, h, bpc):
    """Scale 0 on the matrix cores against the VALU kernel and the oracle: the march kernel (vif_march.hip: first pass on
    exact integer digit planes x two-piece (22-bit) taps, second pass on two-piece f16 splits of the f32 intermediates), 8, 10
    and -- since round 4's last session -- 12 bit (centred samples and the cross term's high digit as sign-magnitude patterns).  Geometries from 64 x 48 up to 1080p, odd sizes included.  The paths must agree far inside the oracle bar,
    PQA_VIF_MFMA=0 (read at pqa_create) must really switch the path off, and a caller pitch the wide loads cannot take
    (odd) must not change a bit: the march kernel then loads sample by sample.  (The round-2 kernel that was this test's
    third party until round 3 left the build: tools/experiments/vif_s0_mfma_round2.hip.txt.)"""
    import os
    import torch
    from pqa2_amd import synth
    from pqa2_amd.engine import FeatureEngine
    from pqa2_amd import _native as N
    n = 2
    refs, diss = synth.make_clip(w, h, n, bpc, chroma=False)
    if bpc > 8:   # the extremes of the sample range in both clips: digit planes at their limits (0 -> -512, 1023 -> 511;
        top = (1 << bpc) - 1   # 12 bit: 0 -> -2048 whose square 2^22 is the one high digit of 2048, 4095 -> 2047)
        refs[0][0][:4, :8] = 0; diss[0][0][:4, :8] = top
        refs[1][0][-3:, -9:] = top; diss[1][0][-3:, -9:] = top
        refs[1][0][:3, :9] = 0; diss[1][0][:3, :9] = 0
    else:
        refs[0][0][:4, :8] = 0; diss[0][0][:4, :8] = 255
        refs[1][0][-3:, -9:] = 255; diss[1][0][-3:, -9:] = 255

    def run(**kw):
        with FeatureEngine(w, h, bit_depth=bpc, features=N.FEAT_VIF, **kw) as eng:
            for i in range(n):
                eng.submit(i, refs[i], diss[i])
            return eng.collect(0, n)[:, :8]

    old = os.environ.get("PQA_VIF_MFMA")
    try:
        os.environ["PQA_VIF_MFMA"] = "1"
        mfma = run()
        mfma101 = run(vif_border=N.VIF_BORDER_INTEGER)
        os.environ["PQA_VIF_MFMA"] = "0"
        valu = run()
        valu101 = run(vif_border=N.VIF_BORDER_INTEGER)
    finally:
        if old is None:
            os.environ.pop("PQA_VIF_MFMA", None)
        else:
            os.environ["PQA_VIF_MFMA"] = old
    assert not np.array_equal(mfma.view(np.uint64), valu.view(np.uint64)), "the switch did not change the path"
    rel = np.abs(mfma - valu) / np.abs(valu)
    assert rel.max() < 2e-6, rel.max()
    assert (np.abs(mfma101 - valu101) / np.abs(valu101)).max() < 2e-6
    assert np.all(np.isfinite(mfma))
    exp = oracle32.clip_features([r[0] for r in refs], [d[0] for d in diss], bpc)[:, :8]
    assert (np.abs(mfma - exp) / np.abs(exp)).max() < REL_TOL
    # device-resident clip with an ODD row pitch: 16-bit loads are not possible, the launcher must fall back
    if w % 2 == 0:
        pitch = w + 1
        es = 1 if bpc <= 8 else 2
        tdt = torch.uint8 if bpc <= 8 else torch.int16
        R = torch.zeros((n, h, pitch), dtype=tdt, device="cuda")
        D = torch.zeros((n, h, pitch), dtype=tdt, device="cuda")
        R[:, :, :w] = torch.from_numpy(np.stack([r[0] for r in refs]).view(np.int16 if bpc > 8 else np.uint8)).cuda()
        D[:, :, :w] = torch.from_numpy(np.stack([d[0] for d in diss]).view(np.int16 if bpc > 8 else np.uint8)).cuda()
        torch.cuda.synchronize()
        with FeatureEngine(w, h, bit_depth=bpc, features=N.FEAT_VIF) as eng:
            eng.submit_resident(0, n, [R.data_ptr()], [D.data_ptr()], [pitch * es], [pitch * h * es])
            odd = eng.collect(0, n)[:, :8]
        assert np.array_equal(odd.view(np.uint64), mfma.view(np.uint64))


def test_worst_known_hd_flip_case_stays_bounded():
    """The one HD-size pair any fuzz run has produced above the 0.01 VMAF target: 1039 x 913, gain
    limit 1.5, a single ADM scale-3 coefficient's angle test.  Kept as data (tests/flip_cases); the kernels must stay
    within 0.012 of the f64 oracle values stored with it, and every feature but ADM scale 3's numerator within 5e-6."""
    import os
    from pqa2_amd.engine import FeatureEngine
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "flip_cases", "r02_1039x913_k4.npz"))
    w, h, bpc, kind, gain, border = d["tag"]
    w, h = int(w), int(h)
    with FeatureEngine(w, h, vif_enhn_gain_limit=float(gain), adm_enhn_gain_limit=float(gain), vif_border=int(border)) as eng:
        for i in range(2):
            eng.submit(i, [d["ref"][i]], [d["dis"][i]])
        got = eng.collect(0, 2)[:, :17]
    rel = np.abs(got[:, :16] - d["exp"][:, :16]) / np.abs(d["exp"][:, :16])
    others = np.delete(rel, 11, axis=1)
    assert others.max() < 5e-6, others.max()
    mdl = M.load_model("vmaf_v0.6.1")
    def vm(r):
        full = np.zeros((2, 24)); full[:, :17] = r
        return M.score_frames(mdl, M.metrics_from_records(full, w, h))["vmaf"]
    assert np.abs(vm(got) - vm(d["exp"])).max() < 0.012


_ONLY_12_BIT = r"""
import os, sys
import numpy as np
from pqa2_amd import synth, _native as N
from pqa2_amd.engine import FeatureEngine
w, h, n = 320, 180, 2
refs, diss = synth.make_clip(w, h, n, 12, chroma=False)
out = []
for mode in ("1", "0"):
    os.environ["PQA_VIF_MFMA"] = mode
    with FeatureEngine(w, h, bit_depth=12, features=N.FEAT_VIF) as eng:
        for i in range(n):
            eng.submit(i, refs[i], diss[i])
        out.append(eng.collect(0, n)[:, :8])
assert not np.array_equal(out[0].view(np.uint64), out[1].view(np.uint64)), "a 12-bit context alone did not get the march kernel"
assert (np.abs(out[0] - out[1]) / np.abs(out[1])).max() < 2e-6
print("only-12-bit ok")
"""


def test_a_12_bit_context_alone_gets_the_march_kernel():
    """The tap table of the march kernel is uploaded by pqa_create.  It once was only for 8- and 10-bit contexts, so a
    process whose FIRST context was 12 bit silently ran the VALU kernel (and every test passed, because an earlier test had
    created an 8-bit context in the same process).  A fresh process with nothing but a 12-bit context: PQA_VIF_MFMA=0 must
    change the records (by rounding only)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _ONLY_12_BIT], env=dict(os.environ, PYTHONPATH=root), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "only-12-bit ok" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_march_kernel_takes_any_base_alignment_and_pitch_bit_for_bit(bpc):
    """(adm_march_kernel and motion_march_kernel -- two samples per lane and load -- are held to the same: round 4.)
    vif_s0_march_kernel loads 8 samples per lane with one 8 / 16-byte load when bases and pitches allow it and sample by
    sample otherwise (and always for the stripes whose columns are mirrored).  A device-resident clip at base offsets 0..7
    samples into a padded allocation, with an odd pitch, and at widths that are not multiples of 16 must give the very same
    records as the packed, aligned clip -- the arithmetic does not depend on how the samples were fetched."""
    import torch
    from pqa2_amd import _native as N
    from pqa2_amd import synth
    from pqa2_amd.engine import FeatureEngine
    es = 1 if bpc == 8 else 2
    tdt, ndt = (torch.uint8, np.uint8) if bpc == 8 else (torch.int16, np.int16)
    for w, h in ((96, 64), (83, 37), (250, 40)):
        n = 2
        refs, diss = synth.make_clip(w, h, n, bpc, chroma=False)
        R0 = np.stack([r[0] for r in refs]).view(ndt)
        D0 = np.stack([d[0] for d in diss]).view(ndt)

        def run(off, pitch):
            buf_r = torch.zeros(n * h * pitch + 16, dtype=tdt, device="cuda")
            buf_d = torch.zeros(n * h * pitch + 16, dtype=tdt, device="cuda")
            vr = buf_r[off:off + n * h * pitch].view(n, h, pitch)
            vd = buf_d[off:off + n * h * pitch].view(n, h, pitch)
            vr[:, :, :w] = torch.from_numpy(R0).cuda()
            vd[:, :, :w] = torch.from_numpy(D0).cuda()
            torch.cuda.synchronize()
            with FeatureEngine(w, h, bit_depth=bpc, features=N.FEAT_VMAF) as eng:   # the ADM and motion march kernels too
                eng.submit_resident(0, n, [vr.data_ptr()], [vd.data_ptr()], [pitch * es], [pitch * h * es])
                return eng.collect(0, n)[:, :17]
        base = run(0, ((w + 15) // 16) * 16)
        for off, pitch in ((1, w), (3, w + 1), (4, w + 8), (7, ((w + 15) // 16) * 16)):
            got = run(off, pitch)
            assert np.array_equal(got.view(np.uint64), base.view(np.uint64)), (w, h, off, pitch)


# ---- ADM and motion as register-only marches (adm_march.hip, motion_march.hip) vs the LDS-tiled kernels and the oracle ------
@pytest.mark.parametrize("w,h,bpc", [(64, 48, 8), (200, 120, 8), (250, 40, 8), (489, 41, 8), (736, 488, 8), (1039, 913, 8),
                                     (1920, 1080, 8), (322, 182, 10), (1281, 721, 10), (720, 486, 12),
                                     (128, 128, 8), (244, 132, 8), (484, 260, 8), (1280, 720, 10), (248, 516, 12)])
def test_adm_and_motion_march_kernels_match_the_tiled_kernels_and_the_oracle(oracle32, w, h, bpc):
    """The march kernels do the tiled kernels' arithmetic per coefficient / per pixel in the same order and differ only in
    how the partial sums are grouped: they must agree to rounding (1e-6; measured 1e-8), PQA_ADM_MARCH=0 / PQA_MOTION_MARCH=0
    (read at pqa_create) must really switch them off, and both must sit inside the oracle bar.  Geometries: one EDGE stripe
    only, two stripes, a fast stripe between two edge stripes, odd sizes (mirrored last column / row), segment boundaries
    inside and outside the 10 % crop, deep scales down to a few coefficients, 8 / 10 / 12 bit."""
    import os
    from pqa2_amd import synth
    from pqa2_amd.engine import FeatureEngine
    from pqa2_amd import _native as N
    n = 3
    refs, diss = synth.make_clip(w, h, n, bpc, chroma=False)

    def run(**env):
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            with FeatureEngine(w, h, bit_depth=bpc, features=N.FEAT_ADM | N.FEAT_MOTION, max_batch=2) as eng:
                for i in range(n):
                    eng.submit(i, refs[i], diss[i])
                return eng.collect(0, n)[:, 8:17]
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v

    march = run()
    tiled = run(PQA_ADM_MARCH="0", PQA_MOTION_MARCH="0")
    # scales 0 and 1 in one launch (adm_pyramid.hip: taken when width and height are multiples of 4 and >= 128 -- the last
    # five geometries and 736 x 488 / 1920 x 1080: one EDGE stripe only, two stripes, fast stripes between edge stripes, one
    # and several segments, 8 / 10 / 12 bit) against the same kernels one scale per launch
    single = run(PQA_ADM_PYRAMID="0")
    den1 = np.maximum(np.abs(single), 1e-30)
    assert (np.abs(march - single) / den1).max() < 1e-6, (np.abs(march - single) / den1).max()
    assert not np.array_equal(march[:, :8].view(np.uint64), tiled[:, :8].view(np.uint64)), "PQA_ADM_MARCH=0 did not change the path"
    assert not np.array_equal(march[1:, 8].view(np.uint64), tiled[1:, 8].view(np.uint64)), "PQA_MOTION_MARCH=0 did not change the path"
    assert march[0, 8] == 0.0 and tiled[0, 8] == 0.0
    den = np.maximum(np.abs(tiled), 1e-30)
    assert (np.abs(march - tiled) / den).max() < 1e-6, (np.abs(march - tiled) / den).max()
    exp = oracle32.clip_features([r[0] for r in refs], [d[0] for d in diss], bpc)[:, 8:17]
    assert (np.abs(march[:, :8] - exp[:, :8]) / np.abs(exp[:, :8])).max() < REL_TOL
    assert (np.abs(march[:, 8] - exp[:, 8]) / np.maximum(1.0, np.abs(exp[:, 8]))).max() < 2e-5   # the f32 oracle sums a plane in f32
