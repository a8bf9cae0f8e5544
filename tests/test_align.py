"""Temporal alignment without a GPU: the C ABI of pqa_cross_sse / pqa_cross_sse_device (declarations, exports, argument
rules), the numpy restatement against a brute force, the premise of the planted clips the GPU tests use, align.best_offset
and align.frame_map (the latter against an exhaustive enumeration), and pipeline.score_files(align=K) on a stand-in
engine."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

from tests import align_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- ABI --------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_exports_both_calls():
    from pqa2_amd import _native as N
    src = open(os.path.join(ROOT, "include", "pqa_vmaf.h")).read()
    for name in ("pqa_cross_sse", "pqa_cross_sse_device"):
        assert re.search(r"PQA_API\s+int\s+" + name + r"\s*\(", src), name
        assert name in N.EXPORTS
    assert int(re.search(r"PQA_PROF_KERNELS\s*=\s*(\d+)", src).group(1)) == 17 == N.PROF_KERNELS
    assert "1u << 7" not in src   # bit 7 stays unassigned, and no PQA_FEAT_* bit was added for alignment
    assert N.FEAT_KNOWN == 0x3FF7F   # the known mask of the parent


def test_argument_rules_need_no_device():
    from pqa2_amd import _native as N
    if not os.path.exists(N.LIB_PATH):
        N.build()
    lib = N.load()
    assert lib.pqa_profile_kernel_name(16) and not lib.pqa_profile_kernel_name(17)
    buf = (C.c_uint8 * 64)()
    p = C.addressof(buf)
    ptrs = (C.c_void_p * 4)(p, p, p, p)
    out = (C.c_uint64 * 1024)()

    def dev(ref=p, n_ref=2, dis=p, n_dis=2, k_lo=-1, k_hi=1, o=out):
        return lib.pqa_cross_sse_device(None, ref, 16, 256, n_ref, dis, 16, 256, n_dis, k_lo, k_hi, o)

    def host(ref=ptrs, n_ref=2, dis=ptrs, n_dis=2, k_lo=-1, k_hi=1, o=out):
        return lib.pqa_cross_sse(None, ref, 16, n_ref, dis, 16, n_dis, k_lo, k_hi, o)
    lib.pqa_last_error.restype = C.c_char_p
    before = lib.pqa_last_error(None)
    for call in (dev, host):   # a null context answers before any rule: PQA_EINVAL, and no message of this thread is touched
        for kw in (dict(ref=None), dict(dis=None), dict(o=None), dict(n_ref=-1), dict(n_dis=-1), dict(k_lo=2, k_hi=1),
                   dict(k_lo=-65, k_hi=0), dict(k_lo=0, k_hi=65), dict(k_lo=-100, k_hi=100), dict()):
            assert call(**kw) == N.PQA_EINVAL, kw
            assert lib.pqa_last_error(None) == before, kw
    # the wording of each rule, which needs a context: tests/test_gpu_align.py::test_argument_rules_speak


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def test_restatement_against_brute_force():
    rng = np.random.default_rng(1)
    for bpc in (8, 12):
        ref = [rng.integers(0, 1 << bpc, (5, 7)).astype(np.uint16) for _ in range(4)]
        dis = [rng.integers(0, 1 << bpc, (5, 7)).astype(np.uint16) for _ in range(6)]
        got = R.cross_sse(ref, dis, -2, 3)
        assert got.shape == (4, 6) and got.dtype == np.uint64
        for i, c in itertools.product(range(4), range(6)):
            j = i - 2 + c
            want = sum((int(a) - int(b)) ** 2 for a, b in zip(ref[i].ravel(), dis[j].ravel())) if 0 <= j < 6 else (1 << 64) - 1
            assert int(got[i, c]) == want
    assert int(R.cross_sse(ref, dis, -2, 3)[0, 0]) == (1 << 64) - 1 and int(R.SENTINEL) == (1 << 64) - 1


def test_generator_retimes_as_documented():
    assert R.shown(5, 2) == [None, None, 0, 1, 2, 3, 4]
    assert R.shown(5, -2) == [2, 3, 4]
    assert R.shown(12, 0, repeats=(4, 9), drops=(6, 7)) == [0, 1, 2, 3, 3, 4, 5, 8, 9, 9, 10, 11]
    ref, dis = R.planted_clip(8, 4, 10, 5, 1, seed=3)
    assert len(dis) == 6 and dis[0].dtype == np.uint16 and max(int(d.max()) for d in dis) <= 1023
    assert all(np.abs(dis[i + 1].astype(int) - ref[i].astype(int)).max() <= 1 for i in range(5))


@pytest.mark.parametrize("name", sorted(R.GPU_CLIPS))
def test_premise_of_the_planted_clips(name):
    """the true offset's mean is at least 10 times below every other offset's: a GPU failure cannot be blamed on the input"""
    ref, dis, (k_lo, k_hi) = R.gpu_clip(name)
    true_k = R.GPU_CLIPS[name][0]["offset"]
    D = R.cross_sse(ref, dis, k_lo, k_hi)
    means = {}
    for c in range(D.shape[1]):
        v = [int(x) for x in D[:, c] if x != R.SENTINEL]
        if v:
            means[k_lo + c] = sum(v) / len(v)
    assert true_k in means
    for k, m in means.items():
        if k != true_k:
            assert m >= 10 * means[true_k], (k, m, means[true_k])


# ---- best_offset ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [-3, 0, 5])
def test_best_offset_finds_the_planted_offset(offset):
    from pqa2_amd import align as AL
    ref, dis = R.planted_clip(24, 10, 8, 16, offset, seed=40 + offset)
    D = R.cross_sse(ref, dis, -6, 6)
    k, mse, conf = AL.best_offset(D, 240)
    assert k == offset and mse < 1.0 and conf > 100
    assert AL.best_offset(D, 240, k_lo=-6, n_dis=len(dis))[0] == offset


def test_best_offset_tie_min_overlap_and_confidence():
    from pqa2_amd import align as AL
    S = (1 << 64) - 1
    # 4 reference and 4 captured frames, band -1 ... 1: rows valid as the clip edges say
    D = np.array([[S, 8, 4], [4, 8, 4], [4, 8, 4], [4, 8, S]], np.uint64)
    k, mse, conf = AL.best_offset(D, 2)
    assert (k, mse, conf) == (-1, 2.0, 1.0)            # -1 and +1 tie at mean 4: the negative one; second best is the tie
    D2 = D.copy()
    D2[:, 1] = 4
    assert AL.best_offset(D2, 2)[0] == 0                 # a three-way tie: the smaller |k|
    # one row of offset +1 is a perfect match, but it overlaps too little under the default rule (half of 4 frames = 2)
    D3 = np.array([[S, 8, S], [4, 8, S], [4, 8, S], [4, 8, 0]], np.uint64)
    assert AL.best_offset(D3, 2, n_dis=4)[0] == -1
    assert AL.best_offset(D3, 2, min_overlap=1, n_dis=4)[0] == 1
    with pytest.raises(ValueError):
        AL.best_offset(D3, 2, min_overlap=5)
    D4 = D.copy()
    D4[:, 1] = 0
    k, mse, conf = AL.best_offset(D4, 2)
    assert (k, mse) == (0, 0.0) and conf == float("inf")
    assert AL.best_offset(np.array([[6, 3]], np.uint64), 1, k_lo=0) == (1, 3.0, 2.0)
    with pytest.raises(ValueError):
        AL.best_offset(np.array([[6, 3]], np.uint64), 1)   # an even band needs k_lo


# ---- frame_map ------------------------------------------------------------------------------------------------------------------
def _exhaustive(D, n_dis, k_lo, P):
    """every legal path, its cost by the definition; the winner under the documented tie rule"""
    from pqa2_amd import align as AL
    span = D.shape[1]
    best = None
    for path in itertools.product(range(k_lo, k_lo + span), repeat=n_dis):
        cost = AL.path_cost(D, list(path), 1, P, k_lo=k_lo)
        if cost is None:
            continue
        own = 0   # the definition once more, independently of path_cost
        for j, k in enumerate(path):
            own += int(D[j - k, k - k_lo])
            if j and k != path[j - 1]:
                own += P * (1 if k == path[j - 1] + 1 else path[j - 1] - k)
        assert own == cost
        key = (cost, [(abs(k), k) for k in reversed(path)])
        if best is None or key < best[0]:
            best = (key, path)
    return best


@pytest.mark.parametrize("seed", range(12))
def test_frame_map_against_exhaustive_enumeration(seed):
    from pqa2_amd import align as AL
    rng = np.random.default_rng(seed)
    n_dis, n_ref = int(rng.integers(1, 7)), int(rng.integers(2, 7))
    hi = 4 if seed % 3 == 0 else 1000          # small costs: plenty of ties, so the tie rule is exercised too
    P = int(rng.integers(0, hi))
    D = rng.integers(0, hi, (n_ref, 3)).astype(np.uint64)
    for i, c in itertools.product(range(n_ref), range(3)):
        if not 0 <= i - 1 + c < n_dis:
            D[i, c] = R.SENTINEL
    want = _exhaustive(D, n_dis, -1, P)
    if want is None:
        with pytest.raises(ValueError):
            AL.frame_map(D, n_dis, P, 1)
        return
    ref_index, repeated, dropped = AL.frame_map(D, n_dis, P, 1)
    path = [j - r for j, r in enumerate(ref_index)]
    assert AL.path_cost(D, path, 1, P, k_lo=-1) == want[0][0]
    assert tuple(path) == want[1]
    assert repeated == [j for j in range(1, n_dis) if ref_index[j] == ref_index[j - 1]]
    assert dropped == [r for j in range(1, n_dis) for r in range(ref_index[j - 1] + 1, ref_index[j])]


@pytest.mark.parametrize("bpc", [8, 10])
def test_frame_map_finds_planted_repeats_and_drops(bpc):
    from pqa2_amd import align as AL
    ref, dis = R.planted_clip(24, 10, bpc, 14, 0, repeats=(4, 9), drops=(6, 7), seed=5)
    D = R.cross_sse(ref, dis, -3, 3)
    ref_index, repeated, dropped = AL.frame_map(D, len(dis), n_pixels=240, bit_depth=bpc)
    assert repeated == [4, 9] and dropped == [6, 7]
    assert ref_index == R.shown(14, 0, (4, 9), (6, 7))
    assert AL.default_penalty(240, 10) == 16 * AL.default_penalty(240, 8)
    with pytest.raises(ValueError):   # captured frame 0 has no reference frame under offsets 2 ... 3
        AL.frame_map(D[:, 5:], len(dis), n_pixels=240, k_lo=2)


# ---- score_files(align=K) ---------------------------------------------------------------------------------------------------------
class _TagEngine:
    """Records which frames were paired: every frame's luma carries its clip and frame number in its first samples."""
    made = []

    def __init__(self, width, height, **kw):
        self.kw, self.pairs = kw, {}
        _TagEngine.made.append(self)

    def cross_sse(self, ref_lumas, dis_lumas, k_lo, k_hi):
        return R.cross_sse(ref_lumas, dis_lumas, k_lo, k_hi)

    def set_motion_halo(self, prev):
        self.halo = int(prev[0, 0])

    def submit(self, index, ref_planes, dis_planes):
        self.pairs[index] = (int(ref_planes[0][0, 0]), int(dis_planes[0][0, 0]))

    def collect(self, first, count):
        from pqa2_amd import _native as N
        rec = np.zeros((count, N.RECORD_DOUBLES))
        rec[:, 4:8] = rec[:, 12:16] = 1.0
        for i in range(count):
            rec[i, N.REC_MOTION] = self.pairs[first + i][0] * 100 + self.pairs[first + i][1]
        return rec

    def cancel(self):
        pass

    def close(self):
        pass


def _write_tagged(tmp_path, offset, n=12):
    from pqa2_amd.yuvio import VideoInfo, write_y4m
    ref, dis = R.planted_clip(32, 16, 8, n, offset, seed=60 + offset)
    seq = R.shown(n, offset)
    for i, f in enumerate(ref):
        f[0, 0] = i
    for j, f in enumerate(dis):
        f[0, 0] = 50 + j
    info = VideoInfo(width=32, height=16, fps_num=25, fps_den=1, bit_depth=8, mono=True, hshift=0, vshift=0, chroma_tag="mono")
    rp, dp = str(tmp_path / "ref.y4m"), str(tmp_path / "dis.y4m")
    write_y4m(rp, [[f] for f in ref], info)
    write_y4m(dp, [[f] for f in dis], info)
    return rp, dp, seq


@pytest.mark.parametrize("offset", [3, -2, 0])
def test_score_files_align_pairs_and_shards(tmp_path, offset):
    from pqa2_amd.pipeline import score_files
    rp, dp, seq = _write_tagged(tmp_path, offset)
    n_out = 12 - abs(offset) if offset < 0 else 12
    _TagEngine.made.clear()
    res = score_files(rp, dp, None, psnr=False, ssim=False, engine_factory=_TagEngine, align=4)
    al = res["alignment"]
    assert al["offset_frames"] == offset and al["searched"] == [-4, 4] and al["repeated"] == [] and al["dropped"] == []
    assert al["offset_seconds"] == offset / 25.0 and al["mse"] < 1.0 + 60 ** 2 / 512 and al["confidence"] > 100   # +-1 noise, and the tags differ by at most 60
    scorer = _TagEngine.made[-1]
    assert len(res["records"]) == n_out == len(scorer.pairs)
    for i in range(n_out):   # output frame 0 is the first scored pair; captured frame r + offset shows reference frame r
        r = i + max(0, -offset)
        assert scorer.pairs[i] == (r, 50 + r + offset)
    # two ranks: the same offset on both, the aligned range sharded, the halo is the aligned predecessor
    from pqa2_amd import shard
    for rank in (0, 1):
        _TagEngine.made.clear()
        try:
            score_files(rp, dp, None, psnr=False, ssim=False, engine_factory=_TagEngine, align=4, rank=rank, world_size=2)
        except Exception:
            pass   # the gather needs a process group; the submits have happened by then
        a, b = shard.shard_bounds(n_out, 2, rank)
        scorer = _TagEngine.made[-1]
        assert sorted(scorer.pairs) == list(range(a, b))
        assert scorer.pairs[a] == (a + max(0, -offset), 50 + a + max(0, -offset) + offset)
        if rank:
            assert scorer.halo == a - 1 + max(0, -offset)
    # align_frames limits the search, align=0 is the plain pairing without the key
    assert score_files(rp, dp, None, psnr=False, ssim=False, engine_factory=_TagEngine, align=4,
                       align_frames=6)["alignment"]["offset_frames"] == offset
    plain = score_files(rp, dp, None, psnr=False, ssim=False, engine_factory=_TagEngine)
    assert "alignment" not in plain and _TagEngine.made[-1].pairs[1] == (1, 51)


def test_report_and_analyzer_options():
    from pqa2_amd import report
    from pqa2_amd.vmaf_analyzer import VMAFAnalyzer
    al = {"offset_frames": 3, "offset_seconds": 0.12, "mse": 0.66, "confidence": float("inf"), "repeated": [26],
          "dropped": [], "searched": [-8, 8]}
    line = report.alignment_summary_line(al)
    assert "+3 frames" in line and "1 repeated" in line and "-8 ... 8" in line
    assert report.alignment_log_keys(al)["alignment"]["confidence"] is None
    assert report.alignment_log_keys(None) == {}
    an = VMAFAnalyzer()
    assert an.align_enabled is False and "align" not in an._ssim_family_kwargs()
    an.set_advanced_options(align_enabled=True, align_max_offset=12)
    assert an._ssim_family_kwargs()["align"] == 12

    class Mgr:
        def get_setting(self, name):
            return {"vmaf": {}, "bookend": {"align_enabled": True, "align_max_offset": 5}, "analysis": {"align_max_offset": 7}}[name]
    an = VMAFAnalyzer()
    an.set_options_from_manager(Mgr())
    assert an.align_enabled and an.align_max_offset == 7


def test_analyzer_result_carries_alignment_and_names_the_offset(tmp_path):
    """the result assembly on its own: the JSON's top-level alignment object reaches the result dict and a status line"""
    import json
    from pqa2_amd.vmaf_analyzer import VMAFAnalyzer
    al = {"offset_frames": 3, "offset_seconds": 0.125, "mse": 455.6, "confidence": None, "repeated": [26], "dropped": [],
          "searched": [-8, 8]}
    path = tmp_path / "vmaf.json"
    path.write_text(json.dumps({"version": "x", "frames": [], "pooled_metrics": {"vmaf": {"mean": 12.5}}, "alignment": al}))
    an = VMAFAnalyzer()
    an.set_advanced_options(align_enabled=True)
    lines = []
    an.status_update.connect(lines.append)
    res = an._parse_vmaf_results(str(path), None, None, "dis.y4m", "ref.y4m")
    assert res and res["alignment"] == al
    assert any("offset +3 frames" in s and "exact match" in s for s in lines)
