"""The premises of tests/test_gpu_long_planes.py, on the CPU (tests/long_planes_ref.py has the clips and the sizes).

  1. The f32 oracle stays within 1e-5 of the f64 oracle on every long size, relative and per feature, so the project's rule
     max(REL_TOL, 4 x rel32) (tests/test_gpu_parity.py) leaves the bar at REL_TOL = 5e-5.  (16384 x 128 and 128 x 16384 are
     held against the f64 oracle alone: they cost eight seconds per precision.)
  2. The fixed-point restatement runs on all six sizes: finite records, positive denominators, motion on frames 1 and 2.
  3. The library's own counts (pqa_debug_partial_counts, pqa_debug_vif_march_shape, pqa_debug_adm_need; host arithmetic, the
     library loads without a GPU) at these sizes and at 16384 x 16384: what the launchers report to write fits what the
     workspace sizing functions return, and no count or product leaves `int`.
"""
import ctypes as C

import numpy as np
import pytest

from tests import long_planes_ref as LP

INT_MAX = 2 ** 31 - 1
LIMIT = (16384, 16384, 8)
MAX_BATCH = 4096       # far above any batch pqa_create chooses for frames this large


def _id(s):
    return f"{s[0]}x{s[1]}_{s[2]}bit"


@pytest.mark.parametrize("size", LP.SIZES, ids=_id)
def test_clip_holds_the_extremes_at_the_far_end(size):
    w, h, bpc = size
    refs, diss = LP.clip(w, h, bpc)
    top = (1 << bpc) - 1
    assert len(refs) == len(diss) == LP.N_FRAMES and refs[0].shape == (h, w)
    assert refs[0].dtype == (np.uint8 if bpc == 8 else np.uint16)
    assert np.all(LP.far_end(refs[0], 0, 8) == 0) and np.all(LP.far_end(diss[0], 0, 8) == top)
    assert np.all(LP.far_end(refs[0], 8, 16) == top) and np.all(LP.far_end(diss[0], 8, 16) == top)
    assert np.all(LP.far_end(refs[1], 0, 8) == top) and np.all(LP.far_end(diss[1], 0, 8) == 0)
    # the very last sample of the long axis is part of it
    assert refs[0][-1, -1] == top and refs[1][-1, -1] == 0
    assert max(int(p.max()) for p in refs + diss) <= top


@pytest.mark.parametrize("size", LP.SMALL, ids=_id)
def test_f32_oracle_stays_within_1e5_of_f64(oracle32, oracle64, size):
    w, h, bpc = size
    e64 = LP.oracle_features(oracle64, w, h, bpc)
    e32 = LP.oracle_features(oracle32, w, h, bpc)
    assert np.all(np.isfinite(e64)) and np.all(e64[:, 4:8] > 0) and np.all(e64[:, 12:16] > 0)
    rel32 = LP.rel_features(e32, e64).max(axis=0)
    print(f"\n{_id(size)}: f32 oracle against f64, worst relative distance per feature")
    for name, r in zip(LP.FEATURES, rel32):
        print(f"  {name:11s} {r:.2e}")
    assert rel32.max() < LP.REL32_MAX, (LP.FEATURES[int(rel32.argmax())], float(rel32.max()))
    assert max(LP.REL_TOL, 4.0 * float(rel32.max())) == LP.REL_TOL      # the rule of tests/test_gpu_parity.py: the bar stays
    assert e64[0, 16] == 0.0 and np.all(e64[1:, 16] > 0)
    assert np.abs(e32[:, 16] - e64[:, 16]).max() < LP.MOTION_ATOL + 5e-6 * e64[:, 16].max()


@pytest.mark.parametrize("size", LP.PYRAMID, ids=_id)
def test_f64_oracle_runs_on_the_pyramid_sizes(oracle64, size):
    w, h, bpc = size
    e64 = LP.oracle_features(oracle64, w, h, bpc)
    assert np.all(np.isfinite(e64)) and np.all(e64[:, 4:8] > 0) and np.all(e64[:, 12:16] > 0)
    assert e64[0, 16] == 0.0 and np.all(e64[1:, 16] > 0)


@pytest.mark.parametrize("size", LP.SIZES, ids=_id)
def test_int_oracle_runs_on_every_size(size):
    w, h, bpc = size
    fx = LP.int_oracle_features(w, h, bpc)
    assert fx.shape == (LP.N_FRAMES, LP.N_FEAT) and np.all(np.isfinite(fx))
    assert np.all(fx[:, 4:8] > 0) and np.all(fx[:, 12:16] > 0) and fx[0, 16] == 0.0 and np.all(fx[1:, 16] > 0)


@pytest.mark.parametrize("size", LP.SIZES + [LIMIT], ids=_id)
def test_partial_counts_fit_their_workspaces_and_int(size):
    """`written` comes from the launchers themselves (a launch of no frames fills *n_partials and launches nothing; the VIF
    march launcher, which needs a device for its tap table, takes its count from vif_march_partials, which the entry calls
    too), `sized` from the functions pqa_create sizes the workspaces with."""
    from pqa2_amd import _native as N
    w, h, bpc = size
    c = LP.partial_counts(w, h, bpc)
    print(f"\n{_id(size)}: {c}")
    kernels = ["vif_march", "motion_march"] + [f"adm_march_{{}}_s{s}" for s in range(4)]
    for k in kernels:
        sized, written = (c[k.format("sized")], c[k.format("written")]) if "{}" in k else (c[k + "_sized"], c[k + "_written"])
        assert 0 < written <= sized <= INT_MAX, (k, written, sized)
        assert sized * 6 <= INT_MAX and sized * 6 * MAX_BATCH < 2 ** 63          # slots x values (x frames of a batch)
    # the pyramid kernel: where its launcher takes the frame the context has sized for it, and for no less
    assert c["adm_pyramid_written"] <= c["adm_pyramid_sized"] <= INT_MAX
    assert (c["adm_pyramid_written"] > 0) == (size in LP.PYRAMID or size == LIMIT)
    # the scale-0 march: the library's own shape gives the same count of waves (four stripes a workgroup, idle ones write 0)
    shape = (C.c_int32 * 6)()
    assert N.load().pqa_debug_vif_march_shape(w, h, C.byref(shape)) == N.PQA_OK
    stripes, blocks, seg_blocks, segs = shape[0], shape[1], shape[2], shape[3]
    assert stripes == -(-w // 16) and blocks == -(-h // 16)
    assert 1 <= seg_blocks <= blocks and segs == -(-blocks // seg_blocks)
    assert c["vif_march_written"] >= stripes * segs                            # a slot for every wave that has a stripe
    assert w * h <= INT_MAX and (w // 2 + 15) // 16 * 16 * (h // 2) * 4 <= INT_MAX     # pixels; bytes of a scale-1 f32 plane
    # the ADM cone's ranges stay inside the bands at this size
    need = (C.c_int32 * 20)()
    assert N.load().pqa_debug_adm_need(w, h, C.byref(need)) == N.PQA_OK
    aw, ah = w, h
    for s in range(4):
        bw, bh = -(-aw // 2), -(-ah // 2)
        r_lo, r_hi, c_lo, c_hi = need[4 * s:4 * s + 4]
        assert 0 <= r_lo < r_hi <= bh and 0 <= c_lo < c_hi <= bw, (s, list(need))
        aw, ah = bw, bh
    assert 0 <= need[16] < need[17] <= h and 0 <= need[18] < need[19] <= w


def test_partial_counts_rejects_bad_arguments():
    from pqa2_amd import _native as N
    lib = N.load()
    out = (C.c_int32 * N.PARTIAL_COUNT_INTS)()
    n = N.PARTIAL_COUNT_INTS
    assert lib.pqa_debug_partial_counts(16384, 16, 8, C.byref(out), n) == N.PQA_OK
    assert lib.pqa_debug_partial_counts(16385, 16, 8, C.byref(out), n) == N.PQA_EINVAL
    assert lib.pqa_debug_partial_counts(16, 15, 8, C.byref(out), n) == N.PQA_EINVAL
    assert lib.pqa_debug_partial_counts(64, 64, 9, C.byref(out), n) == N.PQA_EINVAL
    assert lib.pqa_debug_partial_counts(64, 64, 8, C.byref(out), n - 1) == N.PQA_EINVAL
    assert lib.pqa_debug_partial_counts(64, 64, 8, None, n) == N.PQA_EINVAL
