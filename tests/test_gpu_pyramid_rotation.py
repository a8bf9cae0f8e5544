"""adm_pyramid_kernel's 8-bit instance computes two scale-1 rows per trip of its loop, the window-row pairs swapping names
instead of being copied; a trip may end after its first row.  The kernel is compared with the LDS-tiled kernels
(PQA_ADM_MARCH=0) and with the one-scale-per-launch march (PQA_ADM_PYRAMID=0) at the bar of
test_gpu_configs.py::test_adm_and_motion_march_kernels_match_the_tiled_kernels_and_the_oracle (1e-6) on numerator and
denominator of all four ADM scales, 8 and 10 bit (the 16-bit instance keeps one row per trip and shares the loop body).

Sizes (multiples of 4 from 128 up, segments are 32 scale-1 rows; a segment of r rows runs r + 1 or r + 2 loop iterations):
  132 x 132   33 scale-1 rows: a second segment of a single row; one edge stripe
  256 x 132   the same rows over two stripes
  260 x 392   98 rows: four segments, the last of two rows
so the loop runs odd and even trip counts, among them counts that end in the middle of a pair."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("bpc", [8, 10])
@pytest.mark.parametrize("w,h", [(132, 132), (256, 132), (260, 392)])
def test_pyramid_kernel_matches_tiled_and_one_scale_kernels(w, h, bpc):
    from pqa2_amd import _native as N
    from pqa2_amd import synth
    from pqa2_amd.engine import FeatureEngine
    n = 2
    refs, diss = synth.make_clip(w, h, n, bpc, chroma=False)

    def run(**env):
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            with FeatureEngine(w, h, bit_depth=bpc, features=N.FEAT_ADM | N.FEAT_MOTION, max_batch=2) as eng:
                for i in range(n):
                    eng.submit(i, refs[i], diss[i])
                return eng.collect(0, n)[:, 8:16]
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v

    pyramid = run()
    tiled = run(PQA_ADM_MARCH="0")
    single = run(PQA_ADM_PYRAMID="0")
    assert np.all(np.isfinite(pyramid))
    assert not np.array_equal(pyramid.view(np.uint64), tiled.view(np.uint64)), "PQA_ADM_MARCH=0 did not change the path"
    for name, other in (("tiled", tiled), ("one scale per launch", single)):
        rel = np.abs(pyramid - other) / np.maximum(np.abs(other), 1e-30)
        print(w, h, bpc, name, "max rel per record slot:", rel.max(axis=0))
        assert rel.max() < 1e-6, (name, rel.max(axis=0))
