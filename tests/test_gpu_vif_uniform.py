"""The wave-uniform fast path of the VIF statistic gives the bits of the general path.

vif_s0_march_kernel (vif_march.hip) and vif_hstat (vif.hip) take a shortened statistic when every pixel of a wave is inside
the image and has sigma1_sq >= sigma_nsq; PQA_VIF_UNIFORM=0 (read at pqa_create) sends every wave down the general path.  The
two must agree to the bit on every frame: flat, textured, seams between the two at columns and rows that are no multiple of
16, sigma1_sq straddling 2 pixel by pixel, and frames whose last stripe / block row / tile is partly outside the image
(tests/vif_uniform_ref.py; tests/test_vif_uniform.py pins on the CPU that the clips hold every kind of wave).
"""
import contextlib
import os

import numpy as np
import pytest

from tests import vif_uniform_ref as U

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _switches(env):
    old = {k: os.environ.get(k) for k in env}
    for k, v in env.items():   # None: the library's default, whatever the caller's environment says
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _vif(w, h, bpc, env):
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    refs, diss = U.clip(w, h, bpc)
    with _switches(env):
        eng = FeatureEngine(w, h, bit_depth=bpc, max_batch=3, features=N.FEAT_VIF)   # 7 frames: ends in a partial batch
    with eng:
        for i, (r, d) in enumerate(zip(refs, diss)):
            eng.submit(i, [r], [d])
        return eng.collect(0, len(refs))[:, :8]   # vif_num_s0..3, vif_den_s0..3


@pytest.mark.parametrize("mfma", ["default", "0"])
@pytest.mark.parametrize("bpc", [8, 10, 12])
@pytest.mark.parametrize("w,h", U.SIZES)
def test_fast_paths_bit_equal_general(w, h, bpc, mfma):
    env = {"PQA_VIF_MFMA": None if mfma == "default" else "0"}
    general = _vif(w, h, bpc, dict(env, PQA_VIF_UNIFORM="0"))
    fast = _vif(w, h, bpc, dict(env, PQA_VIF_UNIFORM=None))
    for k, (g, f) in enumerate(zip(general, fast)):
        print(f"{w}x{h} {bpc}-bit mfma={mfma} {U.KINDS[k]:9s} num {f[:4]} den {f[4:]} max|diff| {np.max(np.abs(g - f)):.3e}")
    assert np.all(np.isfinite(fast)) and np.all(fast[:, 4:] > 0)
    for k in range(len(U.KINDS)):
        assert np.array_equal(general[k], fast[k]), (U.KINDS[k], general[k] - fast[k])
