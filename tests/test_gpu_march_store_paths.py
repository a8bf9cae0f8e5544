"""vif_s0_march_kernel writes the input of scale 1 through an address that each lane forms once per segment and moves by
eight rows per block.  Scales 1-3 read those planes, so a store that lands in the wrong row, is dropped, or runs past the
plane's last row shows in THEIR records: the march path is compared with the VALU kernel (PQA_VIF_MFMA=0, which decimates on
its own) on numerator and denominator of all four scales, at the bar of
test_gpu_configs.py::test_vif_mfma_path_matches_valu_path_and_oracle (2e-6), in both border modes, 8 / 10 / 12 bit.

Geometries: the smallest that reach every store path and restart the address in a second and third segment (segments are 8
blocks of 16 rows here):
  272 x 272   17 blocks = segments of 8 / 8 / 1; ow = 136: every store a full 16-byte one, oh = 136 ends with a block
  266 x 250   16 blocks = 8 / 8; ow = 133: the last stripe has one full store and one element by element; oh = 125 ends
              inside a block (rows past it must not be written)
  258 x 262   17 blocks = 8 / 8 / 1; ow = 129: one sample valid in the last stripe's first lane group and the other group
              entirely outside; that stripe loads sample by sample; the single block of the last segment holds oh = 131's
              last three rows"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _clip(w, h, n, bpc, seed):
    """seeded noise on a texture (two gratings and a ramp), the distorted frame a smoothed, re-noised copy"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    refs, diss = [], []
    for t in range(n):
        tex = 128.0 + 45.0 * np.sin(0.21 * xx + 0.4 * t) * np.cos(0.13 * yy) + 25.0 * np.sin(0.05 * (xx + 2.0 * yy)) + 0.1 * (xx - yy)
        r = tex + rng.normal(0.0, 12.0, (h, w))
        d = 0.5 * r + 0.125 * (np.roll(r, 1, 0) + np.roll(r, -1, 0) + np.roll(r, 1, 1) + np.roll(r, -1, 1)) + rng.normal(0.0, 4.0, (h, w))
        scale = 1 << (bpc - 8)
        dt = np.uint8 if bpc == 8 else np.uint16
        refs.append([np.clip(np.rint(r * scale), 0, 256 * scale - 1).astype(dt)])
        diss.append([np.clip(np.rint(d * scale), 0, 256 * scale - 1).astype(dt)])
    return refs, diss


@pytest.mark.parametrize("bpc", [8, 10, 12])
@pytest.mark.parametrize("w,h", [(272, 272), (266, 250), (258, 262)])
def test_next_scale_store_paths_feed_scales_1_to_3(w, h, bpc):
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    n = 2
    refs, diss = _clip(w, h, n, bpc, seed=1000 * bpc + w)

    def run(**kw):
        with FeatureEngine(w, h, bit_depth=bpc, features=N.FEAT_VIF, **kw) as eng:
            for i in range(n):
                eng.submit(i, refs[i], diss[i])
            return eng.collect(0, n)[:, :8]

    old = os.environ.get("PQA_VIF_MFMA")
    try:
        os.environ["PQA_VIF_MFMA"] = "1"
        march = run()
        march101 = run(vif_border=N.VIF_BORDER_INTEGER)
        os.environ["PQA_VIF_MFMA"] = "0"
        valu = run()
        valu101 = run(vif_border=N.VIF_BORDER_INTEGER)
    finally:
        if old is None:
            os.environ.pop("PQA_VIF_MFMA", None)
        else:
            os.environ["PQA_VIF_MFMA"] = old
    assert np.all(np.isfinite(march)) and np.all(np.isfinite(march101))
    assert not np.array_equal(march.view(np.uint64), valu.view(np.uint64)), "the switch did not change the path"
    for name, a, b in (("mirror", march, valu), ("integer border", march101, valu101)):
        rel = np.abs(a - b) / np.abs(b)
        print(w, h, bpc, name, "max rel per record slot:", rel.max(axis=0))
        assert rel.max() < 2e-6, (name, rel.max(axis=0))
