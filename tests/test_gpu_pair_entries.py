"""The one checker and the two drivers that the six spec-driven side analyses share (csrc/pqa_side.hip: spec_check, pair_run;
csrc/host_stage.h), through both entries of each -- pqa_flow_moments, pqa_tile_moments, pqa_band_moments,
pqa_temporal_moments, pqa_edge_profiles, pqa_line_profiles and their _device forms: every rule of the checker refuses with
PQA_EINVAL and names itself and its entry in pqa_last_error, and a valid call after the refusals gives the integers of the
numpy restatements (tests/*_ref.py).  What each analysis computes on larger and awkward inputs is its own file's."""
import ctypes as C

import numpy as np
import pytest

from tests import edge_ref, flow_ref, profile_ref, spectrum_ref, temporal_ref, tile_ref

pytestmark = pytest.mark.gpu

SHAPE = (16, 16)

# name: (spec builder of the engine, its third field and a bad value for it (None: the spec has two fields), the argument of
# the engine's methods for that field, the restatement of a call on (ref, dis))
ANALYSES = {
    "flow_moments": ("_flow_spec", "tile", 12, (8,), lambda r, d: flow_ref.moments(r, d, 8)),
    "tile_moments": ("_tile_spec", "tile", 12, (8,), lambda r, d: tile_ref.tile_moments(r, d, 8, 8)),
    "band_moments": ("_band_spec", "levels", 7, (3,), lambda r, d: spectrum_ref.band_moments(r, d, 3, 8)),
    "temporal_moments": ("_temporal_spec", "tile", 12, (8,), lambda r, d: temporal_ref.temporal_moments(r, d, 8, 8)),
    "edge_profiles": ("_edge_spec", None, None, (), lambda r, d: edge_ref.edge_profiles(r, d, 8)),
    "line_profiles": ("_profile_spec", None, None, (), lambda r, d: profile_ref.line_profiles(r, 8)),
}


def _same(got, want):
    if isinstance(want, tuple):
        return len(got) == len(want) and all(_same(g, w) for g, w in zip(got, want))
    return got.shape == want.shape and np.array_equal(got.view(np.uint64), np.asarray(want).view(np.uint64))


@pytest.mark.parametrize("name", list(ANALYSES))
def test_every_rule_of_the_checker_speaks_and_a_valid_call_follows(name):
    import torch
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    builder, third, bad, extra, restated = ANALYSES[name]
    pair = name != "line_profiles"
    ref, dis = tile_ref.random_pairs(len(name), 2, 16, 16, 8)
    with FeatureEngine(16, 16, n_planes=1, features=N.FEAT_PSNR) as eng:
        lib, ctx = eng.lib, eng._ctx
        keep_r, rp, rs = eng._luma_list(ref, "reference", SHAPE)
        keep_d, dp, ds = eng._luma_list(dis, "captured", SHAPE)
        out = np.zeros(4096, np.uint64)
        dev = 4096      # never dereferenced: every call of the table is refused before any device call

        def spec(**kw):
            s = getattr(eng, builder)(SHAPE, *extra)
            for k, v in kw.items():
                setattr(s, k, v)
            return C.byref(s)

        def host(s="good", r=rp, rst=rs, d=dp, dst=ds, n=2, to=out.ctypes.data):
            s = spec() if s == "good" else s
            clips = (r, rst, d, dst) if pair else (r, rst)
            return getattr(lib, "pqa_" + name)(ctx, s, *clips, n, to)

        def device(s="good", r=dev, rst=16, d=dev, dst=16, n=2, to=out.ctypes.data):
            s = spec() if s == "good" else s
            clips = (r, rst, 256, d, dst, 256) if pair else (r, rst, 256)
            return getattr(lib, "pqa_" + name + "_device")(ctx, s, *clips, n, to)

        rules = [(dict(s=None), b"null"), (dict(s=spec(struct_size=20)), b"struct_size"), (dict(s=spec(width=0)), b"outside"),
                 (dict(s=spec(height=8193)), b"outside"), (dict(n=-1), b"negative"), (dict(r=None), b"null"),
                 (dict(to=None), b"null"), (dict(rst=15), b"smaller than a row")]
        if third:
            rules.append((dict(s=spec(**{third: bad})), third.encode()))
        if pair:
            rules += [(dict(d=None), b"null"), (dict(dst=15), b"smaller than a row")]
        for call in (host, device):
            for kw, word in rules:
                assert call(**kw) == N.PQA_EINVAL, (call.__name__, kw)
                said = lib.pqa_last_error(ctx)
                assert said.startswith(name.encode() + b": ") and word in said, (call.__name__, kw, said)
        assert not out.any()
        del keep_r, keep_d

        want = restated(ref, dis)
        clips = (ref, dis) if pair else (ref,)
        assert _same(getattr(eng, name)(*clips, *extra), want)
        bufs = [torch.from_numpy(np.stack(c)).cuda() for c in clips]
        torch.cuda.synchronize()
        where = [v for b in bufs for v in (b.data_ptr(), 16, 256)]
        assert _same(getattr(eng, name + "_resident")(*where, SHAPE, 2, *extra), want)
