"""The strip kernel of VIF scales 1-3 gives the bits of the tiled kernel.

vif_strip_kernel (vif.hip) marches a workgroup down a segment of tile rows of one tile column and carries the vertical window
in registers: a row is loaded and squared once and scattered to the row pairs of the current tile and of the tile below.  Each
pair still receives its rows in increasing order, the horizontal pass and the statistic are vif_hstat for both kernels, and a
tile's partial lands in the same slot -- so the records must be equal to the bit, whatever the segment length: with
PQA_VIF_STRIP=0 (vif_stat_kernel everywhere), with the library's own segment rule, and with PQA_VIF_STRIP_SEG = 1, 2, 3, which
make these small frames cross segment boundaries (all read at pqa_create).  Scales 2 and 3 read the planes scales 1 and 2
decimated, so their equality also proves the planes.

Geometries: the smallest at which the march can go wrong, not the workload's --
  528 x 400   scale 1: two strips, the second 16 columns wide, 25 tile rows; scale 2: a partial last tile row; scale 3: 7 tile rows
  272 x 272, 264 x 250   the pair of test_gpu_vif_uniform.py (tile rows partly outside the image)
  2064 x 72   many strips, so few tile rows that a segment is one or two steps
  130 x 1056  one narrow strip with many steps
Every clip is one launch of three frames: seeded texture (statistic all in its log branch), a flat frame (all in the other),
and a letterboxed frame (both, with the seam inside tiles).
"""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [(528, 400), (272, 272), (264, 250), (2064, 72), (130, 1056)]
SEGS = (1, 2, 3)
VIF_TILE_W = (240, 248, 252, 252)   # vif.hip kVifTW; tile height 8


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


_CLIPS = {}


def clip(w, h, bpc):
    """Three (ref, dis) frames; built once per geometry and never modified."""
    key = (w, h, bpc)
    if key not in _CLIPS:
        rng = np.random.default_rng(1000 * w + h)
        base = rng.integers(16, 236, size=(h // 4 + 2, w // 4 + 2)).astype(np.float64)
        tex = np.kron(base, np.ones((4, 4)))[:h, :w] + rng.integers(-12, 13, size=(h, w))   # blocks with grain: sigma1_sq >= 2
        ref_t = np.clip(tex, 0, 255)
        dis_t = np.clip(ref_t + rng.integers(-9, 10, size=(h, w)), 0, 255)
        flat_r = np.full((h, w), 128.0)
        flat_d = np.full((h, w), 126.0)
        bar = max(9, h // 5)   # seams at rows that are no multiple of the tile height
        box_r, box_d = ref_t.copy(), dis_t.copy()
        for p in (box_r, box_d):
            p[:bar] = 128.0
            p[h - bar - 3:] = 128.0
        dt = np.uint8 if bpc == 8 else np.dtype("<u2")
        sc = 1 << (bpc - 8)
        frames = [(np.ascontiguousarray((r * sc).astype(dt)), np.ascontiguousarray((d * sc).astype(dt)))
                  for r, d in ((ref_t, dis_t), (flat_r, flat_d), (box_r, box_d))]
        for r, d in frames:
            r.setflags(write=False)
            d.setflags(write=False)
        _CLIPS[key] = frames
    return _CLIPS[key]


def _run(w, h, bpc, border, env):
    """-> (records[3][17] of the clip, strip shape [scale 1..3][4] of the context for a launch of three frames)"""
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    with _switches(env):
        eng = FeatureEngine(w, h, bit_depth=bpc, max_batch=3, features=N.FEAT_VMAF, vif_border=border)
    with eng:
        shapes = []
        for s in (1, 2, 3):
            out = (C.c_int32 * 4)()
            assert eng.lib.pqa_debug_vif_strip_shape(eng._ctx, s, 3, C.byref(out)) == N.PQA_OK
            shapes.append(list(out))
        for i, (r, d) in enumerate(clip(w, h, bpc)):
            eng.submit(i, [r], [d])
        rec = np.ascontiguousarray(eng.collect(0, 3)[:, :17], dtype=np.float64)   # VIF num / den s0..3, ADM num / den s0..3, motion
    return rec, shapes


def _geometry(w, h):
    """[scale 1..3] -> (strips, tile rows) as the kernels tile the pyramid levels"""
    out = []
    for s in (1, 2, 3):
        w, h = w // 2, h // 2
        out.append((-(-w // VIF_TILE_W[s]), -(-h // 8)))
    return out


def _compare(w, h, bpc, border, base_env):
    tiled, shp = _run(w, h, bpc, border, dict(base_env, PQA_VIF_STRIP="0", PQA_VIF_STRIP_SEG=None))
    assert all(s[2] == 0 and s[3] == 0 for s in shp), shp            # PQA_VIF_STRIP=0: no scale marches
    assert np.all(np.isfinite(tiled)) and np.all(tiled[:, 4:8] > 0)
    geo = _geometry(w, h)
    assert [tuple(s[:2]) for s in shp] == geo, (shp, geo)
    runs = [("rule", None)] + [(f"seg{n}", str(n)) for n in SEGS]
    for name, seg in runs:
        # (a forced segment length on every scale: by default only scale 1, the scale at which it measured faster, marches)
        got, shp = _run(w, h, bpc, border, dict(base_env, PQA_VIF_STRIP=None if seg is None else "14", PQA_VIF_STRIP_SEG=seg))
        print(f"{w}x{h} {bpc}-bit border {border} {name}: shape {shp} vif num {got[0, :4]} den {got[0, 4:8]} "
              f"max|diff| {np.max(np.abs(got - tiled)):.3e}")
        if seg is not None:   # the switch really changes the path: every scale marches, in segments of that many tile rows
            n = int(seg)
            for (strips, rows), s in zip(geo, shp):
                assert s == [strips, rows, min(n, rows), -(-rows // min(n, rows))], (name, s)
            if n < 3:
                assert any(s[3] > 1 for s in shp), shp               # ... and some scale crosses a segment boundary
        assert np.array_equal(got.view(np.uint64), tiled.view(np.uint64)), (name, got - tiled)


@pytest.mark.parametrize("border", [0, 1], ids=["border_float", "border_integer"])
@pytest.mark.parametrize("bpc", [8, 10])
@pytest.mark.parametrize("w,h", SIZES)
def test_strip_bit_equal_tiled(w, h, bpc, border):
    _compare(w, h, bpc, border, {"PQA_VIF_MFMA": None})


def test_strip_bit_equal_tiled_behind_the_valu_scale0():
    """PQA_VIF_MFMA=0: scale 1 reads the plane vif_stat_kernel decimated at scale 0, not the march kernel's."""
    _compare(528, 400, 8, 0, {"PQA_VIF_MFMA": "0"})


def test_segment_rule_at_the_workload():
    """The library's own rule (no switch) at the benchmark's geometry: a launch of 75 frames of 2160p marches scale 1 in evenly
    long segments of several tile rows that leave the launch at least eight rounds of workgroups (3 per CU x 256 CUs); scales
    2 and 3 stay on the tiled kernel unless PQA_VIF_STRIP's mask names them, and then follow the same rule.  A launch of three
    frames is too small for eight rounds at every scale and stays tiled."""
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine

    def shapes(mask):
        with _switches({"PQA_VIF_STRIP": mask, "PQA_VIF_STRIP_SEG": None}):
            eng = FeatureEngine(3840, 2160, max_batch=2, features=N.FEAT_VIF, result_capacity=8)
        with eng:
            def shape(scale, n):
                out = (C.c_int32 * 4)()
                assert eng.lib.pqa_debug_vif_strip_shape(eng._ctx, scale, n, C.byref(out)) == N.PQA_OK
                return list(out)
            assert eng.lib.pqa_debug_vif_strip_shape(eng._ctx, 0, 75, C.byref((C.c_int32 * 4)())) == N.PQA_EINVAL
            return [shape(s, 75) for s in (1, 2, 3)], [shape(s, 3) for s in (1, 2, 3)]

    big, small = shapes(None)
    print("2160p x 75 frames, default:", big)
    assert [s[:2] for s in big] == [[8, 135], [4, 68], [2, 34]]
    s1 = big[0]
    assert s1[2] >= 2 and s1[3] == -(-s1[1] // s1[2]) and s1[2] == -(-s1[1] // s1[3])   # several tile rows, evenly long
    assert s1[0] * s1[3] * 75 >= 8 * 3 * 256
    assert big[1][2:] == [0, 0] and big[2][2:] == [0, 0]
    assert [s[2] for s in small] == [0, 0, 0]
    big, small = shapes("14")
    print("2160p x 75 frames, every scale allowed:", big)
    assert big[0] == s1
    for s in big[1:]:
        assert s[2] == 0 or (s[2] >= 2 and s[0] * s[3] * 75 >= 8 * 3 * 256), s
    assert big[1][2] >= 2                       # 4 strips x 68 tile rows x 75 frames: room for eight rounds
    assert [s[2] for s in small] == [0, 0, 0]
