"""Every host entry of FeatureEngine that takes planes, on the MI355X, on every layout of tests/engine_views.py: the result
on views, padded rows, bottom-up rows, other dtypes and mixed strides is the result on contiguous copies of the same samples,
bit for bit (the same kernels on the same bytes).  The scoring entries are compared by the records they leave."""
import numpy as np
import pytest

from tests import engine_views as V

pytestmark = pytest.mark.gpu


def make_engine(name, bits):
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    features = N.FEAT_PSNR | (N.FEAT_SSIM if name.startswith("submit") else N.FEAT_INTEGRITY)
    return FeatureEngine(V.W, V.H, bit_depth=bits, n_planes=3, chroma_shift=V.chroma_shift(name), features=features)


def outcome(eng, name, d, base):
    """the arrays the call of that name leaves on the data `d`; the scoring entries: the records collected after it"""
    result = V.CALLS[name](eng, d)
    if name == "submit":
        result = eng.collect(4, 1)
    elif name == "set_dis_history_planes":      # the SADs of the next frame against the history
        eng.submit(0, base.ref3[0], base.dis3[0])
        result = eng.collect_blocks(0, 1, [4])[1][4]
    elif name.startswith("submit_packed"):
        result = eng.collect(0, V.NF)
    if result is not None and not isinstance(result, np.ndarray):
        assert len(V.flat(result)) >= 1
    if name.startswith("submit") or name == "set_dis_history_planes":
        eng.reset()
    return V.flat(result)


def cell(eng, name, d, base, want):
    """None where the call on `d` gives exactly `want`, else what went wrong in a few words"""
    from pqa2_amd import _native as N
    try:
        got = outcome(eng, name, d, base)
    except N.PqaError as e:
        eng.reset()
        return f"PqaError {e.code}: {str(e).split(': ', 1)[1]}"
    if len(got) != len(want) or any(a.shape != b.shape or a.dtype != b.dtype for a, b in zip(got, want)):
        return "another shape"
    return None if all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got, want)) else "wrong numbers"


_DATA = {}


def data(bits):
    if bits not in _DATA:
        _DATA[bits] = V.Data(bits)
    return _DATA[bits]


@pytest.mark.parametrize("name", list(V.CALLS))
@pytest.mark.parametrize("bits", V.BITS)
def test_every_layout_gives_the_contiguous_result(bits, name):
    base = data(bits)
    with make_engine(name, bits) as eng:
        want = outcome(eng, name, base, base)
        assert len(want) >= 1 and all(a.size for a in want)
        bad = {}
        for layout in V.LAYOUTS:
            why = cell(eng, name, base.laid(layout), base, want)
            if why:
                bad[layout] = why
    assert not bad, (name, bits, bad)


def test_the_results_tell_frames_apart():
    """what the comparison above rests on: other samples give other results, for a call of each kind"""
    base, other = data(8), V.Data(8, seed=1)
    for name in ("submit", "luma_stats", "resample", "tile_moments", "colour_apply"):
        with make_engine(name, 8) as eng:
            a, b = outcome(eng, name, base, base), outcome(eng, name, other, base)
            assert not all(np.array_equal(x, y) for x, y in zip(a, b)), name
