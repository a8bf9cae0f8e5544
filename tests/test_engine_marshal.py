"""How FeatureEngine hands host planes to the library, checked without a device: an engine over a stand-in for the library
that records every call and, INSIDE the call, reads the planes back through the pointers and strides it was given and writes
a pattern through the destination pointers.  Every host entry that takes planes, at 8 and 10 bit, on every layout of
tests/engine_views.py: the library sees the samples, plain inputs arrive at their own addresses, every stride is positive and
at least a row, and the arrays a method returns are the ones the library wrote.  Where libpqa_vmaf.so is built the arguments
of every call also go through the argtypes pqa2_amd/_native.py declares for the real entry."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import engine_views as V

U8, U64 = np.dtype(np.uint8), np.dtype(np.uint64)
HANDLE = 0x5000


def _real_library():
    from pqa2_amd import _native as N
    return N.load() if os.path.exists(N.LIB_PATH) else None


def _pattern(j, shape, dt):
    top = 250 if dt.kind == "f" or dt.itemsize > 2 else int(np.iinfo(dt).max)
    return ((np.arange(shape[0] * shape[1]).reshape(shape) * 3 + 31 * j + 7) % top).astype(dt)


class Recorder:
    """The library as FeatureEngine uses it.  `wire`: (inputs(args), outputs(args)) of the call under test, each a list of
    (pointer, row stride, (rows, samples a row), dtype) per plane."""

    def __init__(self, real):
        self.real, self.calls, self.wire, self.read, self.strides = real, [], None, [], []

    def pqa_config_init(self, cfg, width, height):
        cfg = cfg._obj
        cfg.struct_size, cfg.width, cfg.height, cfg.bit_depth, cfg.n_planes = C.sizeof(cfg), width, height, 8, 1

    def pqa_create(self, cfg, ctx):
        ctx._obj.value = HANDLE
        return 0

    def pqa_destroy(self, ctx):
        pass

    def pqa_last_error(self, ctx):
        return b""

    def __getattr__(self, name):
        if not name.startswith("pqa_"):
            raise AttributeError(name)

        def call(*args):
            if self.real is not None and getattr(self.real, name).argtypes is not None:
                types = getattr(self.real, name).argtypes
                assert len(types) == len(args), name
                for t, a in zip(types, args):
                    t.from_param(a)
            plain = [getattr(a, "_obj", a) for a in args]     # what a byref points at
            self.calls.append((name, plain))
            if self.wire is not None:
                ins, outs = self.wire
                for ptr, stride, shape, dt in ins(plain):
                    self.strides.append((stride, shape[1] * dt.itemsize))
                    rows = [np.frombuffer(C.string_at(ptr + y * stride, shape[1] * dt.itemsize), dt) for y in range(shape[0])]
                    self.read.append(np.stack(rows))
                for j, (ptr, stride, shape, dt) in enumerate(outs(plain)):
                    self.strides.append((stride, shape[1] * dt.itemsize))
                    assert ptr and stride >= shape[1] * dt.itemsize, (name, j)      # before anything is written
                    for y, row in enumerate(_pattern(j, shape, dt)):
                        C.memmove(ptr + y * stride, row.ctypes.data, row.nbytes)
            return 0
        return call


@pytest.fixture(scope="module")
def real():
    return _real_library()


@pytest.fixture
def engine(monkeypatch, real):
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    made = []

    def make(bits=8, n_planes=3, chroma_shift=(1, 1)):
        rec = Recorder(real)
        monkeypatch.setattr(N, "load", lambda: rec)
        eng = FeatureEngine(V.W, V.H, bit_depth=bits, n_planes=n_planes, chroma_shift=chroma_shift)
        made.append(eng)
        return eng, rec
    yield make
    for eng in made:
        eng.close()


_DATA = {}


def _data(bits):
    if bits not in _DATA:
        _DATA[bits] = V.Data(bits)
    return _DATA[bits]


# ---- where the planes of each call are among its arguments (args[0] is the context) ----------------------------------------
def _list(ptrs, stride, n, shape, dt):
    return [(ptrs[i], stride, shape, dt) for i in range(n)]


def _frames(ptrs, strides, n, shapes, dt, step=3):
    return [(ptrs[i * step + p], strides[p], shapes[p], dt) for i in range(n) for p in range(len(shapes))]


def _result(ptr, shape, dt):
    """a result array [n, ...] as one plane of n rows"""
    dt, rest = np.dtype(dt), int(np.prod(shape[1:]))
    return [(ptr, rest * dt.itemsize, (shape[0], rest), dt)]


def _planes(frames):
    return [a for f in frames for a in f]


def _pairs(name, out_shape, out_dt=U64):
    """an analysis of two lists of luma planes: (ctx, spec, ref, stride, dis, stride, n, out)"""
    return dict(c=name,
                ins=lambda a, d: _list(a[2], a[3], a[6], V.LUMA, V.dtype(d.bits)) + _list(a[4], a[5], a[6], V.LUMA, V.dtype(d.bits)),
                given=lambda d: d.ref_y + d.dis_y, outs=lambda a, d: _result(a[7], out_shape, out_dt),
                result=lambda d: [(out_shape, out_dt)])


def _transform(name, src, dst, sptr, dptr, n, given, n_out=None, more=None):
    """a plane transform: source list and stride at args[sptr], args[sptr + 1], destination at args[dptr], args[dptr + 1];
    src / dst: shape, or a function of the data"""
    sh = lambda s, d: s(d) if callable(s) else s
    count = lambda a: a[n] * (n_out or 1)
    return dict(c=name,
                ins=lambda a, d: _list(a[sptr], a[sptr + 1], a[n], sh(src, d), V.dtype(d.bits)) + (more(a, d) if more else []),
                given=given, outs=lambda a, d: _list(a[dptr], a[dptr + 1], count(a), sh(dst, d), V.dtype(d.bits)),
                result=lambda d: [(sh(dst, d), V.dtype(d.bits))] * (V.NF * (n_out or 1)))


def _unpacked(name, given, src_shape, planes):
    """pqa_unpack / pqa_rgb_convert: (ctx, spec, src, stride, n, dst [n * 3], dst strides); the chroma planes of `planes`"""
    out_dt = lambda d: np.dtype(np.uint16 if d.bits > 8 else np.uint8)
    return dict(c=name, ins=lambda a, d: _list(a[2], a[3], a[4], src_shape(d), U8), given=given,
                outs=lambda a, d: _frames(a[5], a[6], a[4], planes, out_dt(d)),
                result=lambda d: [(s, out_dt(d)) for s in planes] * V.NF)


def _host_clip(h, n, d, packed, shapes):
    if packed:
        return _list(h.frames, h.strides[0], n, d.packed_shape, U8)
    return _frames(h.frames, h.strides, n, shapes, V.dtype(d.bits), step=3)


def _three(name, first, out=None):
    """an analysis of two lists of frames [Y, U, V]: (ctx, ..., ref, strides, dis, strides, n, ..., out)"""
    f = first
    return dict(c=name,
                ins=lambda a, d: _frames(a[f], a[f + 1], a[f + 4], V.SHAPES, V.dtype(d.bits)) + _frames(a[f + 2], a[f + 3], a[f + 4], V.SHAPES, V.dtype(d.bits)),
                given=lambda d: _planes(d.ref3) + _planes(d.dis3), outs=lambda a, d: _result(a[-1], *out), result=lambda d: [out])


L = V.H + V.W
TY, TX = -(-V.H // 8), -(-V.W // 8)
dt_of = lambda d: V.dtype(d.bits)
WIRES = {
    "submit": dict(c="pqa_submit", ins=lambda a, d: _frames(a[2], a[3], 1, V.SHAPES, dt_of(d)) + _frames(a[4], a[5], 1, V.SHAPES, dt_of(d)),
                   given=lambda d: d.ref3[0] + d.dis3[0]),
    "set_dis_history_planes": dict(c="pqa_set_dis_history_planes", ins=lambda a, d: _frames(a[1], a[2], 1, V.SHAPES, dt_of(d)),
                                   given=lambda d: d.dis3[1]),
    "frame_sad": dict(c="pqa_frame_sad",
                      ins=lambda a, d: _frames(a[1], a[2], 1, V.SHAPES, dt_of(d)) + _frames(a[3], a[4], a[5], V.SHAPES, dt_of(d)),
                      given=lambda d: d.ref3[0] + _planes(d.dis3), outs=lambda a, d: _result(a[6], (V.NF, 3), U64),
                      result=lambda d: [((V.NF, 3), U64)]),
    "luma_stats": dict(c="pqa_luma_stats", ins=lambda a, d: _list(a[1], a[2], a[3], V.LUMA, dt_of(d)), given=lambda d: d.ref_y,
                       outs=lambda a, d: _result(a[5], (V.NF, 3), U64), result=lambda d: [((V.NF, 3), U64)]),
    "cross_sse": dict(c="pqa_cross_sse",
                      ins=lambda a, d: _list(a[1], a[2], a[3], V.LUMA, dt_of(d)) + _list(a[4], a[5], a[6], V.LUMA, dt_of(d)),
                      given=lambda d: d.ref_y + d.dis_y, outs=lambda a, d: _result(a[9], (V.NF, 3), U64),
                      result=lambda d: [((V.NF, 3), U64)]),
    "shift_sse": dict(c="pqa_shift_sse",
                      ins=lambda a, d: _list(a[1], a[2], a[5], V.LUMA, dt_of(d)) + _list(a[3], a[4], a[5], V.LUMA, dt_of(d)),
                      given=lambda d: d.ref_y + d.dis_y, outs=lambda a, d: _result(a[7], (V.NF, 3, 3), U64),
                      result=lambda d: [((V.NF, 3, 3), U64)]),
    "level_stats": dict(c="pqa_level_stats",
                        ins=lambda a, d: _list(a[1], a[2], a[5], V.CHROMA, dt_of(d)) + _list(a[3], a[4], a[5], V.CHROMA, dt_of(d)),
                        given=lambda d: d.ref_u + d.dis_u, outs=lambda a, d: _result(a[7], (V.NF, 1 << d.bits, 3), U64),
                        result=lambda d: [((V.NF, 1 << d.bits, 3), U64)]),
    "table_apply": _transform("pqa_table_apply", V.LUMA, V.LUMA, 3, 5, 7, lambda d: d.ref_y),
    "deinterlace frame": _transform("pqa_deinterlace", V.LUMA, V.LUMA, 2, 4, 6, lambda d: d.ref_y),
    "deinterlace field": _transform("pqa_deinterlace", V.LUMA, V.LUMA, 2, 4, 6, lambda d: d.ref_y, n_out=2),
    "mask_blend constant": _transform("pqa_mask_blend", V.LUMA, V.LUMA, 3, 7, 9, lambda d: d.ref_y),
    "mask_blend planes": _transform("pqa_mask_blend", V.LUMA, V.LUMA, 3, 7, 9, lambda d: d.ref_y + d.fill,
                                    more=lambda a, d: _list(a[5], a[6], a[9], V.LUMA, dt_of(d))),
    "resample": _transform("pqa_resample", V.LUMA, V.SMALL, 2, 4, 6, lambda d: d.ref_y),
    "format_convert": _transform("pqa_format_convert", V.C422, V.CHROMA, 2, 4, 6, lambda d: d.c422),
    "unpack": _unpacked("pqa_unpack", lambda d: d.packed, lambda d: d.packed_shape, V.SHAPES_422),
    "unpack luma": _unpacked("pqa_unpack", lambda d: d.packed, lambda d: d.packed_shape, V.SHAPES_422[:1]),
    "rgb_convert": _unpacked("pqa_rgb_convert", lambda d: d.rgb, lambda d: V.RGB, V.SHAPES),
    "submit_packed planar, packed": dict(c="pqa_submit_packed", given=lambda d: _planes(d.ref422) + d.packed,
                                         ins=lambda a, d: _host_clip(a[3], a[2], d, False, V.SHAPES_422) + _host_clip(a[4], a[2], d, True, None)),
    "submit_packed packed, planar": dict(c="pqa_submit_packed", given=lambda d: d.packed + _planes(d.dis422),
                                         ins=lambda a, d: _host_clip(a[3], a[2], d, True, None) + _host_clip(a[4], a[2], d, False, V.SHAPES_422)),
    "flow_moments": _pairs("pqa_flow_moments", (V.NF, TY, TX, 6), np.dtype(np.int64)),
    "tile_moments": _pairs("pqa_tile_moments", (V.NF, TY, TX, 6)),
    "band_moments": _pairs("pqa_band_moments", (V.NF, 3, 4, 3)),
    "temporal_moments": _pairs("pqa_temporal_moments", (V.NF - 1, TY, TX, 7)),
    "field_moments": _pairs("pqa_field_moments", (V.NF - 1, 14)),
    "edge_profiles": dict(_pairs("pqa_edge_profiles", (V.NF, L, 3)), result=lambda d: [((V.NF, V.H, 3), U64), ((V.NF, V.W, 3), U64)],
                          back=lambda r: [np.concatenate(r, 1).reshape(V.NF, -1)]),
    "line_profiles": dict(c="pqa_line_profiles", ins=lambda a, d: _list(a[2], a[3], a[4], V.LUMA, dt_of(d)), given=lambda d: d.ref_y,
                          outs=lambda a, d: _result(a[5], (V.NF, L, 2), U64), result=lambda d: [((V.NF, V.H, 2), U64), ((V.NF, V.W, 2), U64)],
                          back=lambda r: [np.concatenate(r, 1).reshape(V.NF, -1)]),
    "colour_moments": _three("pqa_colour_moments", 1, ((V.NF, 28), U64)),
    "colour_apply": dict(c="pqa_colour_apply", ins=lambda a, d: _frames(a[2], a[3], a[6], V.SHAPES, dt_of(d)), given=lambda d: _planes(d.dis3),
                         outs=lambda a, d: _frames(a[4], a[5], a[6], V.SHAPES, dt_of(d)),
                         result=lambda d: [(s, dt_of(d)) for s in V.SHAPES] * V.NF),
    "delta_itp": _three("pqa_delta_itp", 2, ((V.NF, 8), np.dtype(np.float64))),
}


def test_every_call_has_its_wiring():
    assert sorted(WIRES) == sorted(V.CALLS)


@pytest.mark.parametrize("layout", list(V.LAYOUTS))
@pytest.mark.parametrize("name", list(V.CALLS))
@pytest.mark.parametrize("bits", V.BITS)
def test_planes_reach_the_library(engine, bits, name, layout):
    wire, base = WIRES[name], _data(bits)
    d = base.laid(layout)
    eng, rec = engine(bits, chroma_shift=V.chroma_shift(name))
    none = lambda a, d: []
    rec.wire = (lambda a: wire["ins"](a, d), lambda a: wire.get("outs", none)(a, d))
    result = V.CALLS[name](eng, d)
    assert [c[0] for c in rec.calls] == [wire["c"]] and rec.calls[0][1][0].value == HANDLE
    # 1. the library reads the samples
    want, given = wire["given"](base), wire["given"](d)
    assert len(rec.read) == len(want)
    for k, (got, w) in enumerate(zip(rec.read, want)):
        assert got.shape == w.shape and np.array_equal(got, w), (name, layout, "plane", k)
    # 2. plain inputs are not copied
    if layout in V.PLAIN:
        addresses = [p[0] for p in wire["ins"](rec.calls[0][1], d)]
        assert addresses == [g.ctypes.data for g in given], (name, layout)
    # 4. what the method returns is what the library wrote, in the shapes and types the entry documents
    arrays = V.flat(result)
    assert [(a.shape, a.dtype) for a in arrays] == [(tuple(s), np.dtype(t)) for s, t in wire.get("result", lambda d: [])(d)]
    planes = wire.get("back", lambda r: [a.reshape(a.shape[0], -1) for a in V.flat(r)])(result)
    written = wire.get("outs", none)(rec.calls[0][1], d)
    assert len(planes) == len(written)
    for j, (plane, (_, _, shape, dt)) in enumerate(zip(planes, written)):
        assert np.array_equal(plane, _pattern(j, shape, dt)), (name, layout, "output", j)
    # 3. every stride is positive and at least a row
    assert rec.strides and all(stride >= row > 0 for stride, row in rec.strides), (name, layout, rec.strides)


# ---- empty lists -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", V.BITS)
def test_empty_lists(engine, bits):
    """luma_stats and frame_sad return before any call; the others call with n = 0, a pointer array of one entry and the
    default stride: the bytes of a row, 0 for packed rows"""
    d, item = _data(bits), V.dtype(bits).itemsize
    eng, rec = engine(bits)
    assert eng.luma_stats([], 10).shape == (0, 3) and eng.frame_sad(d.ref3[0], []).shape == (0, 3) and rec.calls == []
    row, crow = V.W * item, V.W // 2 * item

    def last(n_at, lists):
        name, a = rec.calls[-1]
        assert a[n_at] == 0, name
        for ptrs, stride, want in lists(a):
            assert len(ptrs) == 1 and not ptrs[0], name
            assert (list(stride) if hasattr(stride, "__len__") else stride) == want, name
    assert eng.cross_sse([], [], -1, 1).shape == (0, 3)
    last(3, lambda a: [(a[1], a[2], row), (a[4], a[5], row)])
    assert eng.shift_sse([], [], 1).shape == (0, 3, 3)
    last(5, lambda a: [(a[1], a[2], row), (a[3], a[4], row)])
    assert eng.level_stats([], [], 1).shape == (0, 1 << bits, 3)
    last(5, lambda a: [(a[1], a[2], crow), (a[3], a[4], crow)])
    assert eng.table_apply([], d.table) == [] and eng.table_apply([], d.table, plane=1) == []
    last(7, lambda a: [(a[3], a[4], crow), (a[5], a[6], crow)])
    assert eng.deinterlace([], rate="field") == []
    last(6, lambda a: [(a[2], a[3], row), (a[4], a[5], row)])
    assert eng.mask_blend([], d.nodes, (3, 3), []) == []
    last(9, lambda a: [(a[3], a[4], row), (a[5], a[6], row), (a[7], a[8], row)])
    assert eng.resample([], V.SMALL) == []
    last(6, lambda a: [(a[2], a[3], V.SMALL[1] * item), (a[4], a[5], V.SMALL[1] * item)])
    assert eng.format_convert([], V.LUMA, (1, 0, 0, 0, bits), (1, 1, 0, 1, bits)) == []
    last(6, lambda a: [(a[2], a[3], crow), (a[4], a[5], crow)])
    assert eng.unpack([], d.fmt, V.LUMA) == [] and eng.rgb_convert([], "bgra", V.LUMA, (1, 1, 0, 1, bits), V.MATRIX) == []
    out_item = 2 if bits > 8 else 1
    last(4, lambda a: [(a[2], a[3], 0), (a[5], a[6], [V.W * out_item, V.W // 2 * out_item, V.W // 2 * out_item])])
    assert eng.tile_moments([], [], 8).shape == (0, TY, TX, 6) and eng.line_profiles([])[0].shape == (0, V.H, 2)
    last(4, lambda a: [(a[2], a[3], row)])
    assert eng.colour_moments([], []).shape == (0, 28) and eng.delta_itp([], [], V.itp_spec(bits)).shape == (0, 8)
    last(6, lambda a: [(a[2], a[3], [row, crow, crow]), (a[4], a[5], [row, crow, crow])])
    assert eng.colour_apply([], V.MATRIX) == []
    last(6, lambda a: [(a[2], a[3], [row, crow, crow]), (a[4], a[5], [row, crow, crow])])
    eng.submit_packed(0, ([], None), ([], d.fmt))
    name, a = rec.calls[-1]
    assert a[2] == 0 and list(a[3].strides) == [0, 0, 0] and list(a[4].strides) == [0, 0, 0] and not a[3].frames[0] and not a[4].frames[0]


# ---- what is refused before the library is called --------------------------------------------------------------------------
def _refusals(d):
    from pqa2_amd import _native as N
    y, u, bad = d.ref_y, d.ref_u, [d.ref_y[0], d.ref_y[1][:-1], d.ref_y[2]]
    bad3 = [d.ref3[0], [d.ref3[1][0], d.ref3[1][1][:, :-1], d.ref3[1][2]], d.ref3[2]]
    cube = [np.zeros((2, 3, 4), np.uint8)] * 2
    packed_bad = [d.packed[0], d.packed[1][:, :-2]]
    E, P = ValueError, N.PqaError
    return [
        (lambda e: e.level_stats(y, y[:2]), P, "pqa error -1: level_stats needs as many captured as reference frames"),
        (lambda e: e.luma_stats(bad, 10), E, f"luma frame 1 is {(V.H - 1, V.W)}, engine is {V.LUMA}"),
        (lambda e: e.cross_sse(y, bad, -1, 1), E, f"captured frame 1 is {(V.H - 1, V.W)}, engine is {V.LUMA}"),
        (lambda e: e.shift_sse(bad, y, 1), E, f"reference frame 1 is {(V.H - 1, V.W)}, engine is {V.LUMA}"),
        (lambda e: e.shift_sse(y, y[:2], 1), E, "shift_sse needs as many captured as reference frames"),
        (lambda e: e.level_stats(y, y, 1), E, f"reference frame 0 is {V.LUMA}, engine is {V.CHROMA}"),
        (lambda e: e.table_apply(bad, d.table), E, f"source frame 1 is {(V.H - 1, V.W)}, engine is {V.LUMA}"),
        (lambda e: e.table_apply(cube, d.table, plane=None), E, "table_apply needs 2-D planes"),
        (lambda e: e.deinterlace(cube), E, "deinterlace needs 2-D planes"),
        (lambda e: e.deinterlace(bad), E, f"source frame 1 is {(V.H - 1, V.W)}, engine is {V.LUMA}"),
        (lambda e: e.mask_blend(cube, d.nodes, (3, 3), 0, plane=None), E, "mask_blend needs 2-D planes"),
        (lambda e: e.mask_blend(y, d.nodes, (3, 3), d.fill[:2]), E, "mask_blend needs as many fill planes as frames"),
        (lambda e: e.mask_blend(y, d.nodes, (3, 3), bad), E, f"fill frame 1 is {(V.H - 1, V.W)}, engine is {V.LUMA}"),
        (lambda e: e.resample(bad, V.SMALL), E, "resample needs 2-D planes of one size"),
        (lambda e: e.resample(cube, V.SMALL), E, "resample needs 2-D planes of one size"),
        (lambda e: e.format_convert(y, V.LUMA, (1, 0, 0, 0, d.bits), (1, 1, 0, 1, d.bits)), E,
         f"format_convert needs 2-D planes of {V.C422[0]} x {V.C422[1]} samples"),
        (lambda e: e.unpack(packed_bad, d.fmt, V.LUMA), E, "unpack needs 2-D arrays of packed rows of one size"),
        (lambda e: e.unpack(cube, d.fmt, V.LUMA), E, "unpack needs 2-D arrays of packed rows of one size"),
        (lambda e: e.rgb_convert(packed_bad, "bgra", V.LUMA, (1, 1, 0, 1, 8), V.MATRIX), E, "rgb_convert needs 2-D arrays of packed rows of one size"),
        (lambda e: e.submit_packed(0, (d.ref3, None), (packed_bad, d.fmt)), E, "submit_packed needs as many reference as captured frames"),
        (lambda e: e.submit_packed(0, (d.ref3[:2], None), (packed_bad, d.fmt)), E, "submit_packed needs 2-D arrays of packed rows of one size"),
        (lambda e: e.tile_moments(y, y[:2], 8), E, "tile_moments needs as many captured as reference frames"),
        (lambda e: e.flow_moments(cube, cube, 8), E, "flow_moments needs 2-D planes"),
        (lambda e: e.band_moments(y, bad, 3), E, f"captured frame 1 is {(V.H - 1, V.W)}, engine is {V.LUMA}"),
        (lambda e: e.line_profiles(bad), E, f"profile frame 1 is {(V.H - 1, V.W)}, engine is {V.LUMA}"),
        (lambda e: e.colour_moments(d.ref3, d.dis3[:2]), E, "colour_moments needs as many captured as reference frames"),
        (lambda e: e.colour_moments(d.ref3, bad3), E, f"captured frame 1 plane 1 is {(V.H // 2, V.W // 2 - 1)}, engine is {V.CHROMA}"),
        (lambda e: e.colour_apply(bad3, V.MATRIX), E, f"source frame 1 plane 1 is {(V.H // 2, V.W // 2 - 1)}, engine is {V.CHROMA}"),
        (lambda e: e.delta_itp(bad3, d.dis3, V.itp_spec(d.bits)), E, f"reference frame 1 plane 1 is {(V.H // 2, V.W // 2 - 1)}, engine is {V.CHROMA}"),
        (lambda e: e.delta_itp(d.ref3, d.dis3[:1], V.itp_spec(d.bits)), E, "delta_itp needs as many captured as reference frames"),
    ]


@pytest.mark.parametrize("k", range(30))
def test_refusals_keep_their_type_and_text(engine, k):
    d = _data(8)
    call, kind, text = _refusals(d)[k]
    eng, rec = engine(8)
    with pytest.raises(kind) as e:
        call(eng)
    assert type(e.value) is kind and str(e.value) == text and rec.calls == []


def test_the_refusal_list_is_whole():
    assert len(_refusals(_data(8))) == 30


@pytest.mark.parametrize("call", ["colour_moments", "colour_apply", "delta_itp"])
def test_three_plane_entries_need_three_planes(engine, call):
    from pqa2_amd import _native as N
    d = _data(8)
    eng, rec = engine(8, n_planes=1)
    with pytest.raises(N.PqaError) as e:
        V.CALLS[call](eng, d)
    assert e.value.code == N.PQA_EINVAL and str(e.value) == f"pqa error -1: {call} needs the chroma planes: n_planes must be 3"
    assert rec.calls == []


# ---- the private builders other tests call ---------------------------------------------------------------------------------
def test_luma_list_and_frame_list_keep_their_shape(engine):
    d = _data(10)
    eng, rec = engine(10)
    keep, ptrs, stride = eng._luma_list(d.ref_u, "reference", V.CHROMA)
    assert [p for p in ptrs] == [a.ctypes.data for a in d.ref_u] and stride == V.W // 2 * 2 and len(keep) == V.NF
    keep, ptrs, strides = eng._frame_list(d.ref3, "reference")
    assert [p for p in ptrs] == [a.ctypes.data for f in d.ref3 for a in f] and list(strides) == [V.W * 2, V.W // 2 * 2, V.W // 2 * 2]
    assert isinstance(strides, C.c_int64 * 3)
    clip = eng._device_clip([4096, 0, 8192], [64, 32, 32], [4096, 1024, 1024])
    assert [clip.plane[p] for p in range(3)] == [4096, None, 8192] and list(clip.row_pitch) == [64, 32, 32] and list(clip.frame_pitch) == [4096, 1024, 1024]


def test_spec_builders_keep_their_names(engine):
    """the builders the argument tests of the raw entries call: each gives the spec of its row of the table"""
    from pqa2_amd import _native as N
    eng, rec = engine(8)
    for name, cls, third in (("_flow_spec", N.PqaFlowSpec, ("tile", 8)), ("_tile_spec", N.PqaTileSpec, ("tile", 16)),
                             ("_band_spec", N.PqaBandSpec, ("levels", 3)), ("_temporal_spec", N.PqaTemporalSpec, ("tile", 8)),
                             ("_profile_spec", N.PqaProfileSpec, None), ("_field_spec", N.PqaFieldSpec, None),
                             ("_edge_spec", N.PqaEdgeSpec, None)):
        sp = getattr(eng, name)((24, 40), *([third[1]] if third else []))
        assert type(sp) is cls and (sp.struct_size, sp.height, sp.width) == (C.sizeof(cls), 24, 40), name
        assert third is None or getattr(sp, third[0]) == third[1], name


def test_resident_clips(engine):
    """the device clips of the resident entries: the planes the caller names, null for 0, the rest untouched"""
    eng, rec = engine(8, n_planes=1)
    eng.submit_resident(3, 2, [4096], [8192], [64], [4096], prev_ref_luma_ptr=0)
    name, a = rec.calls[-1]
    assert name == "pqa_submit_device" and a[1:3] == [3, 2] and a[5] is None
    for clip, ptr in ((a[3], 4096), (a[4], 8192)):
        assert [clip.plane[p] for p in range(3)] == [ptr, None, None] and list(clip.row_pitch) == [64, 0, 0] and list(clip.frame_pitch) == [4096, 0, 0]
    eng.frame_sad_resident([4096], [64], [8192], [128], [16384], 2)
    name, a = rec.calls[-1]
    assert name == "pqa_frame_sad_device" and a[1][0] == 4096 and a[2][0] == 64 and a[3].plane[0] == 8192 and a[3].row_pitch[0] == 128
    eng.unpack_resident("uyvy422", V.LUMA, 4096, 100, 3800, 2, (8192, 0, 12288), (50, 25, 25), (1900, 950, 950))
    name, a = rec.calls[-1]
    assert name == "pqa_unpack_device" and [a[6].plane[p] for p in range(3)] == [8192, None, 12288] and list(a[6].row_pitch) == [50, 25, 25]
    eng.rgb_convert_resident("bgra", V.LUMA, (1, 1, 0, 1, 8), V.MATRIX, 4096, 200, 7600, 2, (8192,), (50,), (1900,))
    name, a = rec.calls[-1]
    assert name == "pqa_rgb_convert_device" and [a[6].plane[p] for p in range(3)] == [8192, None, None] and list(a[6].frame_pitch) == [1900, 0, 0]
