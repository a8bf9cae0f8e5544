"""What tests/test_engine_marshal.py (CPU, a recording stand-in for the library) and tests/test_gpu_engine_views.py (MI355X)
share: one small set of samples, the layouts numpy can hold them in, and one call of every host entry of FeatureEngine that
takes planes.  50 x 38: rows are no multiple of 4 or 16 bytes, 4:2:0 chroma is 25 x 19."""
import numpy as np

W, H, NF = 50, 38, 3
LUMA, CHROMA = (H, W), (H // 2, W // 2)
SHAPES = [LUMA, CHROMA, CHROMA]
BITS = (8, 10)
RGB, C422 = (H, 4 * W), (H, W // 2)                         # BGRA rows, the chroma plane of a 4:2:2 frame
SHAPES_422 = [LUMA, C422, C422]                             # what a packed capture format unpacks to
PACKED_FORMAT = {8: "uyvy422", 10: "v210"}                  # the packed format of each bit depth, and the bytes of its rows
PACKED_ROW = {8: 2 * W, 10: (W + 5) // 6 * 16}
SMALL = (20, 30)                                            # what resample makes
NODES = (((H + 7) >> 3) + 1, ((W + 7) >> 3) + 1)            # mask nodes 8 samples apart
MATRIX = [3 << 14, 15000, -700, 900, 2 << 14, 300, 16000, -500, 1 << 14, -400, 600, 17000]


def dtype(bits):
    return np.dtype(np.uint8) if bits <= 8 else np.dtype("<u2")


def _column_slice(a):
    """columns 4 ... of a buffer whose rows are a multiple of 64 samples (luma: 64): packed 10-bit rows stay 4-byte aligned"""
    buf = np.zeros((a.shape[0], (a.shape[1] + 4 + 63) // 64 * 64), a.dtype)
    buf[:, 4:4 + a.shape[1]] = a
    return buf[:, 4:4 + a.shape[1]]


def _second_column(a):
    buf = np.zeros((a.shape[0], 2 * a.shape[1]), a.dtype)
    buf[:, ::2] = a
    return buf[:, ::2]


# layout name -> (plane, index of its frame) -> an array that holds the same samples
LAYOUTS = {
    "contiguous": lambda a, i: a.copy(),
    "column slice": lambda a, i: _column_slice(a),
    "bottom-up": lambda a, i: np.ascontiguousarray(a[::-1])[::-1],
    "second column": lambda a, i: _second_column(a),
    "wrong dtype": lambda a, i: a.astype(np.int32),
    "fortran": lambda a, i: np.asfortranarray(a),
    "one odd stride": lambda a, i: _column_slice(a) if i == 1 else a.copy(),
}
PLAIN = ("contiguous", "column slice")          # handed to the library as they lie: no copy
NON_POSITIVE = ("bottom-up",)                   # a row stride the library's entries do not agree on


class Data:
    """NF frames of every kind of input: lists of planes (ref_y, dis_y, ref_u, dis_u, fill, packed, rgb, c422) and lists of
    frames [Y, U, V] (ref3, dis3; ref422, dis422 with the chroma planes of 4:2:2)"""

    def __init__(self, bits, seed=0):
        rng = np.random.default_rng(500 + bits + 100 * seed)
        dt, top = dtype(bits), 1 << bits
        samples = lambda shape, d=dt, hi=top: [rng.integers(0, hi, shape).astype(d) for _ in range(NF)]
        self.bits = bits
        self.ref3 = [list(f) for f in zip(samples(LUMA), samples(CHROMA), samples(CHROMA))]
        self.dis3 = [list(f) for f in zip(samples(LUMA), samples(CHROMA), samples(CHROMA))]
        self.ref422 = [list(f) for f in zip(samples(LUMA), samples(C422), samples(C422))]
        self.dis422 = [list(f) for f in zip(samples(LUMA), samples(C422), samples(C422))]
        self.fill, self.c422 = samples(LUMA), samples(C422)
        self.fmt, self.packed_shape = PACKED_FORMAT[bits], (H, PACKED_ROW[bits])
        self.packed, self.rgb = samples(self.packed_shape, np.uint8, 256), samples(RGB, np.uint8, 256)
        self._split()
        self.table = rng.permutation(top).astype(dt)
        self.nodes = rng.integers(0, 257, NODES).astype(np.uint16)

    def _split(self):
        self.ref_y, self.dis_y = [f[0] for f in self.ref3], [f[0] for f in self.dis3]
        self.ref_u, self.dis_u = [f[1] for f in self.ref3], [f[1] for f in self.dis3]

    def laid(self, layout):
        """the same samples in the layout of that name"""
        lay, d = LAYOUTS[layout], object.__new__(Data)
        d.__dict__.update(self.__dict__)
        for name in ("ref3", "dis3", "ref422", "dis422"):
            setattr(d, name, [[lay(a, i) for a in f] for i, f in enumerate(getattr(self, name))])
        for name in ("fill", "packed", "rgb", "c422"):
            setattr(d, name, [lay(a, i) for i, a in enumerate(getattr(self, name))])
        d._split()
        return d


def itp_spec(bits):
    from pqa2_amd import itp
    return itp.spec("pq", bit_depth=bits)


def chroma_shift(name):
    """the chroma shifts of the context a call of that name needs: packed capture formats are 4:2:2"""
    return (1, 0) if name.startswith("submit_packed") else (1, 1)


# every host entry that takes planes: name -> call(engine, data) -> its result (None where the entry returns nothing)
CALLS = {
    "submit": lambda e, d: e.submit(4, d.ref3[0], d.dis3[0]),
    "set_dis_history_planes": lambda e, d: e.set_dis_history_planes(d.dis3[1]),
    "frame_sad": lambda e, d: e.frame_sad(d.ref3[0], d.dis3),
    "luma_stats": lambda e, d: e.luma_stats(d.ref_y, 100 << (d.bits - 8)),
    "cross_sse": lambda e, d: e.cross_sse(d.ref_y, d.dis_y, -1, 1),
    "shift_sse": lambda e, d: e.shift_sse(d.ref_y, d.dis_y, 1),
    "level_stats": lambda e, d: e.level_stats(d.ref_u, d.dis_u, 1),
    "table_apply": lambda e, d: e.table_apply(d.ref_y, d.table),
    "deinterlace frame": lambda e, d: e.deinterlace(d.ref_y, rate="frame"),
    "deinterlace field": lambda e, d: e.deinterlace(d.ref_y, first=1, rate="field"),
    "mask_blend constant": lambda e, d: e.mask_blend(d.ref_y, d.nodes, (3, 3), 7),
    "mask_blend planes": lambda e, d: e.mask_blend(d.ref_y, d.nodes, (3, 3), d.fill),
    "resample": lambda e, d: e.resample(d.ref_y, SMALL),
    "format_convert": lambda e, d: e.format_convert(d.c422, LUMA, (1, 0, 0, 0, d.bits), (1, 1, 0, 1, d.bits)),
    "unpack": lambda e, d: e.unpack(d.packed, d.fmt, LUMA),
    "unpack luma": lambda e, d: e.unpack(d.packed, d.fmt, LUMA, luma_only=True),
    "rgb_convert": lambda e, d: e.rgb_convert(d.rgb, "bgra", LUMA, (1, 1, 0, 1, d.bits), MATRIX),
    "submit_packed planar, packed": lambda e, d: e.submit_packed(0, (d.ref422, None), (d.packed, d.fmt)),
    "submit_packed packed, planar": lambda e, d: e.submit_packed(0, (d.packed, d.fmt), (d.dis422, "planar")),
    "flow_moments": lambda e, d: e.flow_moments(d.ref_y, d.dis_y, 8),
    "tile_moments": lambda e, d: e.tile_moments(d.ref_y, d.dis_y, 8),
    "band_moments": lambda e, d: e.band_moments(d.ref_y, d.dis_y, 3),
    "temporal_moments": lambda e, d: e.temporal_moments(d.ref_y, d.dis_y, 8),
    "line_profiles": lambda e, d: e.line_profiles(d.ref_y),
    "field_moments": lambda e, d: e.field_moments(d.ref_y, d.dis_y),
    "edge_profiles": lambda e, d: e.edge_profiles(d.ref_y, d.dis_y),
    "colour_moments": lambda e, d: e.colour_moments(d.ref3, d.dis3),
    "colour_apply": lambda e, d: e.colour_apply(d.dis3, MATRIX),
    "delta_itp": lambda e, d: e.delta_itp(d.ref3, d.dis3, itp_spec(d.bits)),
}


def flat(result):
    """the arrays of a result, whatever its nesting"""
    if result is None:
        return []
    if isinstance(result, np.ndarray):
        return [result]
    return [a for part in result for a in flat(part)]
