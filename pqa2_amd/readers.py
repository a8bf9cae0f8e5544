"""The reader wrappers of pipeline.score_files: each wraps a reader (yuvio.open_video's, or another wrapper) once a step has
changed a clip and offers `info`, len() and frame(i).  Five are plain host views (_LumaReader, _ShiftedReader, _CroppedReader,
_WovenReader, _LevelledReader); eight put the frames through a GPU transform on a small context of their own, eight at a time (_RunReader)."""
from __future__ import annotations

import dataclasses

import numpy as np

from . import _native as N


def _side_context(make, device, width, height, bit_depth, chroma_shift, n_planes=1):
    """a small context of its own for one side analysis or plane transform: eight pairs a call, no scoring features.
    chroma_shift None: the context is made without one (a one-plane context that never sees chroma)."""
    return make(width, height, bit_depth=bit_depth, n_planes=n_planes, **({} if chroma_shift is None else {"chroma_shift": chroma_shift}),
                features=N.FEAT_PSNR, device=device, max_batch=8, result_capacity=16)


def _clip_context(make, device, info, n_planes=1):
    """_side_context at a clip's own size, depth and chroma shifts"""
    return _side_context(make, device, info.width, info.height, info.bit_depth, (info.hshift, info.vshift), n_planes)


class _RunReader:
    """The base of the wrappers that transform frames on the GPU: a small context of its own (`eng`), frames fetched in runs of
    RUN, so that a run is one upload, one launch and one download per call, and the last run kept.  A subclass gives its
    constructor and _fetch(span): the frames of the run `span` (a range of frame numbers).  No file-descriptor path: the
    transformed samples exist in host arrays only, so the frames go down through FeatureEngine.submit.  close() frees the
    context (as does dropping the reader)."""
    RUN = 8

    def __init__(self, reader, info, eng):
        self._rd, self.info, self._eng = reader, info, eng
        self._first, self._run = 0, []

    def __len__(self):
        return len(self._rd)

    def close(self):
        self._eng.close()

    def frame(self, i: int):
        if not self._first <= i < self._first + len(self._run):
            first = i - i % self.RUN
            self._first, self._run = first, self._fetch(range(first, min(first + self.RUN, len(self))))
        return self._run[i - self._first]


class _ResampledReader(_RunReader):
    """A captured clip resampled to the reference's frame size: what score_files reads under resize=.  Every plane is resized
    to the reference's plane of the same kind (FeatureEngine.resample), one call per plane kind and run.  `info` carries the
    reference's width and height."""

    def __init__(self, reader, ref_info, filter: str, device, make):
        src = reader.info
        info = dataclasses.replace(src, width=ref_info.width, height=ref_info.height)
        self._filter, self._shapes = filter, info.plane_shapes
        super().__init__(reader, info, _side_context(make, device, ref_info.width, ref_info.height, src.bit_depth,
                                                     (src.hshift, src.vshift)))

    def _fetch(self, span):
        frames = [self._rd.frame(j) for j in span]
        planes = [self._eng.resample([f[p] for f in frames], shape, self._filter) for p, shape in enumerate(self._shapes)]
        return [[planes[p][k] for p in range(len(self._shapes))] for k in range(len(frames))]


CHROMA_SITINGS = {"left": (0, 1), "center": (1, 1), "topleft": (0, 0)}   # chroma_siting= -> (hsite, vsite)


class _ConvertedReader(_RunReader):
    """A captured clip in the reference's pixel format -- chroma layout, chroma siting and bit depth --: what score_files reads
    under chroma_mismatch="convert".  One FeatureEngine.format_convert call per plane kind and run (the luma: a depth change
    only, skipped when the depths agree; U and V in ONE call as 2n planes).  `info` carries the reference's shifts, depth and
    chroma tag.  A packed capture file is read through its numpy unpack: its packed frames are not on offer."""

    def __init__(self, reader, ref_info, siting, device, make):
        src = reader.info
        info = dataclasses.replace(src, bit_depth=ref_info.bit_depth, hshift=ref_info.hshift, vshift=ref_info.vshift,
                                   chroma_tag=ref_info.chroma_tag, packed=None)
        forced = CHROMA_SITINGS[siting] if siting is not None else None
        self.src_siting, self.dst_siting = ([(s[0] if i.hshift else 0, s[1] if i.vshift else 0) for i, s in
                                             ((src, forced or src.chroma_siting), (ref_info, forced or ref_info.chroma_siting))])
        self._luma_shape = (src.height, src.width)
        self._src = (src.hshift, src.vshift, *self.src_siting, src.bit_depth)
        self._dst = (ref_info.hshift, ref_info.vshift, *self.dst_siting, ref_info.bit_depth)
        super().__init__(reader, info, _side_context(make, device, src.width, src.height, ref_info.bit_depth,
                                                     (ref_info.hshift, ref_info.vshift)))

    def _fetch(self, span):
        frames = [self._rd.frame(j) for j in span]
        n = len(frames)
        if self._src[4] != self._dst[4]:
            luma = self._eng.format_convert([f[0] for f in frames], self._luma_shape, (0, 0, 0, 0, self._src[4]), (0, 0, 0, 0, self._dst[4]))
        else:
            luma = [f[0] for f in frames]
        chroma = self._eng.format_convert([f[1] for f in frames] + [f[2] for f in frames], self._luma_shape, self._src, self._dst)
        return [[luma[k], chroma[k], chroma[n + k]] for k in range(n)]


def yuvio_info_444(info):
    """the 4:4:4 Y'CbCr clip of an RGB clip's own size and depth: what two RGB clips are both converted to"""
    return dataclasses.replace(info, hshift=0, vshift=0, mono=False, chroma_tag="444" if info.bit_depth == 8 else f"444p{info.bit_depth}",
                               color_range=None, packed=None)


class _RgbReader(_RunReader):
    """A packed RGB clip (yuvio.RgbReader) as Y'CbCr planes in the pixel format of its partner -- chroma layout, siting, depth and
    range --: what score_files reads in place of an RGB file.  ONE FeatureEngine.rgb_convert call a run of packed frames
    (unpack, matrix, range, depth, subsampling and siting in one pass with one rounding).  `info` carries the partner's
    shifts, depth, chroma tag and range; `conversion` is the object score_files reports."""

    def __init__(self, reader, partner, siting, device, make, matrix, rgb_range, side):
        from . import rgb as RGB
        src = reader.info
        if partner.bit_depth not in N.RGB_BIT_DEPTHS:
            raise ValueError(f"a packed RGB clip is converted to 8 or 10 bit, not to the {partner.bit_depth}-bit {partner.pix_fmt} "
                             "of the other clip")
        if partner.mono:
            raise ValueError("a packed RGB clip cannot be scored against a monochrome clip")
        self.format = src.packed
        info = dataclasses.replace(src, bit_depth=partner.bit_depth, hshift=partner.hshift, vshift=partner.vshift,
                                   chroma_tag=partner.chroma_tag, color_range=partner.color_range, packed=None)
        forced = CHROMA_SITINGS[siting] if siting is not None else None
        s = forced or partner.chroma_siting
        self.dst_siting = (s[0] if partner.hshift else 0, s[1] if partner.vshift else 0)
        self.matrix = matrix or RGB.default_matrix(src.height)
        self.rgb_range = rgb_range or RGB.default_range(self.format)
        self.yuv_range = "full" if partner.color_range == "full" else "limited"
        self.coefficients = RGB.conversion_matrix(self.matrix, src.bit_depth, self.rgb_range == "full", partner.bit_depth,
                                                  self.yuv_range == "full")
        self._shape = (src.height, src.width)
        self._dst = (partner.hshift, partner.vshift, *self.dst_siting, partner.bit_depth)
        self.conversion = {"side": side, "from": src.pix_fmt, "to": info.pix_fmt, "matrix": self.matrix, "rgb_range": self.rgb_range,
                           "yuv_range": self.yuv_range, "bit_depth": [src.bit_depth, partner.bit_depth],
                           "siting": {"to": list(self.dst_siting)}, "coefficients": [int(v) for v in self.coefficients]}
        super().__init__(reader, info, _side_context(make, device, src.width, src.height, partner.bit_depth,
                                                     (partner.hshift, partner.vshift)))

    def _fetch(self, span):
        return self._eng.rgb_convert([self._rd.packed_frame(j) for j in span], self.format, self._shape, self._dst, self.coefficients)

    def __iter__(self):
        for i in range(len(self)):
            yield self.frame(i)


class _RegisteredReader(_RunReader):
    """A captured clip resampled onto the reference grid through the window of a measured geometry (the `geometry` object of
    pipeline._find_geometry): what score_files reads under register= once the map is applied.  Every plane keeps its size.
    The luma window is the measured one; a chroma plane of n_c samples along an axis gets geometry_window(d / 2^shift, s,
    n_c)."""

    def __init__(self, reader, geometry: dict, device, make):
        from . import align as AL
        info = reader.info
        self._filter = geometry["filter"]
        dx, sx = AL.window_geometry(geometry["x0_q16"], geometry["w_q16"], info.width)
        dy, sy = AL.window_geometry(geometry["y0_q16"], geometry["h_q16"], info.height)
        self._shapes = info.plane_shapes
        self.windows = [(geometry["x0_q16"], geometry["y0_q16"], geometry["w_q16"], geometry["h_q16"])]
        if not info.mono:
            (x0, ww), (y0, wh) = (AL.geometry_window(dx / (1 << info.hshift), sx, info.chroma_w),
                                  AL.geometry_window(dy / (1 << info.vshift), sy, info.chroma_h))
            self.windows += [(x0, y0, ww, wh)] * 2
        super().__init__(reader, info, _clip_context(make, device, info))

    def _fetch(self, span):
        frames = [self._rd.frame(j) for j in span]
        planes = [self._eng.resample([f[p] for f in frames], shape, self._filter, tuple(v / 65536.0 for v in win))
                  for p, (shape, win) in enumerate(zip(self._shapes, self.windows))]
        return [[planes[p][k] for p in range(len(self._shapes))] for k in range(len(frames))]


class _TableReader(_RunReader):
    """A captured clip with its sample levels mapped back through a transfer curve: plane p of every frame goes through the
    integer table tables[p] on the GPU (FeatureEngine.table_apply; None: the plane is passed on as it is), one call per
    corrected plane and run.  What score_files reads under level_align="apply" with level_curve for the planes of kind
    "curve"."""

    def __init__(self, reader, tables, device, make):
        info = reader.info
        self._tables = list(tables)
        super().__init__(reader, info, _clip_context(make, device, info, 1 if info.mono else 3))

    def _fetch(self, span):
        frames = [list(self._rd.frame(j)) for j in span]
        for p, table in enumerate(self._tables):
            if table is not None:
                for f, mapped in zip(frames, self._eng.table_apply([f[p] for f in frames], table, p)):
                    f[p] = mapped
        return frames


class _DeinterlacedReader(_RunReader):
    """An interlaced clip as a progressive one: what score_files reads under deinterlace=.  Every plane of a frame goes through
    the same FeatureEngine.deinterlace call (one call per plane kind and run): in interlaced 4:2:0 chroma row c belongs to
    field c & 1, as _WovenReader assumes.  rate "field": two frames a source frame, `info` carries the doubled fps_num.  A run
    fetches its source frames plus one neighbour each side where the clip has one and drops the neighbours' outputs, so a
    frame is the same whatever run it is fetched in and equals the whole-clip call.  The source frames of the last run are
    kept, so a clip read front to back asks the wrapped reader for every frame once and in order: a wrapped reader that converts
    in runs of its own (_RgbReader) converts each of its runs once.  Every plane needs two rows."""

    def __init__(self, reader, mode: str, first: int, rate: str, device, make):
        src = reader.info
        if min(h for h, _ in src.plane_shapes) < 2:
            raise ValueError(f"deinterlace needs planes of at least two rows: a {src.pix_fmt} clip of height {src.height} has one of "
                             f"{min(h for h, _ in src.plane_shapes)}")
        self._mode, self._order, self._rate = mode, int(first), rate
        self._per = 2 if rate == "field" else 1
        self._kept = {}                                                # source frames of the last run, by number
        info = dataclasses.replace(src, fps_num=src.fps_num * self._per, interlace="p", packed=None)
        super().__init__(reader, info, _clip_context(make, device, src, 1 if src.mono else 3))

    def __len__(self):
        return len(self._rd) * self._per

    def _fetch(self, span):
        n, per = len(self._rd), self._per
        s0, s1 = span[0] // per, span[-1] // per + 1                  # the source frames of the run
        lo, hi = max(s0 - 1, 0), min(s1 + 1, n)                        # and a neighbour each side
        frames = [self._kept[j] if j in self._kept else self._rd.frame(j) for j in range(lo, hi)]
        self._kept = dict(zip(range(lo, hi), frames))
        planes = [self._eng.deinterlace([f[p] for f in frames], self._mode, self._order, self._rate) for p in range(len(frames[0]))]
        return [[pl[k - lo * per] for pl in planes] for k in span]


class _ColourReader(_RunReader):
    """A captured clip with every frame mapped through a 3 x 4 integer matrix (FeatureEngine.colour_apply, one call a run): the
    counterpart of _LevelledReader for a map that couples the planes, and what score_files reads under
    colour_align="apply"."""

    def __init__(self, reader, matrix, device, make):
        info = reader.info
        self._m = [int(v) for v in matrix]
        super().__init__(reader, info, _clip_context(make, device, info, 3))

    def _fetch(self, span):
        return self._eng.colour_apply([self._rd.frame(j)[:3] for j in span], self._m)


class _MaskedReader(_RunReader):
    """A clip with a burnt-in overlay blended out: plane p of every frame goes through the feathered mask on the GPU
    (FeatureEngine.mask_blend, one call per plane and run) towards the constant fills[p] -- or, with `partner`, towards the
    partner clip's own plane p of the same frame.  The chroma planes take the luma grid at the step their subsampling leaves.
    What score_files reads under overlay_mask="neutral" (both clips) and "reference" (the captured clip, partner: the
    reference)."""

    def __init__(self, reader, mask, fills, partner, device, make):
        info = reader.info
        self._partner, self._fills = partner, fills
        self._nodes, s = mask["nodes"], mask["step_log2"]
        self._steps = [(s, s)] + ([] if info.mono else [(s - info.hshift, s - info.vshift)] * 2)
        super().__init__(reader, info, _clip_context(make, device, info, 1 if info.mono else 3))

    def __len__(self):
        return len(self._rd) if self._partner is None else min(len(self._rd), len(self._partner))

    def _fetch(self, span):
        frames = [list(self._rd.frame(j)) for j in span]
        towards = [self._partner.frame(j) for j in span] if self._partner is not None else None
        for p, steps in enumerate(self._steps):
            fill = [t[p] for t in towards] if towards is not None else self._fills[p]
            for f, blended in zip(frames, self._eng.mask_blend([f[p] for f in frames], self._nodes, steps, fill, p)):
                f[p] = blended
        return frames


class _LumaReader:
    """The luma of a clip as a monochrome clip: what score_files reads under chroma_mismatch="luma".  A packed capture file
    keeps its packed frames on offer: a luma-only context decodes no chroma from them."""

    def __init__(self, reader):
        self._rd = reader
        self.info = dataclasses.replace(reader.info, mono=True, hshift=0, vshift=0)
        if hasattr(reader, "packed_frame"):
            self.packed_frame = reader.packed_frame

    def __len__(self):
        return len(self._rd)

    def frame(self, i: int):
        return self._rd.frame(i)[:1]


class _ShiftedReader:
    """A clip from its frame `start` on: what score_files reads once the alignment offset is known."""

    def __init__(self, reader, start: int):
        self._rd, self._start = reader, int(start)
        self.info = reader.info
        if hasattr(reader, "packed_frame"):   # a packed capture file stays one (the scoring loop's submit_packed)
            self.packed_frame = lambda i: reader.packed_frame(i + self._start)
        for name in ("fileno", "plane_offsets", "run_stride"):   # the file-descriptor submit path, where the reader has it
            if hasattr(reader, name):
                setattr(self, name, getattr(self, "_" + name))

    def __len__(self):
        return max(0, len(self._rd) - self._start)

    def frame(self, i: int):
        return self._rd.frame(i + self._start)

    def _fileno(self):
        return self._rd.fileno()

    def _plane_offsets(self, i: int):
        return self._rd.plane_offsets(i + self._start)

    def _run_stride(self, i: int, n: int):
        return self._rd.run_stride(i + self._start, n)


class _CroppedReader:
    """A clip cut to the window of `width` x `height` luma pixels at (x0, y0): what score_files reads once the spatial shift
    is known.  Frames are strided views of the wrapped reader's planes (nothing is copied); chroma planes are cut at
    (x0 >> hshift, y0 >> vshift) to the chroma size of the window.  No file-descriptor path: rows of a window do not lie
    packed in the file, so the frames go down through FeatureEngine.submit."""

    def __init__(self, reader, x0: int, y0: int, width: int, height: int):
        src = reader.info
        if x0 < 0 or y0 < 0 or width < 1 or height < 1 or x0 + width > src.width or y0 + height > src.height:
            raise ValueError("crop window outside the frame")
        self._rd, self._x0, self._y0 = reader, int(x0), int(y0)
        self.info = dataclasses.replace(src, width=int(width), height=int(height))

    def __len__(self):
        return len(self._rd)

    def windows(self):
        """[(y0, x0, h, w)] of every plane, in samples of that plane"""
        i = self.info
        out = [(self._y0, self._x0, i.height, i.width)]
        if not i.mono:
            out += [(self._y0 >> i.vshift, self._x0 >> i.hshift, i.chroma_h, i.chroma_w)] * 2
        return out

    def frame(self, i: int):
        planes = self._rd.frame(i)
        return [p[y:y + h, x:x + w] for p, (y, x, h, w) in zip(planes, self.windows())]


class _WovenReader:
    """A captured clip with its fields put back where they belong: what score_files reads under field_align="apply".  `plan` is
    fields.weave_plan's: output frame i is frame u = u_lo + i, and its rows of parity r are the rows of parity p of captured
    frame t, (t, p) = plan["sources"][i][r] -- row slices [r::2] and [p::2] of host arrays.  EVERY plane follows the same rule: in
    interlaced 4:2:0 chroma row c belongs to field c & 1.  A row that has no partner (the last row of an odd-height plane when
    the parities are swapped) stays as captured frame u has it.  No context of its own and no file-descriptor path: the woven
    samples exist in host arrays only, so the frames go down through FeatureEngine.submit."""

    def __init__(self, reader, plan: dict):
        self._rd, self._plan = reader, plan
        self.info = reader.info

    def __len__(self):
        return self._plan["u_hi"] - self._plan["u_lo"]

    def frame(self, i: int):
        u = self._plan["u_lo"] + i
        sources = self._plan["sources"][i]
        if all(src == (u, r) for r, src in enumerate(sources)):
            return self._rd.frame(u)
        out = [np.array(p) for p in self._rd.frame(u)]
        for r, (t, p) in enumerate(sources):
            if (t, p) != (u, r):
                for dst, src in zip(out, self._rd.frame(t)):
                    rows = min(len(dst[r::2]), len(src[p::2]))
                    dst[r::2][:rows] = src[p::2][:rows]
        return out


def crop_readers(ref_rd, dis_rd, dx: int, dy: int):
    """both clips cut to their common window under the displacement (dx, dy) of the captured picture: reference pixel (x, y)
    meets captured pixel (x + dx, y + dy)"""
    w, h = ref_rd.info.width - abs(dx), ref_rd.info.height - abs(dy)
    x0, y0 = max(0, -dx), max(0, -dy)
    return _CroppedReader(ref_rd, x0, y0, w, h), _CroppedReader(dis_rd, x0 + dx, y0 + dy, w, h)


class _LevelledReader:
    """A captured clip with its sample levels mapped back onto the reference's: plane p of every frame goes through the
    integer table luts[p] (numpy.take; None: the plane is passed on as it is).  What score_files reads under
    level_align="apply".  No file-descriptor path: the mapped samples exist in host arrays only, so the frames go down
    through FeatureEngine.submit."""

    def __init__(self, reader, luts):
        self._rd, self._luts = reader, list(luts)
        self.info = reader.info

    def __len__(self):
        return len(self._rd)

    def frame(self, i: int):
        planes = self._rd.frame(i)
        return [p if k >= len(self._luts) or self._luts[k] is None else np.take(self._luts[k], p) for k, p in enumerate(planes)]
