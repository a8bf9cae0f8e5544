"""The shape of pipeline.score_files that no per-feature test pins: the run cache of the reader wrappers that own a GPU
context, that a run closes every context it made exactly once, and which of two bad options is reported."""
import dataclasses

import numpy as np
import pytest

from tests import mask_ref as MR

W = H = 16
N_FRAMES = 11


class CountingReader:
    """N_FRAMES frames of W x H 4:2:0, every sample of frame i equal to i; logs the frames asked for"""

    def __init__(self, n=N_FRAMES, packed=None):
        from pqa2_amd import synth
        self.info = dataclasses.replace(synth.clip_info(W, H), packed=packed)
        self.n, self.log = n, []

    def __len__(self):
        return self.n

    def frame(self, i):
        assert 0 <= i < self.n
        self.log.append(i)
        return [np.full((H, W), i, np.uint8), np.full((H // 2, W // 2), i, np.uint8), np.full((H // 2, W // 2), i, np.uint8)]

    packed_frame = frame      # what _RgbReader reads; the identity engine hands the three arrays on as the planes


class IdentityEngine:
    """every plane transform hands its input on; counts its close() calls"""
    made = []

    def __init__(self, width, height, **kw):
        self.kw, self.closed = kw, 0
        IdentityEngine.made.append(self)

    def close(self):
        self.closed += 1

    def resample(self, planes, shape, filter, window=None):
        return list(planes)

    def format_convert(self, planes, luma_shape, src, dst):
        return list(planes)

    def rgb_convert(self, packed, fmt, shape, dst, coefficients):
        return [list(f) for f in packed]

    def table_apply(self, planes, table, plane=0):
        return list(planes)

    def colour_apply(self, frames, matrix):
        return [list(f) for f in frames]

    def mask_blend(self, planes, nodes, steps, fill, plane=0):
        return list(planes)


def _wrappers():
    from pqa2_amd import pipeline as P
    info = CountingReader().info
    geometry = {"filter": "bicubic", "x0_q16": 0, "y0_q16": 0, "w_q16": W << 16, "h_q16": H << 16}
    mask = {"nodes": np.zeros((3, 3), np.uint16), "step_log2": 3}
    return {
        "resampled": lambda rd: P._ResampledReader(rd, info, "bicubic", 0, IdentityEngine),
        "converted": lambda rd: P._ConvertedReader(rd, info, None, 0, IdentityEngine),
        "rgb": lambda rd: P._RgbReader(rd, info, None, 0, IdentityEngine, None, None, "distorted"),
        "registered": lambda rd: P._RegisteredReader(rd, geometry, 0, IdentityEngine),
        "table": lambda rd: P._TableReader(rd, [np.arange(256), None, None], 0, IdentityEngine),
        "colour": lambda rd: P._ColourReader(rd, [0] * 12, 0, IdentityEngine),
        "masked": lambda rd: P._MaskedReader(rd, mask, [16, 128, 128], None, 0, IdentityEngine),
    }


@pytest.mark.parametrize("name", ["resampled", "converted", "rgb", "registered", "table", "colour", "masked"])
def test_run_cache(name):
    src = CountingReader(packed="bgra" if name == "rgb" else None)
    IdentityEngine.made.clear()
    rd = _wrappers()[name](src)
    assert len(IdentityEngine.made) == 1 and len(rd) == N_FRAMES and src.log == []
    for i in range(N_FRAMES):
        planes = rd.frame(i)
        assert len(planes) == 3 and all(int(p[0, 0]) == i for p in planes)
    assert src.log == list(range(N_FRAMES))             # the runs [0, 8) and [8, 11), once each
    assert int(rd.frame(9)[0][0, 0]) == 9 and src.log == list(range(N_FRAMES))     # still the kept run
    assert int(rd.frame(3)[0][0, 0]) == 3 and src.log == list(range(N_FRAMES)) + list(range(8))   # [0, 8) again
    assert IdentityEngine.made[0].closed == 0
    rd.close()
    assert [e.closed for e in IdentityEngine.made] == [1]


def test_masked_reader_ends_with_its_partner():
    from pqa2_amd import pipeline as P
    src, partner = CountingReader(), CountingReader(9)
    IdentityEngine.made.clear()
    rd = P._MaskedReader(src, {"nodes": np.zeros((3, 3), np.uint16), "step_log2": 3}, None, partner, 0, IdentityEngine)
    assert len(rd) == 9
    for i in range(9):
        assert int(rd.frame(i)[0][0, 0]) == i
    assert src.log == list(range(9)) and partner.log == list(range(9))      # the last run is [8, 9)
    rd.close()
    assert [e.closed for e in IdentityEngine.made] == [1]


# ---- score_files through the oracle stand-in ---------------------------------------------------------------------------------
CW, CH, CN = 96, 64, 4


@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    from pqa2_amd import synth
    from pqa2_amd.yuvio import write_y4m
    d = tmp_path_factory.mktemp("steps")
    info = synth.clip_info(CW, CH)
    refs, clean = synth.make_clip(CW, CH, CN)
    logo = [[MR.checker_logo(f[0], (37, 19, 69, 35)), f[1], f[2]] for f in clean]
    paths = {}
    for key, clip in (("ref", refs), ("logo", logo)):
        paths[key] = str(d / (key + ".y4m"))
        write_y4m(paths[key], clip, info)
    return paths


def _counting_factory():
    from tests.fake_engine import OracleEngine

    class Counted(OracleEngine):
        """the oracle stand-in plus the restated tile moments and mask blend; counts close() and release()"""

        def __init__(self, width, height, **kw):
            super().__init__(width, height, **kw)
            self.bits, self.closed = kw.get("bit_depth", 8), 0

        def close(self):
            self.closed += 1
            super().close()

        def release(self):      # what score_files prefers for a healthy scoring context
            self.closed += 1

        def tile_moments(self, ref_frames, dis_frames, tile=32):
            return MR.tile_moments(ref_frames, dis_frames, tile)

        def mask_blend(self, frames, nodes, steps, fill, plane=0):
            return [MR.blend(np.asarray(f), nodes, *steps, fill if isinstance(fill, int) else np.asarray(fill[k]), self.bits)
                    for k, f in enumerate(frames)]

    made = []

    def make(*a, **kw):
        made.append(Counted(*a, **kw))
        return made[-1]
    return make, made


def test_every_context_is_closed_once(clips):
    from pqa2_amd.pipeline import score_files
    make, made = _counting_factory()
    res = score_files(clips["ref"], clips["logo"], "vmaf_v0.6.1", engine_factory=make, overlay_mask="neutral")
    assert res["overlay"]["applied"]
    # the sampled measurement, a masked reader a clip, the scoring context
    assert len(made) == 4 and [e.closed for e in made] == [1] * 4


@pytest.mark.parametrize("options, message", [
    (dict(resize="nearest", align=-1), "resize must be None or one of"),
    (dict(spatial_align=99, distortion_map=7), "spatial_align must be 0 ... 16 pixels"),
    (dict(level_curve=True, spectrum=9), "level_curve needs level_align"),
    (dict(overlay_mask="report", overlay_feather=3, temporal=5), "overlay_feather must be a multiple of 8, or 0"),
    (dict(overlay_feather=3, temporal=5), "temporal must be 0 or a tile size"),      # no mask asked for: the feather is not looked at
    (dict(chroma_siting="x", rgb_matrix="x"), "chroma_siting must be None"),
])
def test_the_earlier_step_reports_its_bad_option(clips, options, message):
    """two bad options, one of an earlier and one of a later step: the earlier step's message is the one raised.  overlay_feather
    is looked at only when a mask is asked for, hence overlay_mask="report"; without it the later step's message is raised"""
    import re
    from pqa2_amd.pipeline import score_files
    from tests.fake_engine import OracleEngine
    with pytest.raises(ValueError, match=re.escape(message)):
        score_files(clips["ref"], clips["logo"], "vmaf_v0.6.1", engine_factory=OracleEngine, **options)
