"""The extension record blocks from pqa_create to collect: FeatureEngine.collect_blocks against collect_ext5 and collect, across
the ring wrap, under n_subsample and in a context without the features.  Everything is compared as bits, so NaNs count."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, FRAMES, BATCH = 64, 48, 24, 8


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same(got, want):
    assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


def _features():
    from pqa2_amd import _native as N
    return N.FEAT_VMAF | N.FEAT_FLOAT_SSIM | N.FEAT_CIEDE | N.FEAT_PSNR_HVS | N.FEAT_XPSNR | N.FEAT_SITI | N.FEAT_INTEGRITY


@pytest.fixture(scope="module")
def frames():
    """24 frame pairs of 64x48 4:2:0 8-bit as host planes: ([ref planes], [dis planes]) per frame."""
    from pqa2_amd import synth_torch
    clip = synth_torch.make_clip_cuda(W, H, FRAMES, 8, chroma=True)
    host = {k: [t.cpu().numpy() for t in v] for k, v in clip.items()}
    return [([np.ascontiguousarray(p[i]) for p in host["ref"]], [np.ascontiguousarray(p[i]) for p in host["dis"]])
            for i in range(FRAMES)]


def _engine(features=None, **kw):
    from pqa2_amd.engine import FeatureEngine
    return FeatureEngine(W, H, bit_depth=8, n_planes=3, chroma_shift=(1, 1), features=_features() if features is None else features,
                         max_batch=BATCH, **kw)


def _submit(eng, frames, lo, hi):
    for i in range(lo, hi):
        eng.submit(i, *frames[i])


@pytest.fixture(scope="module")
def whole(frames):
    """(records, ext, ..., ext5) of the 24 frames from one context that never wraps."""
    with _engine(result_capacity=64) as eng:
        _submit(eng, frames, 0, FRAMES)
        return eng.collect_ext5(0, FRAMES)


@pytest.mark.parametrize("blocks", [(), (4,), (0,), (1, 3), (2, 0), (0, 1, 2, 3, 4)])
def test_collect_blocks_returns_the_requested_blocks(frames, whole, blocks):
    from pqa2_amd import _native as N
    with _engine(result_capacity=64) as eng:
        _submit(eng, frames, 0, FRAMES)
        rec, got = eng.collect_blocks(0, FRAMES, blocks)
        _same(rec, eng.collect(0, FRAMES))
    _same(rec, whole[0])
    assert sorted(got) == sorted(blocks)
    for i in blocks:
        assert got[i].shape == (FRAMES, N.EXT_BLOCKS[i][1])
        _same(got[i], whole[1 + i])


def test_blocks_across_the_ring_wrap(frames, whole):
    with _engine(result_capacity=16) as eng:
        _submit(eng, frames, 0, 16)
        first = eng.collect_blocks(0, 12, range(5))
        _submit(eng, frames, 16, 24)
        second = eng.collect_blocks(12, 12, range(5))   # slots 12 ... 15, then 0 ... 7
    _same(np.concatenate([first[0], second[0]]), whole[0])
    for i in range(5):
        _same(np.concatenate([first[1][i], second[1][i]]), whole[1 + i])


def test_subsampled_rows(frames):
    from pqa2_amd import _native as N
    with _engine(result_capacity=64, n_subsample=2) as eng:
        _submit(eng, frames, 0, FRAMES)
        _, blk = eng.collect_blocks(0, FRAMES, range(5))
    odd, even = np.arange(FRAMES) % 2 == 1, np.arange(FRAMES) % 2 == 0
    # blocks 0 and 1 are written on the frames that get spatial features: index % 2 == 0
    on = {0: [N.EXT_FLOAT_SSIM, *range(N.EXT_FLOAT_SSIM_LCS, N.EXT_FLOAT_SSIM_LCS + 3), N.EXT_CIEDE2000, N.EXT_CIEDE_MEAN_DE],
          1: list(range(N.EXT2_PSNR_HVS_Y, N.EXT2_RESERVED))}
    for i, slots in on.items():
        assert np.isnan(blk[i][odd]).all()
        assert np.isfinite(blk[i][even][:, slots]).all()
    # blocks 2, 3 and 4 are written on every frame: their reserved slots are NaN, and of the others only the integrity SADs
    # of the chain start (frame 0 has no frame in front of it; siti's TI is 0 there)
    reserved = {2: N.EXT3_RESERVED, 3: N.EXT4_RESERVED, 4: N.EXT5_RESERVED}
    for i, r in reserved.items():
        assert np.isnan(blk[i][:, r:]).all()
        assert np.isfinite(blk[i][1:, :r]).all()
    assert np.isfinite(blk[2][0, :N.EXT3_RESERVED]).all()
    assert np.isfinite(blk[3][0, :N.EXT4_RESERVED]).all() and blk[3][0, N.EXT4_TI] == 0 and blk[3][0, N.EXT4_TI_SOURCE] == 0
    assert np.isnan(blk[4][0, N.EXT5_SAD_PREV:N.EXT5_SAD_PREV + 3]).all() and np.isfinite(blk[4][0, N.EXT5_BLACK_COUNT])


def test_a_context_without_the_features_hands_out_nan(frames):
    from pqa2_amd import _native as N
    with _engine(features=N.FEAT_VMAF, result_capacity=64) as eng:
        _submit(eng, frames, 0, FRAMES)
        rec, blk = eng.collect_blocks(0, FRAMES, range(5))
    assert np.isfinite(rec[:, :N.REC_MOTION + 1]).all()
    for i in range(5):
        assert blk[i].shape == (FRAMES, N.EXT_BLOCKS[i][1]) and np.isnan(blk[i]).all()
