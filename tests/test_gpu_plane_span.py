"""Planes cut out of very wide buffers: spans (row pitch x rows) of 2 GiB and more, and the row pitches pqa_submit_device
refuses (include/pqa_vmaf.h states the rules at pqa_submit_device).

The frame is 16 x 16384, 8 bit, three frames at max_batch = 2 (tests/long_planes_ref.py's clip, the sample extremes in its
last 16 rows).  All six planes (three reference, three distorted frames) lie side by side inside the rows of ONE device
allocation, 64 bytes apart (frame pitch 64), so a row pitch of 140 000 bytes gives every plane a span of 2.29 GB and 262 208
bytes one of 4.30 GB = 2^32 + 1 048 576.  Every allocation covers all bytes a kernel could address from these bases even if a
refusal were missing: rows x pitch plus a margin, and 2^32 bytes beyond the base for the refused pitches (a negative or
wrapped 32-bit offset stays below that).  One allocation at a time, freed before the next.

What the kernels of PQA_FEAT_VMAF | PQA_FEAT_PSNR | PQA_FEAT_SSIM do with a row pitch (read from the sources, before the
first run):

  * vif_s0_march_kernel, adm_march / adm_pyramid kernels, motion_march_kernel: a buffer resource of (unsigned)h x pitch
    bytes, row offsets in 32-bit registers.  Their launchers return false from a span of 2^31 bytes on and the tiled
    kernels run (launch_vif_s0_march looked at the pitch alone before this test).  launch_adm_march refuses scale 0 only --
    the first run of this test had scale 0 from the tiled kernel and scales 1-3 from the march kernel, inside the oracle
    bar but the records of neither mode -- so run_adm (pqa_api.hip) takes the whole chain tiled from that span on.
  * vif_stat_kernel (vif.hip), adm_kernel (adm.hip), motion_kernel (motion.hip): the frame's base is a 64-bit pointer
    (base + frame x frame pitch); inside the plane a buffer resource of (unsigned)h x pitch x sample size bytes, the column
    in a VGPR and gy x pitch in an SGPR, both unsigned 32-bit, added by the hardware as unsigned byte offsets and checked
    against the resource's size.  Right while h x pitch < 2^32; beyond it the product wraps, rows read 0 (pqa_device.h:
    out-of-range offsets read 0 instead of faulting) and the frame would be scored on zeros without an error -- hence the
    refusal.  Scales 1-3 read the library's own planes (at most 8192 x 8192 floats: 2^28 bytes).
  * sse_kernel, ssim_kernel (psnr_ssim.hip): plain pointers, pa + (int64_t)y * row_pitch: any pitch.
  * the keep copies of the frame histories: hipMemcpy2DAsync with the caller's pitch.
  * finalize reads partial sums only.
  Of the extension features, siti alone builds such a resource, stops at 2^31 (launch_siti: hipErrorInvalidValue) and has no
  tiled partner: refused at submit time by name.  ciede, psnr_hvs, xpsnr, cambi, integrity, the SSIM family and delta_itp
  add 64-bit row offsets to a pointer (psnr_hvs formed i x pitch, i < 8, in `int` until this change: a chroma plane of a
  few rows may have a pitch near 2^31 samples under the span rule).
"""
import numpy as np
import pytest

from tests import long_planes_ref as LP
from tests.test_gpu_long_planes import DEFAULTS, _bits, _check_oracle
from tests.test_gpu_vif_strip import _switches

pytestmark = pytest.mark.gpu

W, H, BPC = 16, 16384, 8
SLOT = 64                                   # bytes between two planes inside a row: the frame pitch
ROW = 2 * LP.N_FRAMES * SLOT                # bytes of a row the six planes use
PITCH_2G, PITCH_4G = 140_000, 262_208
MARGIN = 1 << 16
TILED = {"PQA_VIF_MFMA": "0", "PQA_ADM_MARCH": "0", "PQA_MOTION_MARCH": "0"}


def _features():
    from pqa2_amd import _native as N
    return N.FEAT_VMAF | N.FEAT_PSNR | N.FEAT_SSIM


def _engine(env=None, features=None):
    from pqa2_amd.engine import FeatureEngine
    with _switches(dict(DEFAULTS, **(env or {}))):
        return FeatureEngine(W, H, bit_depth=BPC, max_batch=LP.MAX_BATCH, features=_features() if features is None else features)


def _submit_tight(eng):
    refs, diss = LP.clip(W, H, BPC)
    for i in range(LP.N_FRAMES):
        eng.submit(i, [refs[i]], [diss[i]])
    return np.ascontiguousarray(eng.collect(0, LP.N_FRAMES))


_TIGHT = {}


def _tight(name):
    """records of the packed clip through the host path: 'default', or 'tiled' (every march kernel switched off)"""
    if name not in _TIGHT:
        with _engine(TILED if name == "tiled" else None) as eng:
            _TIGHT[name] = _submit_tight(eng)
        _TIGHT[name].setflags(write=False)
    return _TIGHT[name]


def _rows():
    """[H, ROW] bytes: reference frames 0 .. 2, then distorted frames 0 .. 2, SLOT bytes apart"""
    refs, diss = LP.clip(W, H, BPC)
    rows = np.zeros((H, ROW), np.uint8)
    for k, plane in enumerate(refs + diss):
        rows[:, k * SLOT:k * SLOT + W] = plane
    return rows


def _alloc(total_bytes):
    import torch
    return torch.zeros(total_bytes, dtype=torch.uint8, device="cuda")


def _lay_rows(buf, first_row, pitch):
    """The clip's rows into `buf`, `pitch` bytes apart (pitch may be negative), row 0 at byte first_row; -> the device
    address of reference frame 0's first row"""
    import torch
    rows = torch.from_numpy(_rows()).cuda()
    lo = first_row if pitch > 0 else first_row + (H - 1) * pitch
    assert lo >= 0 and lo + (H - 1) * abs(pitch) + ROW <= buf.numel()
    view = torch.as_strided(buf, (H, ROW), (abs(pitch), 1), lo)
    view.copy_(rows if pitch > 0 else torch.flip(rows, dims=[0]))
    torch.cuda.synchronize()
    return buf.data_ptr() + first_row


def _free():
    """after the caller dropped its reference: the bytes go back to the device before the next allocation"""
    import torch
    torch.cuda.empty_cache()


def _submit_wide(eng, base, pitch):
    eng.submit_resident(0, LP.N_FRAMES, [base], [base + LP.N_FRAMES * SLOT], [pitch], [SLOT])


def _refused(eng, base, pitch, *words):
    from pqa2_amd import _native as N
    with pytest.raises(N.PqaError) as e:
        _submit_wide(eng, base, pitch)
    assert e.value.code == N.PQA_EINVAL, str(e.value)
    for word in words:
        assert word in str(e.value), (word, str(e.value))
    return str(e.value)


def test_span_between_2_and_4_gib_runs_on_the_tiled_kernels(oracle32, oracle64):
    from pqa2_amd import _native as N
    from pqa2_amd.engine import sse_from_records
    assert (1 << 31) <= PITCH_2G * H < (1 << 32) and PITCH_2G % 16 == 0
    refs, diss = LP.clip(W, H, BPC)
    buf = _alloc(PITCH_2G * H + MARGIN)
    base = _lay_rows(buf, 0, PITCH_2G)
    try:
        with _engine() as eng:
            _submit_wide(eng, base, PITCH_2G)
            got = np.ascontiguousarray(eng.collect(0, LP.N_FRAMES))
        # with siti in the mask: refused by name before anything is launched, and the context goes on working
        with _engine(features=_features() | N.FEAT_SITI) as eng:
            msg = _refused(eng, base, PITCH_2G, "siti", "2^31")
            print(f"\n{msg}")
            after = _submit_tight(eng)
            assert np.array_equal(_bits(after), _bits(_tight("default")))
            assert np.all(np.isfinite(eng.collect_ext4(0, LP.N_FRAMES)[4][:, :4]))
    finally:
        buf = None
        _free()
    _check_oracle(got[:, :LP.N_FEAT], LP.oracle_features(oracle64, W, H, BPC), f"{W}x{H}, row pitch {PITCH_2G}")
    sse = sse_from_records(got)
    for i in range(LP.N_FRAMES):
        assert int(sse[i, 0]) == oracle32.sse_plane(diss[i], refs[i], BPC), i
        assert abs(got[i, N.REC_SSIM] - oracle32.ssim_plane(diss[i], refs[i], BPC)) < 1e-9, i
    # the fallback was taken: the bits of the tiled kernels, not those of the march kernels
    tiled, march = _tight("tiled"), _tight("default")
    assert np.array_equal(_bits(got[:, 8:17]), _bits(tiled[:, 8:17])), (got[:, 8:17] - tiled[:, 8:17])
    assert not np.array_equal(_bits(got[:, 8:16]), _bits(march[:, 8:16])) and not np.array_equal(_bits(got[1:, 16]), _bits(march[1:, 16]))
    assert np.array_equal(_bits(got[:, :8]), _bits(tiled[:, :8])) and not np.array_equal(_bits(got[:, :8]), _bits(march[:, :8]))
    assert np.array_equal(_bits(got[:, 17:]), _bits(march[:, 17:]))          # PSNR / SSIM: one kernel, any pitch


def test_refused_pitches():
    """A span of 4 GiB; a row pitch one sample below a row; a negative row pitch.  One allocation serves all three: 2^32
    bytes and more beyond each base."""
    assert PITCH_4G * H == (1 << 32) + 64 * H
    first = H * ROW                               # bytes in front of the first base: what a negative pitch could walk back over
    buf = _alloc(first + H * ROW + (1 << 32) + MARGIN)
    assert buf.numel() >= first + PITCH_4G * H + MARGIN
    try:
        base = _lay_rows(buf, first, PITCH_4G)
        with _engine() as eng:
            msg = _refused(eng, base, PITCH_4G, "reference plane 0", "2^32")
            print(f"\n{msg}")
            assert np.array_equal(_bits(_submit_tight(eng)), _bits(_tight("default")))      # nothing was launched or kept
        with _engine() as eng:
            print(_refused(eng, base, W - 1, "plane 0", "below a row"))
            print(_refused(eng, base, 0, "plane 0", "below a row"))
            assert np.array_equal(_bits(_submit_tight(eng)), _bits(_tight("default")))
        # rows ROW bytes apart, the first one last in memory: the base is the last row of a block of H rows
        base = _lay_rows(buf, first + (H - 1) * ROW, -ROW)
        with _engine() as eng:
            print(_refused(eng, base, -ROW, "plane 0", "below a row"))
            assert np.array_equal(_bits(_submit_tight(eng)), _bits(_tight("default")))
    finally:
        buf = None
        _free()
