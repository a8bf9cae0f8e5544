"""GPU parity: HIP kernels (through the C ABI) vs the CPU oracle on identical seeded inputs.

Tolerances (written here because floating-point parity is a tolerance, not bit-equality):
  * VIF / ADM num and den per scale: relative 5e-5 against the f64 oracle.  Rationale: libvmaf's own
    f32 arithmetic (oracle f32) sits ~1e-6 from f64; the kernels use FMA, v_rcp_f32/v_log_f32
    (1 ulp) and double cross-tile sums, which lands them at a few 1e-6.
  * motion: absolute 2e-5 (values are O(1..20)).
  * VMAF score from those features: |delta| <= 0.01 (north_star), asserted in test_gpu_engine.py.
  * PSNR SSE: bit-exact integers.  SSIM: 1e-9 absolute (same float window expression, double sum).
"""
import numpy as np
import pytest

from pqa2_amd import synth

pytestmark = pytest.mark.gpu

REL_TOL = 5e-5
MOTION_ATOL = 2e-5


def _engine(w, h, **kw):
    from pqa2_amd.engine import FeatureEngine
    return FeatureEngine(w, h, **kw)


def _oracle_clip(orc, refs, diss, bpc, **kw):
    return orc.clip_features([r[0] for r in refs], [d[0] for d in diss], bpc, **kw)


@pytest.mark.parametrize("w,h", [(64, 48), (176, 144), (321, 241), (130, 18), (16, 16), (640, 362)])
def test_vmaf_features_8bit(oracle32, oracle64, w, h):
    from pqa2_amd import _native as N
    n = 4
    refs, diss = synth.make_clip(w, h, n, 8, chroma=False)
    exp64 = _oracle_clip(oracle64, refs, diss, 8)
    exp32 = _oracle_clip(oracle32, refs, diss, 8)
    with _engine(w, h, max_batch=3) as eng:   # batch 3 over 4 frames: exercises the partial batch + motion carry
        for i in range(n):
            eng.submit(i, refs[i], diss[i])
        rec = eng.collect(0, n)
    got = rec[:, :17]
    rel = np.abs(got[:, :16] - exp64[:, :16]) / np.maximum(np.abs(exp64[:, :16]), 1e-12)
    rel32 = np.abs(exp32[:, :16] - exp64[:, :16]) / np.maximum(np.abs(exp64[:, :16]), 1e-12)
    print(f"\n{w}x{h}: max rel err gpu-vs-f64 {rel.max():.3e} (oracle f32-vs-f64 {rel32.max():.3e}); "
          f"motion abs err {np.abs(got[:, 16] - exp64[:, 16]).max():.3e}")
    assert rel.max() < REL_TOL, f"feature mismatch at {np.unravel_index(rel.argmax(), rel.shape)}"
    assert np.abs(got[:, 16] - exp64[:, 16]).max() < MOTION_ATOL
    assert got[0, 16] == 0.0


@pytest.mark.parametrize("w,h,bpc", [(64, 48, 8), (321, 241, 8), (130, 18, 8), (16, 16, 8), (200, 120, 10)])
def test_vif_integer_border(oracle64, w, h, bpc):
    """pqa_config.vif_border = PQA_VIF_BORDER_INTEGER: integer_vif.c's reflect-101 padding (what the default
    models' extractor uses); ADM and motion are untouched by the switch."""
    from pqa2_amd import _native as N
    n = 2
    refs, diss = synth.make_clip(w, h, n, bpc, chroma=False)
    exp = _oracle_clip(oracle64, refs, diss, bpc, vif_border101=True)
    exp_float = _oracle_clip(oracle64, refs, diss, bpc)
    assert np.abs(exp[:, :8] - exp_float[:, :8]).max() > 0 and np.array_equal(exp[:, 8:], exp_float[:, 8:])
    with _engine(w, h, bit_depth=bpc, vif_border=N.VIF_BORDER_INTEGER) as eng:
        for i in range(n):
            eng.submit(i, refs[i], diss[i])
        got = eng.collect(0, n)[:, :17]
    rel = np.abs(got[:, :16] - exp[:, :16]) / np.maximum(np.abs(exp[:, :16]), 1e-12)
    assert rel.max() < REL_TOL, f"feature mismatch at {np.unravel_index(rel.argmax(), rel.shape)}"
    assert np.abs(got[:, 16] - exp[:, 16]).max() < MOTION_ATOL


@pytest.mark.parametrize("w,h,bpc,gain", [(64, 48, 8, 100.0), (321, 241, 8, 100.0), (130, 18, 8, 100.0), (16, 16, 8, 100.0),
                                          (640, 362, 8, 1.0), (200, 120, 10, 100.0), (96, 80, 12, 1.0)])
def test_fixed_point_is_bit_exact(w, h, bpc, gain):
    """pqa_config.fixed_point: integer_vif.c's, integer_adm.c's and integer_motion.c's arithmetic in HIP
    (csrc/vif_fixed.hip, adm_fixed.hip, motion_fixed.hip).  Integer work, so the bar is bit-equality of all 17
    feature doubles with the fixed-point restatement (oracle/vmaf_int_oracle.c)."""
    from oracle.int_oracle import IntOracle
    from pqa2_amd import _native as N
    into = IntOracle()
    n = 3
    refs, diss = synth.make_clip(w, h, n, bpc, chroma=False)
    want = np.stack([into.vif(refs[i][0], diss[i][0], bpc, gain) for i in range(n)])
    want_adm = np.stack([into.adm(refs[i][0], diss[i][0], bpc, gain) for i in range(n)])
    blur = [into.motion_blur(refs[i][0], bpc) for i in range(n)]
    want_motion = [0.0] + [into.motion_score(into.motion_sad(blur[i - 1], blur[i]), w, h) for i in range(1, n)]
    with _engine(w, h, bit_depth=bpc, fixed_point=N.FIXED_ALL, vif_enhn_gain_limit=gain, adm_enhn_gain_limit=gain,
                 max_batch=2) as eng:
        for i in range(n):
            eng.submit(i, refs[i], diss[i])
        got = eng.collect(0, n)[:, :17]
    assert np.array_equal(got[:, :8].view(np.uint64), want.view(np.uint64)), np.abs(got[:, :8] - want).max()
    assert got[:, 16].tolist() == want_motion
    assert np.array_equal(got[:, 8:16].view(np.uint64), want_adm.view(np.uint64)), np.abs(got[:, 8:16] - want_adm).max()


@pytest.mark.parametrize("bpc", [10, 12])
def test_vmaf_features_hbd(oracle64, bpc):
    w, h, n = 200, 120, 3
    refs, diss = synth.make_clip(w, h, n, bpc, chroma=False)
    exp = _oracle_clip(oracle64, refs, diss, bpc)
    with _engine(w, h, bit_depth=bpc) as eng:
        for i in range(n):
            eng.submit(i, refs[i], diss[i])
        got = eng.collect(0, n)[:, :17]
    rel = np.abs(got[:, :16] - exp[:, :16]) / np.maximum(np.abs(exp[:, :16]), 1e-12)
    assert rel.max() < REL_TOL
    assert np.abs(got[:, 16] - exp[:, 16]).max() < MOTION_ATOL


def test_neg_model_gain_limits(oracle64):
    """vmaf_*neg models set vif/adm enhn_gain_limit = 1.0 (models/vmaf_v0.6.1neg.json feature_opts_dicts)."""
    w, h, n = 176, 144, 2
    refs, diss = synth.make_clip(w, h, n, 8, chroma=False)
    # make the distorted clip an *enhanced* (sharpened) version so the gain limit bites
    diss = [[np.clip(2.0 * r[0].astype(np.float32) - d[0].astype(np.float32), 0, 255).astype(np.uint8)]
            for r, d in zip(refs, diss)]
    exp = _oracle_clip(oracle64, refs, diss, 8, vif_gain_limit=1.0, adm_gain_limit=1.0)
    exp_default = _oracle_clip(oracle64, refs, diss, 8)
    assert np.abs(exp - exp_default).max() > 1e-3  # the option matters on this input
    with _engine(w, h, vif_enhn_gain_limit=1.0, adm_enhn_gain_limit=1.0) as eng:
        for i in range(n):
            eng.submit(i, refs[i], diss[i])
        got = eng.collect(0, n)[:, :17]
    rel = np.abs(got[:, :16] - exp[:, :16]) / np.maximum(np.abs(exp[:, :16]), 1e-12)
    assert rel.max() < REL_TOL


def test_identical_and_static_closed_forms():
    """identical ref/dis -> every vif_scale = 1, adm = 1, SSE = 0, SSIM = 1; static clip -> motion = 0."""
    from pqa2_amd import _native as N
    from pqa2_amd.engine import sse_from_records
    w, h = 192, 108
    ref, _ = synth.make_pair(w, h, 0, 8, chroma=True)
    with _engine(w, h, n_planes=3, features=N.FEAT_ALL) as eng:
        for i in range(3):
            eng.submit(i, ref, ref)
        rec = eng.collect(0, 3)
    np.testing.assert_allclose(rec[:, 0:4] / rec[:, 4:8], 1.0, rtol=0, atol=1e-6)
    np.testing.assert_allclose(rec[:, 8:12] / rec[:, 12:16], 1.0, rtol=0, atol=1e-6)
    assert np.all(rec[:, 16] == 0.0)
    assert np.all(sse_from_records(rec) == 0)
    np.testing.assert_allclose(rec[:, 17:20], 1.0, atol=1e-12)


@pytest.mark.parametrize("bpc,w,h", [(8, 322, 242), (8, 64, 48), (10, 200, 120), (8, 1920, 1080), (12, 64, 48), (12, 322, 242)])
def test_psnr_sse_bit_exact_and_ssim(oracle32, bpc, w, h):
    from pqa2_amd import _native as N
    from pqa2_amd.engine import sse_from_records
    n = 2
    refs, diss = synth.make_clip(w, h, n, bpc, chroma=True)
    with _engine(w, h, bit_depth=bpc, n_planes=3, features=N.FEAT_PSNR | N.FEAT_SSIM) as eng:
        for i in range(n):
            eng.submit(i, refs[i], diss[i])
        rec = eng.collect(0, n)
    sse = sse_from_records(rec)
    for i in range(n):
        for p in range(3):
            assert int(sse[i, p]) == oracle32.sse_plane(diss[i][p], refs[i][p], bpc), (i, p)
            exp = oracle32.ssim_plane(diss[i][p], refs[i][p], bpc)
            assert abs(rec[i, 17 + p] - exp) < 1e-9, (i, p, rec[i, 17 + p], exp)


def _extreme_pairs(w, h, bpc):
    """(name, ref, dis) luma planes at the ends of the sample range; every pair but the last differs by `top` everywhere."""
    top = (1 << bpc) - 1
    dt = np.uint8 if bpc <= 8 else np.uint16
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for period in (1, 4):
        board = ((((xx // period) + (yy // period)) % 2) * top).astype(dt)
        out.append((f"checkerboard of period {period}", board, (top - board).astype(dt)))
    out.append(("flat top against flat 0", np.full((h, w), top, dt), np.zeros((h, w), dt)))
    out.append(("top against top", np.full((h, w), top, dt), np.full((h, w), top, dt)))
    return out


@pytest.mark.parametrize("bpc", [8, 10, 12])
@pytest.mark.parametrize("w,h", [(66, 50), (322, 242)])
def test_psnr_ssim_sample_extremes(oracle32, bpc, w, h):
    """0 / top checkerboards against their inverses, flat top against flat 0, top against top: the largest ss, s12 and
    vars * 64 the SSIM kernel forms and the largest squared differences of both SSE paths (the SSIM kernel's block sums with
    PSNR | SSIM, sse_kernel alone and on the remainder strips: neither size is a multiple of 4).  Chroma planes (4:2:0) hold
    the same patterns."""
    from pqa2_amd import _native as N
    from pqa2_amd.engine import sse_from_records
    top = (1 << bpc) - 1
    cw, ch = (w + 1) // 2, (h + 1) // 2
    pairs = list(zip(_extreme_pairs(w, h, bpc), _extreme_pairs(cw, ch, bpc)))
    n = len(pairs)
    refs = [[y[1], c[1], c[1]] for y, c in pairs]
    diss = [[y[2], c[2], c[2]] for y, c in pairs]
    recs = {}
    for feats in (N.FEAT_PSNR | N.FEAT_SSIM, N.FEAT_PSNR):
        with _engine(w, h, bit_depth=bpc, n_planes=3, features=feats, max_batch=3) as eng:
            for i in range(n):
                eng.submit(i, refs[i], diss[i])
            recs[feats] = eng.collect(0, n)
    rec = recs[N.FEAT_PSNR | N.FEAT_SSIM]
    for i, ((name, _, _), _) in enumerate(pairs):
        for p, (pw, ph) in enumerate(((w, h), (cw, ch), (cw, ch))):
            want = 0 if name == "top against top" else pw * ph * top * top
            assert oracle32.sse_plane(diss[i][p], refs[i][p], bpc) == want, (name, p)
            for feats, r in recs.items():
                assert int(sse_from_records(r)[i, p]) == want, (name, p, feats)
            exp = oracle32.ssim_plane(diss[i][p], refs[i][p], bpc)
            assert abs(rec[i, 17 + p] - exp) < 1e-9, (name, p, rec[i, 17 + p], exp)
            if name == "top against top":
                assert exp == 1.0
            else:
                assert exp < 0.05, (name, p, exp)     # nothing in common: the ends of the range in every window


@pytest.mark.parametrize("bpc", [8, 10])
def test_psnr_ssim_unaligned_resident_planes(oracle32, bpc):
    """Three device-resident planes whose bases sit 0 ... 3 samples into their allocations and whose row pitches are odd
    numbers of samples: every combination of the `aligned` (16 bytes) and `aligned4` tests that choose the kernels' load
    paths fails or holds.  Bit-equal to the host path (whose staging is 64-byte aligned), and equal to the oracle."""
    import torch
    from pqa2_amd import _native as N
    from pqa2_amd.engine import sse_from_records
    w, h, n = 150, 86, 2
    es = 1 if bpc <= 8 else 2
    feats = N.FEAT_PSNR | N.FEAT_SSIM
    refs, diss = synth.make_clip(w, h, n, bpc, chroma=True)
    with _engine(w, h, bit_depth=bpc, n_planes=3, features=feats) as eng:
        for i in range(n):
            eng.submit(i, refs[i], diss[i])
        host = eng.collect(0, n)
    sse = sse_from_records(host)
    for i in range(n):
        for p in range(3):
            assert int(sse[i, p]) == oracle32.sse_plane(diss[i][p], refs[i][p], bpc), (i, p)
            assert abs(host[i, 17 + p] - oracle32.ssim_plane(diss[i][p], refs[i][p], bpc)) < 1e-9, (i, p)

    def resident(clip, p, off, pitch):
        """(tensor, device pointer of frame 0) of plane p of every frame: rows `pitch` samples apart, `off` samples in"""
        ph, pw = clip[0][p].shape
        buf = np.zeros(off + n * ph * pitch + 8, clip[0][p].dtype)
        buf[off:off + n * ph * pitch].reshape(n, ph, pitch)[:, :, :pw] = np.stack([f[p] for f in clip])
        t = torch.from_numpy(buf.view(np.int16) if es == 2 else buf).cuda()
        return t, t.data_ptr() + off * es

    for off in range(4):
        keep, rp, dp, row_pitch, frame_pitch = [], [], [], [], []
        for p in range(3):
            ph, pw = refs[0][p].shape
            pitch = pw + 3 + (pw % 2)            # odd, and not the width
            assert pitch % 2 == 1
            for clip, ptrs in ((refs, rp), (diss, dp)):
                t, ptr = resident(clip, p, off + p, pitch)      # a different base alignment per plane
                keep.append(t)
                ptrs.append(ptr)
            row_pitch.append(pitch * es)
            frame_pitch.append(ph * pitch * es)
        torch.cuda.synchronize()
        with _engine(w, h, bit_depth=bpc, n_planes=3, features=feats) as eng:
            eng.submit_resident(0, n, rp, dp, row_pitch, frame_pitch)
            dev = eng.collect(0, n)
        assert np.array_equal(host, dev), (bpc, off)
        del keep


def test_constant_offset_sse_closed_form():
    from pqa2_amd import _native as N
    from pqa2_amd.engine import sse_from_records
    w, h, c = 130, 70, 7
    ref = [np.full((h, w), 100, np.uint8)]
    dis = [np.full((h, w), 100 + c, np.uint8)]
    with _engine(w, h, features=N.FEAT_PSNR) as eng:
        eng.submit(0, ref, dis)
        rec = eng.collect(0, 1)
    assert int(sse_from_records(rec)[0, 0]) == c * c * w * h


def test_resident_path_matches_host_path_and_halo():
    """Device-resident submit (torch tensor in HBM) == host submit, including the sharding halo."""
    import torch
    from pqa2_amd import _native as N
    w, h, n = 256, 144, 6
    refs, diss = synth.make_clip(w, h, n, 8, chroma=False)
    with _engine(w, h, max_batch=4) as eng:
        for i in range(n):
            eng.submit(i, refs[i], diss[i])
        host = eng.collect(0, n)
    R = torch.from_numpy(np.stack([r[0] for r in refs])).cuda()
    D = torch.from_numpy(np.stack([d[0] for d in diss])).cuda()
    torch.cuda.synchronize()
    with _engine(w, h, max_batch=4) as eng:
        eng.submit_resident(0, n, [R.data_ptr()], [D.data_ptr()], [w], [w * h])
        dev = eng.collect(0, n)
    assert np.array_equal(host, dev)  # fixed-order reductions: bit-identical
    # second half as its own shard with a one-frame halo
    with _engine(w, h, max_batch=4) as eng:
        eng.submit_resident(3, 3, [R[3:].data_ptr()], [D[3:].data_ptr()], [w], [w * h],
                            prev_ref_luma_ptr=R[2].data_ptr(), prev_row_pitch=w)
        shard = eng.collect(3, 3)
    assert np.array_equal(shard, host[3:])


def test_n_subsample_and_cancel():
    from pqa2_amd import _native as N
    w, h, n = 128, 96, 5
    refs, diss = synth.make_clip(w, h, n, 8, chroma=False)
    with _engine(w, h) as eng:
        for i in range(n):
            eng.submit(i, refs[i], diss[i])
        full = eng.collect(0, n)
    with _engine(w, h, n_subsample=2, max_batch=4) as eng:
        for i in range(n):
            eng.submit(i, refs[i], diss[i])
        sub = eng.collect(0, n)
    assert np.array_equal(sub[::2, :16], full[::2, :16])      # spatial features on frames 0, 2, 4
    assert np.array_equal(sub[:, 16], full[:, 16])            # motion on every frame
    # the fixed-point mode goes through the same slot mapping (its own finalize kernels) and a wrapping record ring
    with _engine(w, h, fixed_point=N.FIXED_ALL) as eng:
        for i in range(n):
            eng.submit(i, refs[i], diss[i])
        fx_full = eng.collect(0, n)
    with _engine(w, h, fixed_point=N.FIXED_ALL, n_subsample=2, max_batch=3, result_capacity=4) as eng:
        for i in range(n):
            eng.submit(i, refs[i], diss[i])
            if i == 2:
                first = eng.collect(0, 3)
        fx_sub = np.concatenate([first, eng.collect(3, 2)])
    assert np.array_equal(fx_sub[::2, :16], fx_full[::2, :16]) and np.array_equal(fx_sub[:, 16], fx_full[:, 16])
    assert not np.array_equal(fx_full[:, :16], full[:, :16])
    with _engine(w, h) as eng:
        eng.submit(0, refs[0], diss[0])
        eng.cancel()
        with pytest.raises(N.PqaCancelled):
            eng.submit(1, refs[1], diss[1])
        eng.reset()
        eng.submit(0, refs[0], diss[0])
        assert np.array_equal(eng.collect(0, 1)[:, :16], full[:1, :16])


def test_bad_config_is_rejected():
    from pqa2_amd import _native as N
    with pytest.raises(N.PqaError):
        _engine(8, 8)
    with pytest.raises(N.PqaError):
        _engine(64, 64, bit_depth=9)


@pytest.mark.parametrize("shift,tag", [((0, 0), "444"), ((1, 0), "422"), ((1, 1), "420")])
def test_chroma_layouts_psnr_ssim(oracle32, shift, tag):
    """4:4:4 / 4:2:2 / 4:2:0 chroma planes through the PSNR / SSIM kernels (odd luma size: ceil-shifted chroma)."""
    from pqa2_amd import _native as N
    from pqa2_amd.engine import sse_from_records
    w, h = 150, 86
    cw, ch = -(-w >> shift[0]), -(-h >> shift[1])
    rng = np.random.default_rng(5)
    ref = [rng.integers(0, 256, (h, w), dtype=np.uint8)] + [rng.integers(0, 256, (ch, cw), dtype=np.uint8) for _ in range(2)]
    dis = [np.clip(p.astype(np.int16) + rng.integers(-9, 10, p.shape), 0, 255).astype(np.uint8) for p in ref]
    with _engine(w, h, n_planes=3, chroma_shift=shift, features=N.FEAT_PSNR | N.FEAT_SSIM) as eng:
        eng.submit(0, ref, dis)
        rec = eng.collect(0, 1)
    sse = sse_from_records(rec)
    for p in range(3):
        assert int(sse[0, p]) == oracle32.sse_plane(dis[p], ref[p], 8), (tag, p)
        assert abs(rec[0, 17 + p] - oracle32.ssim_plane(dis[p], ref[p], 8)) < 1e-9, (tag, p)


def test_unaligned_pitch_and_strided_rows(oracle64):
    """Host planes that are views with a row stride (cropped from a wider buffer) and an odd width."""
    w, h = 203, 77
    big_r, big_d = synth.make_clip(256, 96, 2, 8, chroma=False)
    refs = [[f[0][5:5 + h, 11:11 + w]] for f in big_r]      # non-contiguous views, odd offsets
    diss = [[f[0][5:5 + h, 11:11 + w]] for f in big_d]
    exp = oracle64.clip_features([np.ascontiguousarray(r[0]) for r in refs], [np.ascontiguousarray(d[0]) for d in diss], 8)
    with _engine(w, h) as eng:
        for i in range(2):
            eng.submit(i, refs[i], diss[i])
        got = eng.collect(0, 2)[:, :17]
    rel = np.abs(got[:, :16] - exp[:, :16]) / np.abs(exp[:, :16])
    assert rel.max() < REL_TOL and np.abs(got[:, 16] - exp[:, 16]).max() < MOTION_ATOL


def test_torch_stream_and_profile_hooks():
    import torch
    w, h, n = 320, 180, 4
    refs, diss = synth.make_clip(w, h, n, 8, chroma=False)
    R = torch.from_numpy(np.stack([r[0] for r in refs])).cuda()
    D = torch.from_numpy(np.stack([d[0] for d in diss])).cuda()
    torch.cuda.synchronize()
    with _engine(w, h) as eng:
        eng.submit_resident(0, n, [R.data_ptr()], [D.data_ptr()], [w], [w * h])
        base = eng.collect(0, n)
    s = torch.cuda.Stream()
    with _engine(w, h) as eng:
        eng._check(eng.lib.pqa_set_stream(eng._ctx, s.cuda_stream))
        eng.profile_enable([0, 7, 11])
        eng.submit_resident(0, n, [R.data_ptr()], [D.data_ptr()], [w], [w * h])
        got = eng.collect(0, n)
        prof = eng.profile_read()
    assert np.array_equal(base, got)
    assert prof["vif_stat_s0"]["launches"] == 1 and prof["vif_stat_s0"]["frames"] == n and prof["vif_stat_s0"]["ms"] > 0
    assert prof["adm_scale_s0"]["launches"] == 1 and prof["motion"]["launches"] == 1
    assert prof["vif_stat_s1"]["launches"] == 0        # not in the mask


def test_result_ring_wraps():
    w, h, n = 64, 64, 10
    refs, diss = synth.make_clip(w, h, n, 8, chroma=False)
    with _engine(w, h, max_batch=2) as eng:
        for i in range(n):
            eng.submit(i, refs[i], diss[i])
        full = eng.collect(0, n)
    with _engine(w, h, max_batch=2, result_capacity=4) as eng:   # ring of 4 records
        out = []
        for i in range(n):
            eng.submit(i, refs[i], diss[i])
            if i % 3 == 2:
                out.append(eng.collect(i - 2, 3))
        out.append(eng.collect(9, 1))
    assert np.array_equal(np.concatenate(out), full)


@pytest.mark.parametrize("bpc,w,h", [(8, 1920, 1080), (8, 333, 77), (10, 640, 360)])
def test_luma_stats_exact(bpc, w, h):
    """sum / sum of squares / count-above-threshold per frame: exact integers (bookend detection inputs)."""
    import torch
    n = 5
    rng = np.random.default_rng(11)
    peak = (1 << bpc) - 1
    clip = rng.integers(0, peak + 1, (n, h, w)).astype(np.uint8 if bpc <= 8 else np.uint16)
    clip[1] = peak  # a white frame
    thr = 200 << (bpc - 8)
    t = torch.from_numpy(clip.view(np.int16) if bpc > 8 else clip).cuda()
    torch.cuda.synchronize()
    es = 1 if bpc <= 8 else 2
    with _engine(w, h, bit_depth=bpc, max_batch=2) as eng:
        got = eng.luma_stats_resident(t.data_ptr(), w * es, w * h * es, n, thr)
    c = clip.astype(np.int64)
    want = np.stack([c.sum((1, 2)), (c * c).sum((1, 2)), (c > thr).sum((1, 2))], 1).astype(np.uint64)
    assert np.array_equal(got, want)
    from pqa2_amd import bookend
    mean, std, ratio = bookend.brightness_from_stats(got, w * h)
    assert bookend.starts_with_bookend(ratio) and ratio[1] == 1.0 and std[1] == 0.0


def test_random_geometry_sweep(oracle64, oracle32):
    """Seeded sweep over odd / tiny / non-tile-multiple geometries and content types (noise, flat patches,
    ramps), every feature at once, against the oracle: tile seams, halo mirroring and masked lanes."""
    from pqa2_amd import _native as N
    from pqa2_amd.engine import sse_from_records
    from pqa2_amd import model as M_
    mdl_ = M_.load_model("vmaf_v0.6.1")
    rng = np.random.default_rng(20250418)
    sizes = [(16, 16), (17, 31), (61, 29), (63, 63), (121, 15 + 16), (239, 17), (241, 33), (253, 40), (130, 57),
             (rng.integers(16, 300), rng.integers(16, 120)), (rng.integers(16, 300), rng.integers(16, 120))]
    for (w, h) in sizes:
        w, h = int(w), int(h)
        cw, ch = (w + 1) // 2, (h + 1) // 2
        kind = rng.integers(0, 3)
        frames = []
        for t in range(2):
            if kind == 0:
                y = rng.integers(0, 256, (h, w))
            elif kind == 1:   # flat patches: exact zeros in the high-pass bands, low-variance VIF branch
                y = np.repeat(np.repeat(rng.integers(0, 256, (-(-h // 16), -(-w // 16))), 16, 0), 16, 1)[:h, :w] + t
            else:             # ramps
                y = (np.add.outer(np.arange(h) * 2, np.arange(w)) + 7 * t) % 256
            frames.append(np.clip(y, 0, 255).astype(np.uint8))
        refs = [[f, rng.integers(0, 256, (ch, cw), dtype=np.uint8), rng.integers(0, 256, (ch, cw), dtype=np.uint8)] for f in frames]
        diss = [[np.clip(p.astype(np.int16) + rng.integers(-6, 7, p.shape), 0, 255).astype(np.uint8) for p in fr] for fr in refs]
        exp = oracle64.clip_features([r[0] for r in refs], [d[0] for d in diss], 8)
        exp32 = oracle32.clip_features([r[0] for r in refs], [d[0] for d in diss], 8)
        with _engine(w, h, n_planes=3, features=N.FEAT_ALL, max_batch=2) as eng:
            for i in range(2):
                eng.submit(i, refs[i], diss[i])
            rec = eng.collect(0, 2)
        assert np.all(np.isfinite(rec[:, :20])), (w, h, kind)
        rel = np.abs(rec[:, :16] - exp[:, :16]) / np.maximum(np.abs(exp[:, :16]), 1e-9)
        rel32 = np.abs(exp32[:, :16] - exp[:, :16]) / np.maximum(np.abs(exp[:, :16]), 1e-9)
        # tiny planes with hard steps amplify f32 cancellation (sigma = E[x^2] - mu^2 on a few pixels): the bar
        # there is "no worse than a few times libvmaf's own float rounding" (the f32 oracle vs the f64 truth)
        tol = max(REL_TOL, 4.0 * float(rel32.max()))
        print(f"\n{w}x{h} kind {int(kind)}: gpu-vs-f64 {rel.max():.2e}, f32-oracle-vs-f64 {rel32.max():.2e}")
        assert rel.max() < tol, (w, h, int(kind), float(rel.max()), float(rel32.max()), np.unravel_index(rel.argmax(), rel.shape))
        # what the relative bar means in VMAF points, stated as an ABSOLUTE bound per frame size (DESIGN.md section 1:
        # a decision taken at a 1e-7 margin flips in any f32 evaluation order, and one flipped coefficient weighs
        # 1 / (number of coefficients)): 0.01 from 500 k pixels up (north_star's target, asserted at 1080p / 2160p in
        # test_gpu_engine.py / test_gpu_configs.py), 0.05 from 20 k pixels, 0.25 below that
        full64 = np.zeros((2, 24)); full64[:, :17] = exp
        v_gpu = M_.score_frames(mdl_, M_.metrics_from_records(rec, w, h, "integer_"))["vmaf"]
        v_f64 = M_.score_frames(mdl_, M_.metrics_from_records(full64, w, h, "integer_"))["vmaf"]
        dv = float(np.abs(v_gpu - v_f64).max())
        bound = 0.01 if w * h >= 500_000 else (0.05 if w * h >= 20_000 else 0.25)
        print(f"   |dVMAF| {dv:.4f} (bound {bound} at {w * h} pixels)")
        assert dv <= bound, (w, h, int(kind), dv)
        assert abs(rec[1, 16] - exp[1, 16]) < MOTION_ATOL + 5e-6 * exp[1, 16]
        sse = sse_from_records(rec)
        for p in range(3):
            assert int(sse[1, p]) == oracle32.sse_plane(diss[1][p], refs[1][p], 8)
            assert abs(rec[1, 17 + p] - oracle32.ssim_plane(diss[1][p], refs[1][p], 8)) < 1e-9


def test_fixed_point_random_geometry_sweep():
    """The fixed-point kernels over odd / tiny / non-tile-multiple geometries and hard content (noise, flat
    patches with exact zeros, ramps, saturated extremes): every feature double bit-equal to the restatement."""
    from oracle.int_oracle import IntOracle
    from pqa2_amd import _native as N
    into = IntOracle()
    rng = np.random.default_rng(20250419)
    sizes = [(16, 16), (17, 31), (61, 29), (63, 63), (121, 31), (239, 17), (241, 33), (253, 40), (130, 57), (484, 30),
             (rng.integers(16, 300), rng.integers(16, 120)), (rng.integers(16, 300), rng.integers(16, 120))]
    for n_case, (w, h) in enumerate(sizes):
        w, h = int(w), int(h)
        kind = n_case % 4
        bpc = 10 if n_case % 5 == 4 else 8
        peak = (1 << bpc) - 1
        frames = []
        for t in range(2):
            if kind == 0:
                y = rng.integers(0, peak + 1, (h, w))
            elif kind == 1:
                y = np.repeat(np.repeat(rng.integers(0, peak + 1, (-(-h // 16), -(-w // 16))), 16, 0), 16, 1)[:h, :w] + t
            elif kind == 2:
                y = (np.add.outer(np.arange(h) * 2, np.arange(w)) + 7 * t) % (peak + 1)
            else:             # extremes: checkerboard of 0 / peak, the largest coefficients the Q formats must hold
                y = ((np.add.outer(np.arange(h), np.arange(w)) + t) % 2) * peak
            frames.append(np.clip(y, 0, peak).astype(np.uint8 if bpc == 8 else np.uint16))
        dis = [np.clip(f.astype(np.int32) + rng.integers(-6, 7, f.shape), 0, peak).astype(f.dtype) for f in frames]
        want = np.zeros((2, 17))
        for i in range(2):
            want[i, 0:8] = into.vif(frames[i], dis[i], bpc)
            want[i, 8:16] = into.adm(frames[i], dis[i], bpc)
        b0, b1 = into.motion_blur(frames[0], bpc), into.motion_blur(frames[1], bpc)
        want[1, 16] = into.motion_score(into.motion_sad(b0, b1), w, h)
        with _engine(w, h, bit_depth=bpc, fixed_point=N.FIXED_ALL, max_batch=2) as eng:
            for i in range(2):
                eng.submit(i, [frames[i]], [dis[i]])
            got = eng.collect(0, 2)[:, :17]
        bad = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
        assert bad.size == 0, (w, h, kind, bpc, bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def test_against_committed_golden_fixtures():
    """The HIP path against tests/golden/ (no oracle at run time): f32 kernels within the stated tolerances of the
    f64 fixture, PSNR SSE exact, SSIM 1e-9, VMAF 0.01; the fixed-point kernels bit-equal to the fixed-point fixture."""
    import json
    import os
    from pqa2_amd import _native as N
    from pqa2_amd import model as M
    from pqa2_amd.engine import sse_from_records
    gold_dir = os.path.join(os.path.dirname(__file__), "golden")
    with open(os.path.join(gold_dir, "golden_features.json")) as f:
        g = json.load(f)["cases"]["c64x48_8"]
    z = np.load(os.path.join(gold_dir, "c64x48_8_frames.npz"))
    n, w, h = g["n"], g["w"], g["h"]
    refs = [[z[f"ref{i}_{p}"] for p in range(3)] for i in range(n)]
    diss = [[z[f"dis{i}_{p}"] for p in range(3)] for i in range(n)]
    with _engine(w, h, n_planes=3, features=N.FEAT_ALL) as eng:
        for i in range(n):
            eng.submit(i, refs[i], diss[i])
        rec = eng.collect(0, n)
    want = np.array(g["records"])
    rel = np.abs(rec[:, :16] - want[:, :16]) / np.maximum(np.abs(want[:, :16]), 1e-12)
    assert rel.max() < REL_TOL and np.abs(rec[:, 16] - want[:, 16]).max() < MOTION_ATOL
    assert sse_from_records(rec).tolist() == g["sse"]
    assert np.abs(rec[:, N.REC_SSIM:N.REC_SSIM + 3] - np.array(g["ssim"])).max() < 1e-9
    vm = M.score_frames(M.load_model("vmaf_v0.6.1"), M.metrics_from_records(rec, w, h, "integer_"))["vmaf"]
    assert np.abs(vm - np.array(g["vmaf_v0.6.1"])).max() < 0.01
    with _engine(w, h, fixed_point=N.FIXED_ALL) as eng:
        for i in range(n):
            eng.submit(i, refs[i][:1], diss[i][:1])
        fx = eng.collect(0, n)[:, :17]
    assert np.array_equal(fx, np.array(g["records_fixed_point"]))
