"""The pixel-format converter on the MI355X (csrc/format_convert.hip, pqa_format_convert / pqa_format_convert_device) against
the numpy restatement tests/format_convert_ref.py: equality, no tolerance, everywhere.  Content is uniform noise over the full
sample range with a 0, a maximum and, in a u16 container, one value above the maximum.  The rows kernels (the fast paths) take a
plane only when both sides' bases and pitches are multiples of 16 -- the host entry's staging always is, a device clip when the
test makes it so -- and each such result is also held against PQA_CONVERT_GENERIC on the same input.  A lane of the rows
kernels owns 16 bytes of a row and a workgroup 64 lanes, so the widths below end inside a span (1, 17, 31, 33), fill spans
exactly (16) and pass 64 x 16 bytes (1025); heights 1 ... 37 cover rows where every tap clamps, odd heights and several runs.
On the parent commit there is no FeatureEngine.format_convert and score_files(chroma_mismatch="convert") raises ValueError."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import format_convert_ref as FR

pytestmark = pytest.mark.gpu

DEPTHS = (8, 10, 12)
LAYOUTS = list(itertools.product((0, 1, 2), (0, 1, 2)))     # (hshift, vshift)


def _engine(**kw):
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    return FeatureEngine(64, 48, bit_depth=kw.pop("bit_depth", 8), n_planes=1, features=kw.pop("features", N.FEAT_PSNR), **kw)


@pytest.fixture(scope="module")
def eng():
    with _engine() as e:   # the context's own size and depth do not matter
        yield e


def _dt(bits):
    return np.uint8 if bits == 8 else np.uint16


def _shape(luma_shape, lay):
    return FR.plane_size(luma_shape[0], lay[1]), FR.plane_size(luma_shape[1], lay[0])


def _noise(seed, luma_shape, lay, n=2):
    """n planes of the layout `lay`: noise with the extremes and (u16) one container value above the depth's maximum"""
    rng = np.random.default_rng(seed)
    bits, shape = lay[4], _shape(luma_shape, lay)
    out = []
    for f in range(n):
        p = rng.integers(0, 1 << bits, shape).astype(_dt(bits))
        flat = p.reshape(-1)
        flat[f % flat.size] = 0
        flat[-1 - (f % flat.size)] = (1 << bits) - 1
        if bits > 8 and flat.size > 2:
            flat[flat.size // 2] = 0xFFFF if f % 2 == 0 else (1 << bits)
        out.append(p)
    return out


def _want(planes, luma_shape, src, dst):
    return [FR.convert(p, luma_shape, src, dst) for p in planes]


def _check(eng, planes, luma_shape, src, dst, both=True):
    """the host entry (aligned staging: the fast path where there is one) and the general kernel against the restatement"""
    want = _want(planes, luma_shape, src, dst)
    for generic in ((False, True) if both else (True,)):
        got = eng.format_convert(planes, luma_shape, src, dst, generic=generic)
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (luma_shape, src, dst, generic)


@pytest.mark.parametrize("src_lay", LAYOUTS)
def test_every_layout_pair_on_the_general_path(eng, src_lay):
    """81 layout pairs x the four same-choice-on-both-axes siting pairs, luma 13 x 11, 8 -> 8 bit"""
    luma = (11, 13)
    for dst_lay, ssite, dsite in itertools.product(LAYOUTS, (0, 1), (0, 1)):
        src, dst = (*src_lay, ssite, ssite, 8), (*dst_lay, dsite, dsite, 8)
        _check(eng, _noise(hash((src_lay, dst_lay, ssite, dsite)) & 0xFFFF, luma, src), luma, src, dst, both=False)


@pytest.mark.parametrize("a,b", [((1, 1), (1, 0)), ((1, 0), (0, 0)), ((1, 1), (0, 0))])
def test_all_sixteen_sitings_of_the_common_pairs(eng, a, b):
    luma = (11, 13)
    for (s_lay, d_lay), sites in itertools.product(((a, b), (b, a)), itertools.product((0, 1), repeat=4)):
        src, dst = (*s_lay, sites[0], sites[1], 8), (*d_lay, sites[2], sites[3], 8)
        _check(eng, _noise(sum(sites) + 16 * s_lay[1], luma, src), luma, src, dst)


FAST1_SIZES = [(2, 1), (2, 2), (34, 3), (62, 5), (66, 7), (2050, 37)]      # luma w x h


@pytest.mark.parametrize("w,h", FAST1_SIZES)
@pytest.mark.parametrize("down", [True, False])
def test_fast_path_vertical_two_to_one(eng, w, h, down):
    """4:2:2 <-> 4:2:0 (and 1 <-> 2 vertically), both vertical sitings, 8 and 10 bit"""
    luma = (h, w)
    for (lo, hi), vsite, (sb, db) in itertools.product((((1, 0), (1, 1)), ((1, 1), (1, 2))), (0, 1), ((8, 8), (10, 10), (10, 8))):
        s_lay, d_lay = (lo, hi) if down else (hi, lo)
        src, dst = (*s_lay, 0, vsite, sb), (*d_lay, 0, vsite, db)
        _check(eng, _noise(w + h + vsite, luma, src), luma, src, dst)
    # mixed vertical siting, and a horizontal siting that is the same on both sides
    src, dst = ((1, 0, 1, 0, 8), (1, 1, 1, 1, 8)) if down else ((1, 1, 1, 1, 8), (1, 0, 1, 0, 8))
    _check(eng, _noise(w * h, luma, src), luma, src, dst)


@pytest.mark.parametrize("w", [1, 15, 16, 17, 1025])
def test_fast_path_depth_only(eng, w):
    luma = (3, w)
    for sb, db in itertools.product(DEPTHS, DEPTHS):
        src, dst = (0, 0, 0, 0, sb), (0, 0, 1, 1, db)
        _check(eng, _noise(w + sb + db, luma, src), luma, src, dst)


@pytest.mark.parametrize("sb,db", list(itertools.product(DEPTHS, DEPTHS)))
def test_every_depth_pair(eng, sb, db):
    """fast path 1 both ways, fast path 2 on a chroma plane, and one general layout (4:4:4 -> 4:2:0 centred)"""
    luma = (7, 66)
    for s_lay, d_lay in (((1, 0, 0, 0), (1, 1, 0, 1)), ((1, 1, 0, 1), (1, 0, 0, 0)), ((1, 1, 0, 1), (1, 1, 0, 1)), ((0, 0, 0, 0), (1, 1, 1, 1))):
        src, dst = (*s_lay, sb), (*d_lay, db)
        _check(eng, _noise(sb * 16 + db, luma, src), luma, src, dst)
    top = np.full((7, 66), (1 << sb) - 1, _dt(sb))           # the maximum: c << d when widening, else the maximum (1023 -> 255)
    want = ((1 << sb) - 1) << (db - sb) if db >= sb else (1 << db) - 1
    assert (eng.format_convert([top], luma, (0, 0, 0, 0, sb), (0, 0, 0, 0, db))[0] == want).all()


def _device_convert(eng, planes, luma_shape, src, dst, spad, dpad, lead, generic=False):
    """through pqa_format_convert_device: rows `pad` bytes longer than a row (0: pitches rounded up to 16 and then 16 more),
    bases `lead` samples in; a spare row between the frames.  Returns the planes; every destination byte outside the rows'
    samples must have kept its canary."""
    import torch
    ses, des = np.dtype(_dt(src[4])).itemsize, np.dtype(_dt(dst[4])).itemsize
    n, (sh, sw), (dh, dw) = len(planes), planes[0].shape, _shape(luma_shape, dst)
    spitch = sw * ses + spad if spad else -(-sw * ses // 16) * 16 + 16
    dpitch = dw * des + dpad if dpad else -(-dw * des // 16) * 16 + 16
    sfp, dfp = (sh + 1) * spitch, (dh + 1) * dpitch
    sbuf = np.full(lead * ses + n * sfp, 0x5C, np.uint8)
    for f, p in enumerate(planes):
        rows = sbuf[lead * ses + f * sfp:lead * ses + f * sfp + sh * spitch].reshape(sh, spitch)
        rows[:, :sw * ses] = np.ascontiguousarray(p).view(np.uint8).reshape(sh, sw * ses)
    ts = torch.from_numpy(sbuf).cuda()
    td = torch.full((lead * des + n * dfp,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    eng.format_convert_resident(luma_shape, src, dst, ts.data_ptr() + lead * ses, spitch, sfp, td.data_ptr() + lead * des, dpitch, dfp, n,
                                generic=generic)
    raw = td.cpu().numpy()
    assert (raw[:lead * des] == 0xA5).all()
    out = raw[lead * des:].reshape(n, dh + 1, dpitch)
    assert (out[:, :dh, dw * des:] == 0xA5).all() and (out[:, dh:, :] == 0xA5).all(), (luma_shape, src, dst, spad, dpad, lead)
    return [np.ascontiguousarray(out[f, :dh, :dw * des]).view(_dt(dst[4])).reshape(dh, dw) for f in range(n)]


CASES = [((1, 0, 0, 0), (1, 1, 0, 1)), ((1, 1, 0, 1), (1, 0, 0, 0)), ((0, 0, 0, 0), (0, 0, 0, 0)), ((0, 0, 0, 0), (1, 1, 1, 1))]


@pytest.mark.parametrize("sb,db", [(8, 8), (8, 10), (10, 8), (12, 12)])
def test_device_entry_aligned_and_unaligned(eng, sb, db):
    """aligned clips (the rows kernels) equal the host entry and the general kernel; an odd base and row pitches of a row + 1
    and + 17 bytes (u16: + 2, + 18) on both sides give the same integers, and the canaries between the destination's rows
    and behind its last row are intact"""
    luma = (9, 70)
    for s_lay, d_lay in CASES:
        src, dst = (*s_lay, sb), (*d_lay, db)
        planes = _noise(sb + db, luma, src, n=3)
        want = _want(planes, luma, src, dst)
        host = eng.format_convert(planes, luma, src, dst)
        ses, des = (1 if sb == 8 else 2), (1 if db == 8 else 2)
        for spad, dpad, lead, generic in ((0, 0, 0, False), (0, 0, 0, True), (ses, des, 1, False), (17 * ses if ses == 1 else 18, 17 if des == 1 else 18, 1, False),
                                          (ses, 0, 0, False), (0, des, 1, False)):
            got = _device_convert(eng, planes, luma, src, dst, spad, dpad, lead, generic)
            for g, w, hst in zip(got, want, host):
                assert np.array_equal(g, w) and np.array_equal(g, hst), (src, dst, spad, dpad, lead, generic)


def test_frame_counts(eng):
    """17 frames cross the host entry's chunk of 8 twice; no frames is no work"""
    luma, src, dst = (10, 36), (1, 0, 0, 0, 8), (1, 1, 0, 1, 8)
    planes = _noise(3, luma, src, n=17)
    assert len({p.tobytes() for p in planes}) == 17
    got = eng.format_convert(planes, luma, src, dst)
    assert len(got) == 17 and all(np.array_equal(g, w) for g, w in zip(got, _want(planes, luma, src, dst)))
    assert eng.format_convert([], luma, src, dst) == []
    eng.format_convert_resident(luma, src, dst, 0, 18, 180, 0, 18, 90, 0)
    # frames that are views with a common stride that is no multiple of 16
    buf = np.zeros((17, 10, 23), np.uint8)
    buf[:, :, 2:20] = np.stack(planes)
    got = eng.format_convert([buf[f, :, 2:20] for f in range(17)], luma, src, dst)
    assert all(np.array_equal(g, w) for g, w in zip(got, _want(planes, luma, src, dst)))


def test_argument_rules(eng):
    import torch
    from pqa2_amd import _native as N
    luma, src, dst = (10, 36), (1, 0, 0, 0, 10), (1, 1, 0, 1, 8)       # source rows: 18 samples = 36 bytes; destination: 18 bytes
    buf = torch.zeros(1 << 14, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    q = p + 8192

    def spec(**kw):
        sp = eng._convert_spec(luma, src, dst, False)
        for k, v in kw.items():
            setattr(sp, k, v)
        return sp

    def refused(rc_call, word):
        with pytest.raises(N.PqaError) as e:
            eng._check(rc_call())
        assert e.value.code == N.PQA_EINVAL and word in str(e.value), str(e.value)

    dev = lambda sp, s=p, srp=36, sfp=360, d=q, drp=18, dfp=90, n=1: (
        lambda: eng.lib.pqa_format_convert_device(eng._ctx, C.byref(sp) if sp is not None else None, s or None, srp, sfp, d or None, drp, dfp, n))
    refused(dev(None), "null spec")
    refused(dev(spec(struct_size=8)), "struct_size")
    refused(dev(spec(flags=2)), "flag")
    refused(dev(spec(flags=0x80000001)), "flag")
    for k in ("src_bits", "dst_bits"):
        for v in (0, 9, 16):
            refused(dev(spec(**{k: v})), "depth")
    for k in ("src_hshift", "src_vshift", "dst_hshift", "dst_vshift"):
        refused(dev(spec(**{k: 3})), "shift")
    for k in ("src_hsite", "src_vsite", "dst_hsite", "dst_vsite"):
        refused(dev(spec(**{k: 2})), "siting")
    for k in ("luma_width", "luma_height"):
        for v in (0, 8193):
            refused(dev(spec(**{k: v})), "size")
    refused(dev(spec(), n=-1), "negative")
    refused(dev(spec(), s=0), "null")
    refused(dev(spec(), d=0), "null")
    refused(dev(spec(), srp=34), "source pitch")
    refused(dev(spec(), drp=17), "destination pitch")
    refused(dev(spec(), srp=37), "sample size")
    refused(dev(spec(), sfp=361), "sample size")
    refused(dev(spec(), s=p + 1), "sample size")
    refused(dev(spec(dst_bits=10), d=q + 1, drp=36, dfp=180), "sample size")
    # the host entry: a null list, a null frame, short rows
    a = np.zeros((10, 18), np.uint16)
    o = np.zeros((5, 18), np.uint8)
    sptr, dptr, null = (C.c_void_p * 1)(a.ctypes.data), (C.c_void_p * 1)(o.ctypes.data), (C.c_void_p * 1)(None)
    host = lambda sp, s=sptr, ss=36, d=dptr, ds=18, n=1: (lambda: eng.lib.pqa_format_convert(eng._ctx, C.byref(sp), s, ss, d, ds, n))
    refused(host(spec(), s=None), "null")
    refused(host(spec(), d=None), "null")
    refused(host(spec(), s=null), "null")
    refused(host(spec(), d=null), "null")
    refused(host(spec(), ss=35), "stride")
    refused(host(spec(), ds=17), "stride")
    refused(host(spec(), n=-2), "negative")
    refused(host(spec(luma_width=0)), "size")
    # nothing was written, and both entries work afterwards
    assert not o.any() and not buf.cpu().numpy().any()
    assert eng.lib.pqa_format_convert_device(eng._ctx, C.byref(spec()), None, 36, 360, None, 18, 90, 0) == 0
    a[:] = 1023
    eng._check(host(spec())())
    assert (o == 255).all()
    eng._check(dev(spec())())
    with pytest.raises(ValueError):
        eng.format_convert([a[:3]], luma, src, dst)


def test_independent_of_the_scoring_chain():
    from pqa2_amd import _native as N
    rng = np.random.default_rng(7)
    ref = [rng.integers(0, 256, (48, 64)).astype(np.uint8) for _ in range(6)]
    dis = [np.clip(r.astype(int) + rng.integers(-9, 10, r.shape), 0, 255).astype(np.uint8) for r in ref]
    luma, src, dst = (37, 130), (1, 0, 0, 0, 10), (1, 1, 0, 1, 8)
    planes = _noise(11, luma, src, n=3)

    def run(with_call):
        with _engine(features=N.FEAT_VMAF | N.FEAT_PSNR | N.FEAT_SSIM, max_batch=4) as e:
            outs = []
            for i in range(6):
                e.submit(i, [ref[i]], [dis[i]])
                if with_call and i in (0, 2, 4):    # inside a pending batch, and right after one was launched
                    outs.append(e.format_convert(planes, luma, src, dst))
                    outs.append(e.format_convert(planes, luma, src, dst, generic=True))
            return e.collect(0, 6), outs
    plain, _ = run(False)
    mixed, outs = run(True)
    assert np.array_equal(plain.view(np.uint64), mixed.view(np.uint64))
    want = _want(planes, luma, src, dst)
    assert len(outs) == 6 and all(np.array_equal(g, w) for o in outs for g, w in zip(o, want))


# ---- end to end -----------------------------------------------------------------------------------------------------------
def _same(a, b, where=""):
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), (where, list(a), list(b))
        for k in a:
            _same(a[k], b[k], f"{where}/{k}")
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), where
    else:
        assert a == b, where


@pytest.mark.parametrize("kind", ["422.y4m", ".uyvy", ".v210"])
def test_score_files_converts_a_capture_to_the_master(tmp_path, kind):
    """64 x 48, 6 frames, PSNR | SSIM | CIEDE: the capture scored with chroma_mismatch="convert" equals, record for record and
    key for key, the same clip converted beforehand by the restatement and written as a 4:2:0 8-bit Y4M"""
    from pqa2_amd import synth, yuvio
    from pqa2_amd.pipeline import score_files
    from tests import packed_ref as PR
    w, h, n = 64, 48, 6
    refs, diss = synth.make_clip(w, h, n, 8, chroma=True)
    master = yuvio.VideoInfo(w, h, 8, 1, 1, False, 30, 1, 0, "420mpeg2")
    ref = str(tmp_path / "ref.y4m")
    yuvio.write_y4m(ref, refs, master)
    rng = np.random.default_rng(9)
    bits = 10 if kind == ".v210" else 8
    cap_frames = []
    for f in diss:   # 4:2:2 chroma with detail of its own between the 4:2:0 rows; 10 bit: low bits that the rounding must weigh
        planes = [f[0]] + [np.clip(np.repeat(p, 2, axis=0)[:h].astype(np.int64) + rng.integers(-4, 5, (h, p.shape[1])), 0, 255) for p in f[1:]]
        if bits == 10:
            planes = [np.clip(p.astype(np.int64) * 4 + rng.integers(0, 4, p.shape), 0, 1023) for p in planes]
        cap_frames.append([p.astype(_dt(bits)) for p in planes])
    if kind == "422.y4m":
        cap = str(tmp_path / "cap_422.y4m")
        yuvio.write_y4m(cap, cap_frames, yuvio.VideoInfo(w, h, 8, 1, 0, False, 30, 1, 0, "422"))
        pix = "yuv422p"
    else:
        fmt = {".uyvy": "uyvy422", ".v210": "v210"}[kind]
        cap = str(tmp_path / f"cap_{w}x{h}{kind}")
        with open(cap, "wb") as fh:
            for i, (y, u, v) in enumerate(cap_frames):
                fh.write(PR.pack(fmt, y, u, v, stride=PR.file_stride(fmt, w), seed=i).tobytes())
        pix = fmt
    with pytest.raises(ValueError, match="differ in pixel format"):
        score_files(ref, cap, psnr=True, ssim=True, ciede=True)
    got = score_files(ref, cap, psnr=True, ssim=True, ciede=True, chroma_mismatch="convert")
    src, dst = (1, 0, 0, 0, bits), (1, 1, 0, 1, 8)
    pre = str(tmp_path / "pre.y4m")
    yuvio.write_y4m(pre, [FR.convert_frame(f, src, dst, (h, w)) for f in cap_frames], master)
    want = score_files(ref, pre, psnr=True, ssim=True, ciede=True)
    skip = {"input", "fps", "info"}
    assert [k for k in got if k not in skip] == [k for k in want if k not in skip]
    for k in want:
        if k not in skip:
            _same(got[k], want[k], k)
    assert {"psnr_cb", "psnr_cr", "ciede2000", "vmaf"} <= set(got["metrics"])      # the chroma PSNR columns are psnr_cb / psnr_cr here
    assert got["input"] == {"reference": "yuv420p", "distorted": pix, "planes_scored": "yuv", "packed_upload": False,
                            "conversion": {"side": "distorted", "from": pix, "to": "yuv420p", "bit_depth": [bits, 8],
                                           "siting": {"from": [0, 0], "to": [0, 1]}}}
    assert "input" not in want
