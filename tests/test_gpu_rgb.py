"""Packed RGB captures on the MI355X (csrc/rgb_convert.hip, pqa_rgb_convert / pqa_rgb_convert_device) against the numpy
restatement tests/rgb_ref.py: equality, no tolerance, everywhere.  The rows kernels (the fast paths: luma only, 4:4:4, 4:2:2
co-sited, 4:2:0 left) take a call only when every base and pitch is a multiple of 16 -- the host entry's staging always is, a
device clip when the test makes it so -- and each such result is also held against PQA_RGB_GENERIC on the same input.  A lane of
the rows kernels owns 16 pixels and a workgroup 64 lanes by 4 units, so the sizes end inside a span (1, 2, 17, 19, 33, 66, 130,
642), fill spans exactly (16, 1920) and pass a workgroup both ways (1920 x 1080).  On the parent commit there is no
FeatureEngine.rgb_convert, no pqa2_amd.rgb, and score_files sends a .bgra file to ffmpeg."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import format_convert_ref as FR
from tests import rgb_ref as R

pytestmark = pytest.mark.gpu

COS, CEN = FR.COSITED, FR.CENTRE
# (hshift, vshift, hsite, vsite): 4:4:4; 4:2:2 co-sited, centred; 4:2:0 left, centre, topleft; 4:4:0
LAYOUTS = {"444": (0, 0, 0, 0), "422": (1, 0, COS, 0), "422c": (1, 0, CEN, 0), "420left": (1, 1, COS, CEN), "420centre": (1, 1, CEN, CEN),
           "420topleft": (1, 1, COS, COS), "440": (0, 1, 0, CEN)}
FAST = {"444", "422", "420left"}
SIZES = [(1, 1), (2, 3), (16, 16), (17, 5), (19, 17), (33, 4), (66, 6), (130, 9), (642, 362), (1920, 1080)]


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


def _matrix(std, fmt, db):
    """the named matrix a capture of this format would get: full-range RGB at 8 bit, limited in r210; limited Y'CbCr"""
    from pqa2_amd import rgb
    sb = R.BIT_DEPTH[fmt]
    return rgb.conversion_matrix(std, sb, sb == 8, db, False)


def _frames(seed, fmt, w, h, n=2, stride=None, ones=False):
    """n packed frames of random RGB over the full range with a 0 and a maximum in every component"""
    rng = np.random.default_rng(seed)
    top = (1 << R.BIT_DEPTH[fmt]) - 1
    out = []
    for f in range(n):
        rgb = rng.integers(0, top + 1, (3, h, w))
        rgb[:, 0, 0] = 0 if f % 2 == 0 else top
        rgb[:, -1, -1] = top if f % 2 == 0 else 0
        out.append(R.pack(fmt, rgb[0], rgb[1], rgb[2], stride=stride, seed=seed * 16 + f, ones=ones))
    return out


def _same(got, want, what):
    assert len(got) == len(want), what
    for g, w in zip(got, want):
        assert len(g) == len(w), what
        for p, (a, b) in enumerate(zip(g, w)):
            assert a.dtype == b.dtype and a.shape == b.shape, (what, p, a.dtype, b.dtype, a.shape, b.shape)
            assert np.array_equal(a, b), (what, "plane", p, "first difference at", np.argwhere(a != b)[0].tolist())


def _device(eng, fmt, frames, w, h, dst, m, aligned, luma_only=False, generic=False):
    """through pqa_rgb_convert_device.  aligned: pitches rounded up to 16 and then 16 more (the 16-byte path); otherwise rows
    padded by an odd number of samples on both sides.  A spare row between the frames; the source allocation ends at the last
    used byte of the last row; every destination byte outside the rows' samples must have kept its sentinel."""
    import torch
    n, es = len(frames), np.dtype(_dt(dst[4])).itemsize
    ch, cw = FR.plane_size(h, dst[1]), FR.plane_size(w, dst[0])
    spitch = -(-4 * w // 16) * 16 + 16 if aligned else 4 * w + (12 if fmt == "r210" else 5)
    sfp = (h + 1) * spitch
    sbuf = np.full((n - 1) * sfp + (h - 1) * spitch + 4 * w, 0x5C, np.uint8)
    for f, fr in enumerate(frames):
        for y in range(h):
            sbuf[f * sfp + y * spitch:f * sfp + y * spitch + 4 * w] = fr[y, :4 * w]
    ts = torch.from_numpy(sbuf).cuda()
    shapes = [(h, w)] if luma_only else [(h, w), (ch, cw), (ch, cw)]
    pitch = [(-(-pw * es // 16) * 16 + 16) if aligned else (pw + 3) * es for _, pw in shapes]
    fp = [(ph + 1) * p for (ph, _), p in zip(shapes, pitch)]
    td = [torch.full((n * q,), 0xA5, dtype=torch.uint8, device="cuda") for q in fp]
    torch.cuda.synchronize()
    eng.rgb_convert_resident(fmt, (h, w), dst, m, ts.data_ptr(), spitch, sfp, n, [t.data_ptr() for t in td], pitch + [0] * (3 - len(pitch)),
                             fp + [0] * (3 - len(fp)), generic=generic)
    out = [[] for _ in range(n)]
    for (ph, pw), p, t in zip(shapes, pitch, td):
        raw = t.cpu().numpy().reshape(n, ph + 1, p)
        assert (raw[:, :ph, pw * es:] == 0xA5).all() and (raw[:, ph:, :] == 0xA5).all(), (fmt, w, h, dst, aligned, "sentinel")
        for f in range(n):
            out[f].append(np.ascontiguousarray(raw[f, :ph, :pw * es]).view(_dt(dst[4])).reshape(ph, pw))
    return out


def _combos(w, h):
    """(format, layout name, dst_bits, standard): every combination on the small sizes; on 642 x 362 every format with every layout,
    depth and matrix alternating; on 1920 x 1080 the three fast layouts, one format each"""
    if w * h > 1_000_000:
        return [("bgra", "420left", 8, "bt709"), ("r210", "422", 10, "bt709"), ("argb", "444", 8, "bt601")]
    full = list(itertools.product(R.FORMATS, LAYOUTS, (8, 10), ("bt709", "bt601")))
    if w * h > 10_000:
        return [(f, lay, (8, 10)[(i + j) % 2], ("bt709", "bt601")[(i + j // 2) % 2]) for i, f in enumerate(R.FORMATS) for j, lay in enumerate(LAYOUTS)]
    return full


@pytest.mark.parametrize("w,h", SIZES)
def test_kernel_against_the_restatement(eng, w, h):
    n = 1 if w * h > 1_000_000 else 2
    big = w * h > 10_000
    for k, (fmt, lay, db, std) in enumerate(_combos(w, h)):
        dst, m = (*LAYOUTS[lay], db), _matrix(std, fmt, db)
        frames = _frames(w * 31 + h + k, fmt, w, h, n=n, stride=R.file_stride(fmt, w))
        want = [R.convert(fr, fmt, w, h, m, dst) for fr in frames]
        what = (fmt, lay, db, std, w, h)
        _same(eng.rgb_convert(frames, fmt, (h, w), dst, m), want, what + ("host",))          # file strides, aligned staging
        _same(_device(eng, fmt, frames, w, h, dst, m, aligned=True), want, what + ("device aligned",))
        _same(_device(eng, fmt, frames, w, h, dst, m, aligned=False), want, what + ("device odd pitches",))
        if lay in FAST:
            _same(_device(eng, fmt, frames, w, h, dst, m, aligned=True, generic=True), want, what + ("generic",))
        if not big or lay == "420left":
            luma = [[p[0]] for p in want]
            _same(eng.rgb_convert(frames, fmt, (h, w), dst, m, luma_only=True), luma, what + ("host luma only",))
            _same(_device(eng, fmt, frames, w, h, dst, m, aligned=True, luma_only=True), luma, what + ("device luma only",))
            _same(_device(eng, fmt, frames, w, h, dst, m, aligned=False, luma_only=True), luma, what + ("device luma only odd",))


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_padding_bits_change_nothing(eng, fmt):
    w, h, dst = 37, 6, (*LAYOUTS["420left"], 8)
    m = _matrix("bt709", fmt, 8)
    rng = np.random.default_rng(5)
    rgb = rng.integers(0, 1 << R.BIT_DEPTH[fmt], (3, h, w))
    a = R.pack(fmt, *rgb, seed=1, ones=False)
    b = R.pack(fmt, *rgb, seed=2, ones=True)
    assert not np.array_equal(a, b)
    for generic in (False, True):
        _same(eng.rgb_convert([a], fmt, (h, w), dst, m, generic=generic), eng.rgb_convert([b], fmt, (h, w), dst, m, generic=generic), (fmt, generic))


def _selection(order=(2, 3, 1)):
    """Y, U, V = G, B, R: 2^14 on one component, offset 0"""
    m = [0] * 12
    for c, k in enumerate(order):
        m[4 * c + k] = 1 << 14
    return m


def _component_planes(fmt, fr, w):
    """G, B, R of packed rows read straight from the bytes (not through rgb_ref.unpack)"""
    px = fr[:, :4 * w].reshape(fr.shape[0], w, 4)
    if fmt == "r210":
        word = px.astype(np.uint32) @ np.array([1 << 24, 1 << 16, 1 << 8, 1], np.uint32)
        return [((word >> s) & 1023).astype(np.uint16) for s in (10, 0, 20)]
    at = {"bgra": (1, 0, 2), "argb": (2, 3, 1), "rgba": (1, 2, 0), "abgr": (2, 1, 3)}[fmt]
    return [np.ascontiguousarray(px[..., k]) for k in at]


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_selection_matrix_and_the_existing_converter(eng, fmt):
    """4:4:4 with a selection matrix: Y, U, V are the packed G, B, R byte for byte.  Every subsampled layout then equals
    pqa_format_convert_device applied to those 4:4:4 planes: the new kernel against the existing one."""
    import torch
    w, h = 70, 9
    sb = R.BIT_DEPTH[fmt]
    frames = _frames(77, fmt, w, h, n=2, stride=R.file_stride(fmt, w))
    m = _selection()
    for generic in (False, True):
        got = eng.rgb_convert(frames, fmt, (h, w), (0, 0, 0, 0, sb), m, generic=generic)
        _same(got, [_component_planes(fmt, fr, w) for fr in frames], (fmt, generic))
    es = np.dtype(_dt(sb)).itemsize
    for lay in LAYOUTS:   # at the source's own depth: a selection matrix carries no depth change, pqa_format_convert would
        db = sb
        dst = (*LAYOUTS[lay], db)
        mine = eng.rgb_convert(frames, fmt, (h, w), dst, m)
        des = np.dtype(_dt(db)).itemsize
        dh, dw = FR.plane_size(h, dst[1]), FR.plane_size(w, dst[0])
        for p in (1, 2):
            src = torch.from_numpy(np.stack([g[p] for g in got]).view(np.uint8).reshape(-1)).cuda()
            out = torch.zeros(2 * dh * dw * des, dtype=torch.uint8, device="cuda")
            eng.format_convert_resident((h, w), (0, 0, 0, 0, sb), dst, src.data_ptr(), w * es, w * h * es, out.data_ptr(), dw * des, dw * dh * des, 2)
            theirs = out.cpu().numpy().view(_dt(db)).reshape(2, dh, dw)
            for f in range(2):
                assert np.array_equal(mine[f][p], theirs[f]), (fmt, lay, db, p, f)


@pytest.mark.parametrize("fmt", ["bgra", "r210"])
def test_clamps(eng, fmt):
    """gain 2 with offsets that drive all-zero frames below 0 and all-maximum frames above the top"""
    w, h, sb = 35, 5, R.BIT_DEPTH[fmt]
    top = (1 << sb) - 1
    for db, lay in itertools.product((8, 10), ("444", "420left", "420centre")):
        dst, dtop = (*LAYOUTS[lay], db), (1 << db) - 1
        # Y and V start below 0; U starts where twice the source maximum passes the top (as high as the int32 bound lets it)
        m = [-(5 << 14), 2 << 14, 0, 0, max(0, dtop - top) << 14, 0, 2 << 14, 0, -(3 << 14) - 1, 0, 0, 2 << 14]
        from pqa2_amd import rgb
        assert rgb.matrix_fits(m, sb, dst[0], dst[1])
        frames = [R.pack(fmt, *np.full((3, h, w), v), seed=v) for v in (0, top)]
        want = [R.convert(fr, fmt, w, h, m, dst) for fr in frames]
        assert (want[0][0] == 0).all() and (want[0][2] == 0).all() and (want[1][1] == dtop).all()
        for generic in (False, True):
            _same(eng.rgb_convert(frames, fmt, (h, w), dst, m, generic=generic), want, (fmt, db, lay, generic))


def test_refused_calls(eng):
    import torch
    from pqa2_amd import _native as N
    from pqa2_amd import rgb
    w, h, dst = 36, 10, (1, 1, COS, CEN, 10)          # source rows 144 bytes; Y rows 72 bytes, chroma rows 36
    m = rgb.conversion_matrix("bt709", 10, False, 10, False)
    buf = torch.full((1 << 15,), 0xA5, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    q = [p + 8192, p + 16384, p + 20480]

    def spec(fmt="r210", **kw):
        sp = eng._rgb_spec(fmt, (h, w), dst, m, False)
        for k, v in kw.items():
            if k == "m":
                for i, x in enumerate(v):
                    sp.m[i] = x
            else:
                setattr(sp, k, v)
        return sp

    def clip(ptrs=q, rp=(72, 36, 36), fpitch=(720, 180, 180)):
        d = N.PqaDeviceClip()
        for i in range(3):
            d.plane[i], d.row_pitch[i], d.frame_pitch[i] = ptrs[i] or None, rp[i], fpitch[i]
        return d

    def refused(rc_call, word):
        with pytest.raises(N.PqaError) as e:
            eng._check(rc_call())
        assert e.value.code == N.PQA_EINVAL and word in str(e.value), str(e.value)

    dev = lambda sp, s=p, srp=144, sfp=1440, n=1, d=None: (
        lambda: eng.lib.pqa_rgb_convert_device(eng._ctx, C.byref(sp) if sp is not None else None, s or None, srp, sfp, n, C.byref(d or clip())))
    refused(dev(None), "null spec")
    refused(dev(spec(struct_size=16)), "struct_size")
    for f in (0, 3, 5, 11):
        refused(dev(spec(format=f)), "not a packed RGB format")
    refused(dev(spec(flags=2)), "flag")
    for b in (0, 9, 12, 16):
        refused(dev(spec(dst_bits=b)), "depth")
    for k in ("hshift", "vshift"):
        refused(dev(spec(**{k: 2})), "shift")
    for k in ("hsite", "vsite"):
        refused(dev(spec(**{k: 2})), "siting")
    for k in ("width", "height"):
        for v in (0, 8193):
            refused(dev(spec(**{k: v})), "size")
    refused(dev(spec(), n=-1), "negative")
    refused(dev(spec(), s=0), "null")
    refused(dev(spec(), srp=143), "source pitch")
    refused(dev(spec(), srp=146), "multiple of 4")
    refused(dev(spec(), sfp=1442), "multiple of 4")
    refused(dev(spec(), s=p + 2), "4-byte aligned")
    refused(dev(spec(), d=clip(ptrs=[q[0] + 1, q[1], q[2]])), "whole samples")
    refused(dev(spec(), d=clip(rp=(72, 37, 36))), "whole samples")
    refused(dev(spec(), d=clip(rp=(70, 36, 36))), "pitch smaller")
    refused(dev(spec(), d=clip(rp=(72, 36, 34))), "pitch smaller")
    refused(dev(spec(), d=clip(ptrs=[0, q[1], q[2]])), "null luma")
    refused(dev(spec(), d=clip(ptrs=[q[0], q[1], 0])), "both or neither")
    refused(dev(spec(), d=clip(ptrs=[q[0], 0, q[2]])), "both or neither")
    refused(dev(spec(m=[4 * v for v in m])), "int32")                       # a named matrix scaled by 4
    refused(dev(spec(m=[0, 1 << 21, 0, 0] + list(m[4:]))), "int32")         # 1023 * 2^21 * 64 reaches 2^37
    # the 8-bit formats take any source pitch from 4 * w on, and the host entry has the same rules
    eng._check(dev(spec("bgra"), srp=145, sfp=1451)())
    a = np.zeros((h, 4 * w), np.uint8)
    o = [np.full((h, w), 0xA5A5, np.uint16), np.full((5, 18), 0xA5A5, np.uint16), np.full((5, 18), 0xA5A5, np.uint16)]
    sptr, null1 = (C.c_void_p * 1)(a.ctypes.data), (C.c_void_p * 1)(None)
    dptr = (C.c_void_p * 3)(*[x.ctypes.data for x in o])
    one = (C.c_void_p * 3)(o[0].ctypes.data, o[1].ctypes.data, None)
    strides = (C.c_int64 * 3)(72, 36, 36)
    host = lambda sp, s=sptr, ss=144, n=1, d=dptr, ds=strides: (lambda: eng.lib.pqa_rgb_convert(eng._ctx, C.byref(sp), s, ss, n, d, C.byref(ds) if ds is not None else None))
    refused(host(spec(), s=None), "null")
    refused(host(spec(), d=None), "null")
    refused(host(spec(), s=null1), "null")
    refused(host(spec(), d=one), "both or neither")
    refused(host(spec(), ds=None), "null destination strides")
    refused(host(spec(), ss=140), "source pitch")
    refused(host(spec(), ss=146), "multiple of 4")
    refused(host(spec(), ds=(C.c_int64 * 3)(72, 34, 36)), "stride smaller")
    refused(host(spec(), ds=(C.c_int64 * 3)(73, 36, 36)), "whole samples")
    refused(host(spec(dst_bits=12)), "depth")
    refused(host(spec(m=[4 * v for v in m])), "int32")
    assert all((x == 0xA5A5).all() for x in o)
    # nothing was written on the device either (the accepted bgra call above wrote the planes' samples only: check the rest)
    raw = buf.cpu().numpy()
    assert (raw[:8192] == 0xA5).all() and (raw[8192 + 720:16384] == 0xA5).all() and (raw[16384 + 180:20480] == 0xA5).all() and (raw[20480 + 180:] == 0xA5).all()
    # no frames is no work; both entries work afterwards
    assert eng.lib.pqa_rgb_convert_device(eng._ctx, C.byref(spec()), None, 144, 1440, 0, C.byref(clip())) == 0
    eng._check(host(spec())())
    _same([o], [R.convert(a, "r210", w, h, m, dst)], "host entry after the refusals")
    # the older entries refuse the new format values as before
    for f in (N.SURFACE_BGRA, N.SURFACE_ARGB, N.SURFACE_RGBA, N.SURFACE_ABGR, N.SURFACE_R210):
        sp = eng._unpack_spec(f, (h, w))
        refused(lambda: eng.lib.pqa_unpack_device(eng._ctx, C.byref(sp), p, 144, 1440, 1, C.byref(clip())), "is not a packed capture format")
        hc = N.PqaHostClip()
        hc.struct_size, hc.format, hc.frames = C.sizeof(N.PqaHostClip), f, C.cast(sptr, C.POINTER(C.c_void_p))
        hc.strides[0] = 256
        refused(lambda: eng.lib.pqa_submit_packed(eng._ctx, 0, 1, C.byref(hc), C.byref(hc)), "is neither planar nor a packed capture format")
    with pytest.raises(ValueError):
        eng.rgb_convert([a], "rgb24", (h, w), dst, m)


# ---- end to end -----------------------------------------------------------------------------------------------------------
def _equal(a, b, where=""):
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), (where, list(a), list(b))
        for k in a:
            _equal(a[k], b[k], f"{where}/{k}")
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), where
    else:
        assert a == b, where


def _to_rgb(planes, bits, limited):
    """a host inverse of BT.601 limited-range Y'CbCr 4:2:0 8 bit: R, G, B code values of `bits` bits (chroma repeated)"""
    y = planes[0].astype(np.float64)
    h, w = y.shape
    cb, cr = (np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)[:h, :w].astype(np.float64) - 128 for p in planes[1:])
    yn = (y - 16) / 219
    r, b = yn + 1.402 * cr / 224, yn + 1.772 * cb / 224
    g = (yn - 0.299 * r - 0.114 * b) / 0.587
    f = 1 << (bits - 8)
    lo, span = (16 * f, 219 * f) if limited else (0, (1 << bits) - 1)
    return [np.clip(np.rint(lo + span * c), 0, (1 << bits) - 1).astype(np.int64) for c in (r, g, b)]


def _clips(tmp_path, fmt, name):
    """the 64 x 48 master as Y4M and its distorted clip as a packed RGB file: (reference path, capture path, packed frames)"""
    from pqa2_amd import synth, yuvio
    w, h, n = 64, 48, 5
    refs, diss = synth.make_clip(w, h, n, 8, chroma=True)
    master = yuvio.VideoInfo(w, h, 8, 1, 1, False, 30, 1, 0, "420mpeg2")
    ref = str(tmp_path / "ref.y4m")
    yuvio.write_y4m(ref, refs, master)
    bits = R.BIT_DEPTH[fmt]
    packed = [R.pack(fmt, *_to_rgb(f, bits, fmt == "r210"), stride=R.file_stride(fmt, w), seed=i) for i, f in enumerate(diss)]
    cap = str(tmp_path / f"{name}_{w}x{h}.{fmt}")
    with open(cap, "wb") as fh:
        for p in packed:
            fh.write(p.tobytes())
    return ref, cap, packed, master, refs


@pytest.mark.parametrize("fmt", ["bgra", "r210"])
def test_score_files_with_a_yuv_master(tmp_path, fmt):
    """the capture scored as it is equals, record for record and key for key, the same file converted beforehand by the
    restatement and written as a 4:2:0 8-bit Y4M"""
    from pqa2_amd import rgb, yuvio
    from pqa2_amd.pipeline import score_files
    w, h = 64, 48
    ref, cap, packed, master, _ = _clips(tmp_path, fmt, "cap")
    got = score_files(ref, cap, psnr=True, ssim=True, ciede=True)
    sb = R.BIT_DEPTH[fmt]
    m = rgb.conversion_matrix("bt601", sb, fmt != "r210", 8, False)          # 48 lines: bt601; the cards' ranges; a limited master
    dst = (1, 1, COS, CEN, 8)
    pre = str(tmp_path / "pre.y4m")
    yuvio.write_y4m(pre, [R.convert(p, fmt, w, h, m, dst) for p in packed], master)
    want = score_files(ref, pre, psnr=True, ssim=True, ciede=True)
    skip = {"input", "fps", "info"}
    assert [k for k in got if k not in skip] == [k for k in want if k not in skip]
    for k in want:
        if k not in skip:
            _equal(got[k], want[k], k)
    assert {"psnr_cb", "psnr_cr", "ciede2000", "vmaf"} <= set(got["metrics"])
    assert got["input"] == {"reference": "yuv420p", "distorted": fmt, "planes_scored": "yuv", "packed_upload": False,
                            "conversion": {"side": "distorted", "from": fmt, "to": "yuv420p", "matrix": "bt601",
                                           "rgb_range": "limited" if fmt == "r210" else "full", "yuv_range": "limited",
                                           "bit_depth": [sb, 8], "siting": {"to": [0, 1]}, "coefficients": m}}
    assert "input" not in want
    # the options reach the conversion; chroma_mismatch does not matter
    other = score_files(ref, cap, psnr=True, ssim=False, rgb_matrix="bt709", rgb_range="limited", chroma_siting="center", chroma_mismatch="luma")
    conv = other["input"]["conversion"]
    assert (conv["matrix"], conv["rgb_range"], conv["siting"]) == ("bt709", "limited", {"to": [1, 1]})
    assert conv["coefficients"] == rgb.conversion_matrix("bt709", sb, False, 8, False) and other["input"]["planes_scored"] == "yuv"


def test_score_files_with_two_rgb_files(tmp_path):
    """two RGB files against each other are scored at 4:4:4, at the reference's depth"""
    from pqa2_amd import rgb, yuvio
    from pqa2_amd.pipeline import score_files
    w, h = 64, 48
    _, cap, packed, _, refs = _clips(tmp_path, "r210", "cap")
    master = str(tmp_path / f"master_{w}x{h}.argb")
    mp = [R.pack("argb", *_to_rgb(f, 8, False), seed=40 + i) for i, f in enumerate(refs)]
    with open(master, "wb") as fh:
        for p in mp:
            fh.write(p.tobytes())
    got = score_files(master, cap, psnr=True, ssim=True)
    info444 = yuvio.VideoInfo(w, h, 8, 0, 0, False, 30, 1, 0, "444")
    dst = (0, 0, 0, 0, 8)
    ma, mb = rgb.conversion_matrix("bt601", 8, True, 8, False), rgb.conversion_matrix("bt601", 10, False, 8, False)
    a, b = str(tmp_path / "a.y4m"), str(tmp_path / "b.y4m")
    yuvio.write_y4m(a, [R.convert(p, "argb", w, h, ma, dst) for p in mp], info444)
    yuvio.write_y4m(b, [R.convert(p, "r210", w, h, mb, dst) for p in packed], info444)
    want = score_files(a, b, psnr=True, ssim=True)
    for k in want["metrics"]:
        assert np.array_equal(got["metrics"][k], want["metrics"][k]), k
    assert list(got["metrics"]) == list(want["metrics"]) and "psnr_cb" in got["metrics"]
    conv = got["input"]["conversion"]
    assert [c["side"] for c in conv] == ["reference", "distorted"] and [c["to"] for c in conv] == ["yuv444p", "yuv444p"]
    assert [c["bit_depth"] for c in conv] == [[8, 8], [10, 8]] and got["input"]["planes_scored"] == "yuv"
