"""The deinterlacer on the MI355X (csrc/deinterlace.hip, pqa_deinterlace / pqa_deinterlace_device): every output plane equals
the numpy restatement (tests/deinterlace_ref.py) bit for bit -- exact integers, no tolerance.  The binding and the argument
rules, the smallest planes, tails and every load width on padded and offset layouts with guard bytes behind every destination
row, the clamp, the seams of the kernel's block with a bright sample at every seam position of P, C and N, the half-static noise
clip with all four branches in one wave and in one 16-byte piece and whole still waves beside it (fast path on and off), the
extreme triples, the launch seam and the window of the host entry, a plane size other than the context's; the calls leave the
scoring chain alone."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import deinterlace_ref as R

pytestmark = pytest.mark.gpu

SETTINGS = [(m, f, r) for m in R.MODES for f in (0, 1) for r in R.RATES]


def _engine(w, h, bpc=8, **kw):
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    return FeatureEngine(w, h, bit_depth=bpc, n_planes=kw.pop("n_planes", 1), features=kw.pop("features", N.FEAT_PSNR), **kw)


def _dt(bpc):
    return np.uint8 if bpc == 8 else np.uint16


def _noise(seed, n, w, h, bpc):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 1 << bpc, (h, w)).astype(_dt(bpc)) for _ in range(n)]


def _same(got, want):
    return len(got) == len(want) and all(g.dtype == w.dtype and np.array_equal(g, w) for g, w in zip(got, want))


def _padded(frames, pad=5, lead=1, fill=0):
    """the same frames as views into one buffer: rows `pad` samples longer than a row, base `lead` samples in"""
    h, w = frames[0].shape
    buf = np.full((len(frames), h, w + pad), fill, frames[0].dtype)
    buf[:, :, lead:lead + w] = np.stack(frames)
    return buf, [buf[i, :, lead:lead + w] for i in range(len(frames))]


GUARD = 0xA5


def _resident(eng, frames, mode, first, rate, src_layout=(0, 0), dst_layout=(0, 0)):
    """(output planes, bytes of one load the launch takes, guard bytes intact) of a clip uploaded on src_layout = (pad, lead) and
    deinterlaced into a destination on dst_layout whose every byte outside the samples holds GUARD"""
    import torch
    h, w = frames[0].shape
    es = frames[0].itemsize
    per = 2 if rate == "field" else 1
    sbuf, _ = _padded(frames, *src_layout)
    dbuf = np.full((len(frames) * per, h, w + dst_layout[0]), GUARD * 0x0101 if es == 2 else GUARD, frames[0].dtype)
    ts = torch.from_numpy(sbuf.view(np.uint8).reshape(-1)).cuda()
    td = torch.from_numpy(dbuf.view(np.uint8).reshape(-1)).cuda()
    torch.cuda.synchronize()
    ps, pd = ts.data_ptr() + src_layout[1] * es, td.data_ptr() + dst_layout[1] * es
    bits = ps | pd | sbuf.strides[1] | sbuf.strides[0] | dbuf.strides[1] | dbuf.strides[0]
    load = 16 if bits % 16 == 0 else 4 if bits % 4 == 0 else es      # load_bytes of plane_scan.h
    eng.deinterlace_resident((h, w), ps, sbuf.strides[1], sbuf.strides[0], pd, dbuf.strides[1], dbuf.strides[0], len(frames), mode, first, rate)
    torch.cuda.synchronize()
    back = td.cpu().numpy().view(frames[0].dtype).reshape(dbuf.shape)
    lead = dst_layout[1]
    guard = np.ones(back.shape, bool)
    guard[:, :, lead:lead + w] = False
    intact = bool((back.view(np.uint8).reshape(back.shape + (es,))[guard] == GUARD).all())
    return [back[i, :, lead:lead + w].copy() for i in range(len(back))], load, intact


def test_the_binding_states_the_kernels_constants():
    import os
    import re
    from pqa2_amd import _native as N
    src = open(os.path.join(os.path.dirname(N.LIB_PATH), "kernels.h")).read()

    def const(name):
        return int(re.search(name + r"\s*=\s*(\d+)", src).group(1))
    lib = N.load()
    assert const("kDeintChunk") == N.DEINT_CHUNK == lib.pqa_deint_chunk() == 8
    assert const("kDeintColBytes") == N.DEINT_BLOCK_BYTES == lib.pqa_deint_block_bytes()
    assert const("kDeintWaves") * const("kDeintBand") == N.DEINT_BLOCK_ROWS == lib.pqa_deint_block_rows() and const("kDeintBand") % 2 == 0
    assert C.sizeof(N.PqaDeintSpec) == 24


@pytest.mark.parametrize("bpc", [8, 10])
def test_argument_rules(bpc):
    from pqa2_amd import _native as N
    src = _noise(bpc, 3, 16, 16, bpc)
    es = src[0].itemsize
    with _engine(64, 48, bpc) as eng:
        want = R.deinterlace(src, "adaptive", 0, "field", bpc)
        assert _same(eng.deinterlace(src, "adaptive", 0, "field"), want)
        lib, ctx = eng.lib, eng._ctx
        keep, sp_, ss = eng._luma_list(src, "source", (16, 16))
        out = [np.zeros((16, 16), _dt(bpc)) for _ in range(6)]
        dp_ = (C.c_void_p * 6)(*[o.ctypes.data for o in out])

        def spec(**kw):
            s = eng._deint_spec((kw.pop("height", 16), kw.pop("width", 16)), "adaptive", 0, "field")
            for k, v in kw.items():
                setattr(s, k, v)
            return C.byref(s)
        null_src = (C.c_void_p * 3)(sp_[0], None, sp_[2])
        null_dst = (C.c_void_p * 6)(dp_[0], dp_[1], dp_[2], dp_[3], dp_[4], None)
        same_dst = (C.c_void_p * 6)(dp_[0], dp_[1], dp_[2], sp_[1], dp_[4], dp_[5])
        dev, dev2 = 4096, 1 << 20      # never dereferenced: every call below is refused before any device call

        def host(s=None, f=sp_, fst=ss, d=dp_, dst=16 * es, n=3):
            return lib.pqa_deinterlace(ctx, spec() if s is None else s, f, fst, d, dst, n)

        def device(s=None, f=dev, rp=16 * es, fp=256 * es, d=dev2, drp=16 * es, dfp=256 * es, n=3):
            return lib.pqa_deinterlace_device(ctx, spec() if s is None else s, f, rp, fp, d, drp, dfp, n)
        calls = {
            "null spec": lambda: lib.pqa_deinterlace(ctx, None, sp_, ss, dp_, 16 * es, 3),
            "null spec, device": lambda: lib.pqa_deinterlace_device(ctx, None, dev, 16 * es, 256 * es, dev2, 16 * es, 256 * es, 3),
            "null source list": lambda: host(f=None),
            "null destination list": lambda: host(d=None),
            "null source frame": lambda: host(f=null_src),
            "null destination frame": lambda: host(d=null_dst),
            "null source clip": lambda: device(f=None),
            "null destination clip": lambda: device(d=None),
            "struct_size": lambda: host(spec(struct_size=12)),
            "struct_size, device": lambda: device(spec(struct_size=28)),
            "height 1": lambda: host(spec(height=1)),
            "height 1, device": lambda: device(spec(height=1)),
            "height 0": lambda: host(spec(height=0)),
            "width 0": lambda: host(spec(width=0)),
            "width 8193": lambda: host(spec(width=8193), fst=8193 * es, dst=8193 * es),
            "height 8193": lambda: device(spec(height=8193)),
            "mode 2": lambda: host(spec(mode=2)),
            "mode 2, device": lambda: device(spec(mode=2)),
            "first 2": lambda: host(spec(first=2)),
            "first 2, device": lambda: device(spec(first=2)),
            "rate 2": lambda: host(spec(rate=2)),
            "rate 2, device": lambda: device(spec(rate=2)),
            "short source stride": lambda: host(fst=16 * es - 1),
            "short destination stride": lambda: host(dst=16 * es - 1),
            "negative source stride": lambda: host(fst=-16 * es),
            "negative destination stride": lambda: host(dst=-16 * es),
            "short source pitch": lambda: device(rp=15 * es),
            "short destination pitch": lambda: device(drp=15 * es),
            "negative pitch": lambda: device(rp=-16 * es),
            "negative frame count": lambda: host(n=-1),
            "negative frame count, device": lambda: device(n=-1),
            "a destination frame that is a source frame": lambda: host(d=same_dst),
            "the destination is the source": lambda: device(d=dev),
        }
        if es == 2:      # a pitch that is no multiple of the sample size
            calls["odd source stride"] = lambda: host(fst=33)
            calls["odd destination stride"] = lambda: host(dst=35)
            calls["odd row pitch"] = lambda: device(rp=33)
            calls["odd frame pitch"] = lambda: device(dfp=513)
            calls["odd base"] = lambda: device(d=dev2 + 1)
        for name, call in calls.items():
            assert call() == N.PQA_EINVAL, name
        assert host(spec(height=1)) == N.PQA_EINVAL and b"height 1" in lib.pqa_last_error(ctx)      # the entry's own rule
        assert not any(o.any() for o in out)
        assert host(n=0) == N.PQA_OK and device(n=0) == N.PQA_OK and not any(o.any() for o in out)
        assert host(f=None, d=None, n=0) == N.PQA_OK and device(f=None, d=None, n=0) == N.PQA_OK
        assert eng.deinterlace([], "adaptive", 0, "field") == []
        assert host() == N.PQA_OK and _same(out, want)      # refused calls leave the context usable
        del keep
        for bad in (dict(mode="bob"), dict(rate="double"), dict(first=2)):
            with pytest.raises(ValueError):
                eng.deinterlace(src, **bad)


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_smallest_planes(bpc):
    with _engine(64, 48, bpc) as eng:
        for (w, h), n in itertools.product(((1, 2), (1, 3), (2, 2), (17, 5), (16, 9)), (1, 2, 3)):
            src = _noise(w * 31 + h + n + bpc, n, w, h, bpc)
            for mode, first, rate in SETTINGS:
                want = R.deinterlace(src, mode, first, rate, bpc)
                assert _same(eng.deinterlace(src, mode, first, rate), want), (w, h, n, mode, first, rate)
                got, _, intact = _resident(eng, src, mode, first, rate)
                assert _same(got, want) and intact, (w, h, n, mode, first, rate, "resident")


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_tails_pitches_and_guard_bytes(bpc):
    """widths around the lanes' 16 bytes and one past the block's columns on 11 rows; a contiguous clip, rows padded to a multiple
    of 16 bytes (16-byte loads), a base 4 samples in with rows 4-byte aligned (4-byte loads), rows padded by 5 samples and a base
    one sample in (sample by sample), and source and destination on different layouts.  `seen` holds the load width that the rule
    of plane_scan.h (load_bytes) gives for the addresses and pitches of each call, computed HERE from a copy of that rule: the
    library has no query for the width it dispatched, so `seen == {16, 4, es}` says that the layouts offered call for all three
    instances, not that the library took them; what is checked against the library is every plane, bit for bit, and the guard
    bytes"""
    from pqa2_amd import _native as N
    es = 1 if bpc == 8 else 2
    seen = set()
    with _engine(64, 48, bpc) as eng:
        for w in (15, 16, 17, 31, 33, 63, 65, N.DEINT_BLOCK_BYTES // es + 1):
            src = _noise(w + bpc, 3, w, 11, bpc)
            a16 = -w % 16 or 16      # rows a multiple of 16 samples: 16-byte loads at either sample size
            a4 = -(w + 4) % 4 + 4
            for k, (mode, first, rate) in enumerate((("adaptive", 0, "field"), ("intra", 1, "frame"), ("adaptive", 1, "frame"))):
                want = R.deinterlace(src, mode, first, rate, bpc)
                assert _same(eng.deinterlace(src, mode, first, rate), want), (w, mode)
                assert _same(eng.deinterlace(_padded(src, 5, 1)[1], mode, first, rate), want), (w, mode, "padded host rows")
                for sl, dl in (((0, 0), (0, 0)), ((a16, 0), (a16, 0)), ((a4, 4), (a4, 4)), ((5, 1), (5, 1)), ((a16, 0), (5, 1)), ((a4, 4), (a16, 0))):
                    got, load, intact = _resident(eng, src, mode, first, rate, sl, dl)
                    assert _same(got, want), (w, mode, first, rate, sl, dl, load)
                    assert intact, (w, mode, sl, dl, "a byte outside the destination's samples was written")
                    seen.add(load)
    assert seen == {16, 4, es}


def test_samples_above_the_maximum_are_clamped():
    rng = np.random.default_rng(5)
    src = [rng.integers(0, 1 << 16, (21, 70)).astype(np.uint16) for _ in range(3)]
    assert (src[0] > 1023).any()
    with _engine(70, 21, 10) as eng:
        for mode, first, rate in SETTINGS:
            want = R.deinterlace([np.minimum(f, 1023) for f in src], mode, first, rate, 10)
            assert _same(R.deinterlace(src, mode, first, rate, 10), want)
            assert _same(eng.deinterlace(src, mode, first, rate), want), (mode, first, rate)


@pytest.mark.parametrize("bpc", [8, 10])
def test_seams_of_the_block(bpc):
    """plane sizes at block - 1, block, block + 1 and 2 block + 1 each way on random planes"""
    from pqa2_amd import _native as N
    bc, br = N.DEINT_BLOCK_BYTES // (1 if bpc == 8 else 2), N.DEINT_BLOCK_ROWS
    with _engine(64, 64, bpc) as eng:
        for w, h in ((bc - 1, br - 1), (bc, br), (bc + 1, br + 1), (2 * bc + 1, 20), (20, 2 * br + 1), (bc + 1, br - 1)):
            src = _noise(w * 7 + h + bpc, 3, w, h, bpc)
            for mode, first, rate in (("adaptive", 0, "field"), ("adaptive", 1, "field"), ("intra", 0, "field")):
                assert _same(eng.deinterlace(src, mode, first, rate), R.deinterlace(src, mode, first, rate, bpc)), (w, h, mode, first)


@pytest.mark.parametrize("bpc", [8, 10])
def test_a_bright_sample_at_every_seam_position(bpc):
    """a clip of 2 band + 3 rows by block + 1 columns with one bright sample at every seam position in turn, in each of P, C and
    N: the spot frames go through the clip one by one (quiet, spot, quiet, quiet, spot, ...), so that every spot is the N, the C
    and the P of three consecutive source frames.  The quiet picture is a smooth ramp, not flat: on a flat clip the temporal clamp
    rejects a lone sample of P or N altogether"""
    from pqa2_amd import _native as N
    es = 1 if bpc == 8 else 2
    bc, band = N.DEINT_BLOCK_BYTES // es, N.DEINT_BLOCK_ROWS // 4
    w, h = bc + 1, 2 * band + 3
    lanes = 16 // es
    xs = sorted({0, lanes - 1, lanes, bc - 1, bc})
    ys = sorted({0, 1, 2, 3, 4, band - 5, band - 4, band - 3, band - 2, band - 1, band, band + 1, band + 2, band + 3, band + 4,
                 2 * band - 1, 2 * band, 2 * band + 1, 2 * band + 2})
    top = (1 << bpc) - 1
    y, x = np.mgrid[0:h, 0:w]
    quiet = ((3 * y + x) % (top // 2)).astype(_dt(bpc))
    frames = [quiet]
    for sy in ys:
        f = quiet.copy()
        for sx in xs:      # one row's spots share a frame: they are more than a piece apart or in different columns anyway
            f[sy, sx] = top
        frames += [f, quiet, quiet]
    with _engine(w, h, bpc) as eng:
        for first in (0, 1):
            want = R.deinterlace(frames, "adaptive", first, "field", bpc)
            got = eng.deinterlace(frames, "adaptive", first, "field")
            for k, (g, v) in enumerate(zip(got, want)):
                assert np.array_equal(g, v), (first, k, np.argwhere(g != v)[:4])


def _fast_path_clips(bpc):
    """the 70 x 21 half-static clip, the same kind of clip 3000 columns wide, and a clip that is still everywhere"""
    small = R.half_static_clip(11, bpc)
    return small, R.half_static_clip(12, bpc, w=3000, h=37, shift=90), [small[0]] * 3


# run in a child process of its own: a context made there cannot be one that an earlier test parked, and the switch is in the
# environment before the library is loaded
_FAST_PATH_CHILD = """
import sys
import numpy as np
from pqa2_amd import _native as N
from pqa2_amd.engine import FeatureEngine
from tests.test_gpu_deinterlace import _fast_path_clips
out = {}
for bpc in (8, 10, 12):
    with FeatureEngine(64, 48, bit_depth=bpc, n_planes=1, features=N.FEAT_PSNR) as eng:
        for c, clip in enumerate(_fast_path_clips(bpc)):
            for first in (0, 1):
                out[f"{bpc}_{c}_{first}"] = np.stack(eng.deinterlace(clip, "adaptive", first, "field"))
np.savez(sys.argv[1], **out)
print("fast-path child ok")
"""


def test_half_static_noise_and_the_fast_path(tmp_path):
    """the 70 x 21 clip whose left half is still: all four branches inside one wave and, at the seam column 35, inside one 16-byte
    piece.  The same kind of clip 3000 columns wide: whole waves are still and take the fast path, the waves of the right half do
    not, the wave with the seam holds both.  PQA_DEINT_UNIFORM=0 (read at pqa_create) sends every wave down the general path: each
    setting runs in a fresh child process, and both give the restatement's planes at 8, 10 and 12 bit"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    got = {}
    for uniform in ("default", "0"):
        env = dict(os.environ, PYTHONPATH=root)
        env.pop("PQA_DEINT_UNIFORM", None)
        if uniform == "0":
            env["PQA_DEINT_UNIFORM"] = "0"
        path = str(tmp_path / f"uniform_{uniform}.npz")
        r = subprocess.run([sys.executable, "-c", _FAST_PATH_CHILD, path], env=env, cwd=root, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "fast-path child ok" in r.stdout, (uniform, r.stdout[-500:], r.stderr[-2000:])
        got[uniform] = np.load(path)
    for bpc in (8, 10, 12):
        clips = _fast_path_clips(bpc)
        stats = {}
        R.deinterlace(clips[0], "adaptive", 0, "field", bpc, stats)
        assert all(stats[k] > 0 for k in ("still", "temporal", "spatial", "clamp"))
        for c, clip in enumerate(clips):
            for first in (0, 1):
                want = np.stack(R.deinterlace(clip, "adaptive", first, "field", bpc))
                for uniform, planes in got.items():
                    g = planes[f"{bpc}_{c}_{first}"]
                    assert g.dtype == want.dtype and np.array_equal(g, want), (uniform, bpc, c, first)


@pytest.mark.parametrize("bpc", [8, 12])
def test_extreme_triples(bpc):
    planes = R.extreme_planes(bpc)
    with _engine(64, 48, bpc) as eng:
        for first in (0, 1):
            # the 6^3 triples as one clip each would be 216 calls: a de Bruijn-like walk instead -- every triple (P, C, N) occurs as
            # three consecutive frames of one clip
            clip = [planes[i] for trio in itertools.product(range(6), repeat=3) for i in trio]
            want = R.deinterlace(clip, "adaptive", first, "field", bpc)
            assert _same(eng.deinterlace(clip, "adaptive", first, "field"), want), first


@pytest.mark.parametrize("bpc", [8, 10])
def test_the_launch_seam_and_the_window(bpc):
    """random frames, n = 2 DEINT_CHUNK + 1 first (so that stale frames lie in the buffers), then DEINT_CHUNK and its neighbours:
    the host entry uploads every frame once and keeps the last two of a chunk as predecessors of the next, the resident entry
    launches DEINT_CHUNK source frames at a time; both equal the restatement output by output at both rates"""
    from pqa2_amd import _native as N
    K = N.DEINT_CHUNK
    src = _noise(50 + bpc, 2 * K + 1, 48, 32, bpc)
    with _engine(48, 32, bpc) as eng:
        for n in (2 * K + 1, K, K + 1, K + 2, 2 * K):
            for rate in R.RATES:
                want = R.deinterlace(src[:n], "adaptive", 1, rate, bpc)
                host = eng.deinterlace(src[:n], "adaptive", 1, rate)
                res = _resident(eng, src[:n], "adaptive", 1, rate)[0]
                assert len(host) == len(res) == len(want)
                for k in range(len(want)):
                    assert np.array_equal(host[k], want[k]), (n, rate, k, "host")
                    assert np.array_equal(res[k], want[k]), (n, rate, k, "resident")
        # a clip that starts inside the other one: its first frame must not see a predecessor left behind
        assert _same(eng.deinterlace(src[5:16], "adaptive", 0, "field"), R.deinterlace(src[5:16], "adaptive", 0, "field", bpc))
        assert _same(eng.deinterlace(src[:2], "adaptive", 0, "frame"), R.deinterlace(src[:2], "adaptive", 0, "frame", bpc))


@pytest.mark.parametrize("bpc", [8, 10])
def test_a_plane_size_other_than_the_contexts(bpc):
    with _engine(50, 18, bpc) as eng:
        for w, h in ((25, 9), (100, 70)):
            src = _noise(70 + w, 3, w, h, bpc)
            assert _same(eng.deinterlace(src, "adaptive", 0, "field"), R.deinterlace(src, "adaptive", 0, "field", bpc)), (w, h)


def test_independent_of_the_scoring_chain():
    from pqa2_amd import _native as N
    rng = np.random.default_rng(7)
    ref = [rng.integers(0, 256, (48, 64)).astype(np.uint8) for _ in range(6)]
    dis = [np.clip(r.astype(int) + rng.integers(-9, 10, r.shape), 0, 255).astype(np.uint8) for r in ref]
    other = _noise(8, 3, 100, 30, 8)

    def run(with_call):
        with _engine(64, 48, features=N.FEAT_VMAF | N.FEAT_PSNR | N.FEAT_SSIM, max_batch=4) as eng:
            got = []
            for i in range(6):
                eng.submit(i, [ref[i]], [dis[i]])
                if with_call and i in (0, 2, 4):    # inside a pending batch, and right after one was launched
                    got.append(eng.deinterlace(dis, "adaptive", 0, "field"))
                    got.append(eng.deinterlace(other, "intra", 1, "frame"))
            return eng.collect(0, 6), got
    plain, _ = run(False)
    mixed, got = run(True)
    assert np.array_equal(plain.view(np.uint64), mixed.view(np.uint64))
    assert len(got) == 6
    assert all(_same(g, R.deinterlace(dis, "adaptive", 0, "field")) for g in got[0::2])
    assert all(_same(g, R.deinterlace(other, "intra", 1, "frame")) for g in got[1::2])


def _e2e_files(tmp_path):
    """96 x 64 4:2:0: 16 progressive frames at 50 fps, their interlace to 8 frames tagged It, and the restated field clips"""
    import dataclasses
    from pqa2_amd.yuvio import VideoInfo, write_y4m
    from tests import field_ref
    info = VideoInfo(width=96, height=64, fps_num=25, fps_den=1, bit_depth=8, mono=False, hshift=1, vshift=1, chroma_tag="420", interlace="t")
    prog = field_ref.moving_clip(5, 16, 96, 64, wobble=0)
    woven = [[R.interlace([f[p] for f in prog], 0)[t] for p in range(3)] for t in range(8)]
    P = {}

    def restated(mode):
        planes = [R.deinterlace([f[p] for f in woven], mode, 0, "field") for p in range(3)]
        return [[planes[p][k] for p in range(3)] for k in range(16)]
    p50 = dataclasses.replace(info, fps_num=50, interlace="p")
    for name, frames, i in (("ref", prog, p50), ("cap", woven, info), ("adaptive", restated("adaptive"), p50), ("intra", restated("intra"), p50)):
        P[name] = str(tmp_path / (name + ".y4m"))
        write_y4m(P[name], frames, i)
    return P


def _bits(res):
    return res["records"].view(np.uint64)


def test_score_files_scores_an_interlaced_capture(tmp_path):
    from pqa2_amd.pipeline import score_files
    P = _e2e_files(tmp_path)
    kw = dict(psnr=True, ssim=True)
    got = score_files(P["ref"], P["cap"], "vmaf_v0.6.1", deinterlace="adaptive", deinterlace_rate="field", **kw)
    want = score_files(P["ref"], P["adaptive"], "vmaf_v0.6.1", **kw)
    assert len(got["records"]) == 16 and np.array_equal(_bits(got), _bits(want))
    assert got["input"]["deinterlace"] == {"side": "distorted", "mode": "adaptive", "rate": "field", "order": "tff",
                                           "declared": {"reference": "p", "distorted": "t"}, "frames": [8, 16]}
    intra = score_files(P["ref"], P["cap"], "vmaf_v0.6.1", deinterlace="intra", deinterlace_rate="field", **kw)
    assert np.array_equal(_bits(intra), _bits(score_files(P["ref"], P["intra"], "vmaf_v0.6.1", **kw)))
    print("mean psnr_y: adaptive", got["metrics"]["psnr_y"].mean(), "intra", intra["metrics"]["psnr_y"].mean())
    assert got["metrics"]["psnr_y"].mean() > intra["metrics"]["psnr_y"].mean()
    both = score_files(P["cap"], P["cap"], "vmaf_v0.6.1", deinterlace="adaptive", deinterlace_rate="field", deinterlace_side="both", **kw)
    assert np.array_equal(_bits(both), _bits(score_files(P["adaptive"], P["adaptive"], "vmaf_v0.6.1", **kw)))


def test_field_repair_interpolates_a_dropped_field(tmp_path):
    from pqa2_amd.pipeline import score_files
    from pqa2_amd.yuvio import VideoInfo, write_y4m
    from tests import field_ref
    info = VideoInfo(width=96, height=64, fps_num=25, fps_den=1, bit_depth=8, mono=False, hshift=1, vshift=1, chroma_tag="420")
    ref = field_ref.moving_clip(5, 10, 96, 64)
    cap = field_ref.top_doubled(field_ref.with_noise(ref, 105))
    planes = [R.deinterlace([f[p] for f in cap], "intra", 0, "frame") for p in range(3)]
    P = {}
    for name, frames in (("ref", ref), ("doubled", cap), ("repaired", [[planes[p][t] for p in range(3)] for t in range(10)])):
        P[name] = str(tmp_path / (name + ".y4m"))
        write_y4m(P[name], frames, info)
    kw = dict(psnr=True, ssim=True)
    today = score_files(P["ref"], P["doubled"], "vmaf_v0.6.1", field_align="apply", **kw)
    assert np.array_equal(_bits(today), _bits(score_files(P["ref"], P["doubled"], "vmaf_v0.6.1", **kw)))
    assert today["alignment"]["fields"]["kind"] == "single_field" and not today["alignment"]["fields"]["applied"]
    fixed = score_files(P["ref"], P["doubled"], "vmaf_v0.6.1", field_align="apply", field_repair=True, **kw)
    assert fixed["alignment"]["fields"]["applied"] is True and fixed["alignment"]["fields"]["repair"] == "intra"
    assert np.array_equal(_bits(fixed), _bits(score_files(P["ref"], P["repaired"], "vmaf_v0.6.1", **kw)))
