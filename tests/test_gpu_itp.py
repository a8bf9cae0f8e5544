"""Delta E ITP on the MI355X (csrc/delta_itp.hip, pqa_delta_itp): the kernel's ICtCp device function and the full path against
the f64 restatement (tests/itp_ref.py), with the restatement's own f32 mode as the yardstick; exact results where the
definition is exact; bit-identical rows across every way frames reach the kernel; the argument rules; the pipeline with one
and two ranks.

The yardstick: E32 = the worst distance 720 ||(I, T, P)_f32 - (I, T, P)_f64|| of the restatement's f32 mode on 100 000 seeded
code triples of the transfer and depth; the kernel must stay within TOL = 4 E32 (the hardware log2 / exp2 are a few ulp, numpy's
powers are correctly rounded).  Measured on the MI355X (worst kernel distance / E32): pq 10 bit 0.0649 / 0.0722, hlg 10 bit
0.0782 / 0.0667, bt1886 8 bit 0.0336 / 0.0376, pq 12 bit 0.0612 / 0.0653.

The issue's case 130 x 10 is below the 16 x 16 a context accepts (pqa_create refuses it); 130 x 18 stands in for it: in 4:4:4
it is two whole tiles and two columns wide, four whole tile rows and two rows high."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import itp_ref as R
from tests.test_gpu_ciede import _planes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [("pq", 10), ("hlg", 10), ("bt1886", 8), ("pq", 12)]


def _triples(bpc, seed=5, n=100_000):
    """half uniform over the code cube, half near-neutral (chroma mid +- N(0, 40) at 10 bit, scaled with the depth)"""
    rng = np.random.default_rng(seed)
    top, mid = (1 << bpc) - 1, 1 << (bpc - 1)
    cube = rng.integers(0, top + 1, (n // 2, 3)).astype(np.float64)
    y = rng.integers(0, top + 1, (n // 2, 1)).astype(np.float64)
    c = np.clip(np.rint(mid + rng.normal(0, 40.0 * (1 << bpc) / 1024, (n // 2, 2))), 0, top)
    return np.vstack([cube, np.hstack([y, c])])


def _spec(transfer, bpc, **kw):
    """(the spec the library gets, the restatement's own f64 spec)"""
    from pqa2_amd import itp
    matrix = "bt2020" if transfer != "bt1886" else "bt709"
    return itp.spec(transfer, matrix, False, bpc, **kw), R.make_spec(transfer, matrix, False, bpc, **kw)


@functools.lru_cache(maxsize=None)
def _yardstick(transfer, bpc):
    """(E32, the f64 coordinates of the sample): computed once, shared, left unchanged"""
    t = _triples(bpc)
    ref = R.make_spec(transfer, bit_depth=bpc)
    want = R.ictcp(t, ref)
    e32 = float(np.linalg.norm(R.ictcp(t, ref, np.float32).astype(np.float64) - want, axis=-1).max())
    want.setflags(write=False)
    return e32, want


def _tol(transfer, bpc):
    return 4.0 * _yardstick(transfer, bpc)[0]


def _debug(sp, triples):
    from pqa2_amd import _native as N, itp
    lib = N.load()
    t = np.ascontiguousarray(triples, np.float32).reshape(-1, 3)
    out = np.zeros_like(t)
    ns = itp.native_spec(sp)
    assert lib.pqa_debug_itp(C.byref(ns), t.ctypes.data, t.shape[0], out.ctypes.data) == N.PQA_OK
    return out.astype(np.float64)


@pytest.mark.parametrize("transfer,bpc", CONFIGS)
def test_debug_hook_against_f64(transfer, bpc):
    e32, want = _yardstick(transfer, bpc)
    got = _debug(_spec(transfer, bpc)[0], _triples(bpc))
    d = np.linalg.norm(got - want, axis=-1)
    print(f"\n{transfer} {bpc} bit: worst kernel distance {d.max():.4f} (mean {d.mean():.4f}); E32 {e32:.4f}, bound {4 * e32:.4f}")
    assert np.isfinite(got).all()
    assert d.max() <= 4.0 * e32


def test_debug_hook_greys_are_neutral():
    for transfer, bpc in CONFIGS:
        mid = 1 << (bpc - 1)
        y = np.arange(0, 1 << bpc, 7, dtype=np.float64)
        got = _debug(_spec(transfer, bpc)[0], np.column_stack([y, np.full_like(y, mid), np.full_like(y, mid)]))
        assert (got[:, 1] == 0.0).all() and (got[:, 2] == 0.0).all(), (transfer, bpc)


# ---- the full path -------------------------------------------------------------------------------------------------
def _engine(w, h, bpc, hs, vs, **kw):
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    return FeatureEngine(w, h, bit_depth=bpc, n_planes=3, chroma_shift=(hs, vs), features=kw.pop("features", N.FEAT_PSNR), **kw)


GEOMETRIES = [(64, 48, 1, 1), (64, 48, 1, 0), (64, 48, 0, 0), (161, 161, 1, 1), (161, 161, 1, 0), (161, 161, 0, 0),
              (130, 18, 0, 0), (161, 161, 2, 2), (161, 161, 0, 2), (352, 288, 1, 1)]


def _check_rows(rows, refs, diss, ref_spec, hs, vs, tol, what):
    thr = ref_spec["threshold"]
    for i in range(len(refs)):
        de, d, i_ref = R.frame_de(refs[i], diss[i], ref_spec, hs, vs)
        px = de.size
        mean, mx = de.mean(), de.max()
        lo, hi = int((de > thr + 2 * tol).sum()), int((de > thr - 2 * tol).sum())
        r = rows[i]
        print(f"\n{what} frame {i}: mean {r[0] / px:.5f} (f64 {mean:.5f}), max {r[4]:.4f} (f64 {mx:.4f}), above {int(r[5])} "
              f"(f64 {lo} ... {hi}), 2 TOL {2 * tol:.4f}")
        assert r[6] == px
        assert abs(r[0] / px - mean) <= 2 * tol
        assert abs(r[4] - mx) <= 2 * tol
        assert lo <= r[5] <= hi
        # the remaining slots: rms parts within the same per-pixel bound, the reference's intensity within its coordinate's
        for k in range(3):
            assert abs(np.sqrt(r[1 + k] / px) - np.sqrt((d[..., k] ** 2).mean())) <= 2 * tol
        assert abs(r[7] / px - i_ref.mean() / 720.0) <= tol / 720.0


@pytest.mark.parametrize("transfer,bpc", CONFIGS)
@pytest.mark.parametrize("w,h,hs,vs", GEOMETRIES)
def test_full_path_against_f64(w, h, hs, vs, transfer, bpc):
    sp, ref_spec = _spec(transfer, bpc)
    frames = [_planes(w, h, bpc, hs, vs, seed=w + h + bpc + 7 * i + hs) for i in range(2)]
    refs, diss = [f[0] for f in frames], [f[1] for f in frames]
    with _engine(w, h, bpc, hs, vs) as eng:
        rows = eng.delta_itp(refs, diss, sp)
    _check_rows(rows, refs, diss, ref_spec, hs, vs, _tol(transfer, bpc), f"{w}x{h} ({hs},{vs}) {transfer} {bpc} bit")


# ---- exactness ------------------------------------------------------------------------------------------------------
def test_identical_clips_give_zero():
    w, h, bpc = 161, 161, 10
    r, _ = _planes(w, h, bpc, 1, 1, seed=3)
    for transfer in ("pq", "hlg"):
        with _engine(w, h, bpc, 1, 1) as eng:
            rows = eng.delta_itp([r, r], [r, r], _spec(transfer, bpc)[0])
        assert (rows[:, :6] == 0.0).all() and (rows[:, 6] == w * h).all() and (rows[:, 7] > 0).all()


def test_flat_grey_pair_is_pure_luminance():
    w, h, bpc = 64, 48, 10
    sp, _ = _spec("pq", bpc)

    def grey(v):
        return [np.full((h, w), v, np.uint16), np.full((h // 2, w // 2), 512, np.uint16), np.full((h // 2, w // 2), 512, np.uint16)]
    with _engine(w, h, bpc, 1, 1) as eng:
        rows = eng.delta_itp([grey(502)], [grey(503)], sp)
        back = eng.delta_itp([grey(503)], [grey(502)], sp)
    tol = _tol("pq", bpc)
    px = w * h
    print(f"\ngrey 502 / 503: mean {rows[0, 0] / px:.6f}, max {rows[0, 4]:.6f}")
    assert abs(rows[0, 0] / px - 0.82192) <= 2 * tol and abs(rows[0, 4] - 0.82192) <= 2 * tol
    assert rows[0, 2] == 0.0 and rows[0, 3] == 0.0
    assert rows[0, 5] == 0 and rows[0, 6] == px
    assert np.array_equal(rows[0, :7], back[0, :7])      # dE is symmetric


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("bpc", [8, 10])
def test_bit_identical_across_entries_pitches_alignment_and_chunks(bpc):
    import torch
    from pqa2_amd import _native as N
    w, h, hs, vs = 64, 48, 1, 1
    n = N.ITP_CHUNK + 1
    sp, _ = _spec("pq" if bpc == 10 else "bt1886", bpc)
    frames = [_planes(w, h, bpc, hs, vs, seed=90 + i) for i in range(n)]
    refs, diss = [f[0] for f in frames], [f[1] for f in frames]
    dt = np.uint8 if bpc == 8 else np.uint16
    es = np.dtype(dt).itemsize
    with _engine(w, h, bpc, hs, vs) as eng:
        base = eng.delta_itp(refs, diss, sp)
        assert base.shape == (n, N.ITP_SUMS) and (base[:, 0] > 0).all()
        for i in range(n):      # a frame's row does not depend on the call it is part of
            one = eng.delta_itp(refs[i:i + 1], diss[i:i + 1], sp)
            assert np.array_equal(_bits(one[0]), _bits(base[i])), i
        # host frames as views of padded arrays (row strides larger than a row)
        pad = [[np.zeros((p.shape[0], p.shape[1] + 5 + k), dt) for k, p in enumerate(f)] for f in refs]
        views = []
        for f, big in zip(refs, pad):
            for k in range(3):
                big[k][:, :f[k].shape[1]] = f[k]
            views.append([big[k][:, :f[k].shape[1]] for k in range(3)])
        assert np.array_equal(_bits(eng.delta_itp(views, diss, sp)), _bits(base))
        # device-resident planes: tight and aligned, padded pitches, a base 16 bytes + one sample off
        sizes = [(w, h), (w >> hs, h >> vs), (w >> hs, h >> vs)]
        for off, padw in ((0, 0), (16 // es + 1, 3), (7, 13)):
            ptrs, keep, rps, fps = ([], []), [], [], []
            for p, (pw, ph) in enumerate(sizes):
                pitch = pw + padw + p
                rps.append(pitch * es)
                fps.append(ph * pitch * es)
                for side, src in enumerate((refs, diss)):
                    buf = np.full(off + n * ph * pitch, 0xA5, dt)
                    for i in range(n):
                        buf[off + i * ph * pitch: off + (i + 1) * ph * pitch].reshape(ph, pitch)[:, :pw] = src[i][p]
                    t = torch.from_numpy(buf.view(np.uint8)).cuda()
                    keep.append(t)
                    ptrs[side].append(t.data_ptr() + off * es)
            torch.cuda.synchronize()
            got = eng.delta_itp_resident(ptrs[0], ptrs[1], rps, fps, n, sp)
            assert np.array_equal(_bits(got), _bits(base)), f"resident offset {off} pad {padw}"
        assert eng.delta_itp([], [], sp).shape == (0, N.ITP_SUMS)


def test_a_call_changes_nothing_in_the_records():
    from pqa2_amd import _native as N
    w, h, bpc, n = 64, 48, 10, 5
    frames = [_planes(w, h, bpc, 1, 1, seed=60 + i) for i in range(n)]
    refs, diss = [f[0] for f in frames], [f[1] for f in frames]
    sp, _ = _spec("pq", bpc)
    out = []
    for call in (False, True):
        with _engine(w, h, bpc, 1, 1, features=N.FEAT_ALL, max_batch=2) as eng:
            for i in range(n):
                eng.submit(i, refs[i], diss[i])
                if call and i == 2:
                    eng.delta_itp(refs[:3], diss[:3], sp)
            out.append(eng.collect(0, n))
    assert np.array_equal(_bits(out[0]), _bits(out[1]))


# ---- argument rules -----------------------------------------------------------------------------------------------
def test_argument_rules():
    from pqa2_amd import _native as N, itp
    from pqa2_amd.engine import FeatureEngine
    w, h, bpc = 64, 48, 10
    sp, _ = _spec("hlg", bpc)
    r, d = _planes(w, h, bpc, 1, 1, seed=1)
    out = np.zeros((1, N.ITP_SUMS))

    def lists(eng, frames):
        keep, ptrs, strides = eng._frame_list(frames, "reference")
        return keep, ptrs, strides

    with _engine(w, h, bpc, 1, 1) as eng:
        lib, ctx = eng.lib, eng._ctx
        kr, rp, rs = lists(eng, [r])
        kd, dp, ds = lists(eng, [d])

        def host(ns, rp_=rp, rs_=rs, dp_=dp, ds_=ds, n=1, out_=out.ctypes.data):
            rc = lib.pqa_delta_itp(ctx, ns, rp_, C.byref(rs_) if rs_ is not None else None, dp_,
                                   C.byref(ds_) if ds_ is not None else None, n, out_)
            return rc, lib.pqa_last_error(ctx).decode()

        def bad(**change):
            ns = itp.native_spec(sp)
            for k, v in change.items():
                if isinstance(v, tuple):
                    getattr(ns, k)[v[0]] = v[1]
                else:
                    setattr(ns, k, v)
            return C.byref(ns)

        assert host(bad())[0] == N.PQA_OK
        cases = [("unknown transfer", bad(transfer=3)), ("not finite", bad(yuv_to_rgb=(5, float("nan")))),
                 ("not finite", bad(rgb_to_lms=(8, float("inf")))), ("peak", bad(peak=0.0)), ("peak", bad(peak=-1.0)),
                 ("peak", bad(peak=float("nan"))), ("threshold", bad(threshold=-0.5)), ("threshold", bad(threshold=float("inf")))]
        for word, ns in cases:
            rc, msg = host(ns)
            assert rc == N.PQA_EINVAL and "delta_itp" in msg and word in msg, (word, msg)
        ns = itp.native_spec(sp)
        ns.transfer, ns.peak = N.ITP_PQ, -1.0      # PQ does not read the peak
        assert host(C.byref(ns))[0] == N.PQA_OK
        for word, kw in (("null spec", dict(ns=None)), ("null frame list", dict(ns=bad(), rp_=None)),
                         ("null frame list", dict(ns=bad(), ds_=None)), ("null output", dict(ns=bad(), out_=None)),
                         ("negative frame count", dict(ns=bad(), n=-1))):
            rc, msg = host(**kw)
            assert rc == N.PQA_EINVAL and "delta_itp" in msg and word in msg, (word, msg)
        assert host(bad(), n=0, out_=None)[0] == N.PQA_OK
        short = (C.c_int64 * 3)(w * 2 - 2, rs[1], rs[2])
        rc, msg = host(bad(), rs_=short)
        assert rc == N.PQA_EINVAL and "delta_itp" in msg and "stride smaller than a row" in msg
        null = (C.c_void_p * 3)(rp[0], None, rp[2])
        rc, msg = host(bad(), rp_=null)
        assert rc == N.PQA_EINVAL and "delta_itp" in msg and "pointer is null" in msg
        # clips in device memory: null clip, null plane, a pitch that is no multiple of the sample size, one below a row
        def dev(clip_r, clip_d, n=1):
            rc = lib.pqa_delta_itp_device(ctx, bad(), clip_r, clip_d, n, out.ctypes.data)
            return rc, lib.pqa_last_error(ctx).decode()
        import torch
        t = torch.zeros(w * h * 2 * 2, dtype=torch.uint8).cuda()
        good = eng._device_clip([t.data_ptr()] * 3, [w * 2, w, w], [w * h * 2, w * h // 2, w * h // 2])
        assert dev(C.byref(good), C.byref(good))[0] == N.PQA_OK
        rc, msg = dev(None, C.byref(good))
        assert rc == N.PQA_EINVAL and "delta_itp" in msg and "null clip" in msg
        for word, change in (("pointer is null", ("plane", 1, None)), ("multiple of the sample size", ("row_pitch", 0, w * 2 + 1)),
                             ("pitch smaller than a row", ("row_pitch", 2, w - 2))):
            c = eng._device_clip([t.data_ptr()] * 3, [w * 2, w, w], [w * h * 2, w * h // 2, w * h // 2])
            getattr(c, change[0])[change[1]] = change[2]
            rc, msg = dev(C.byref(good), C.byref(c))
            assert rc == N.PQA_EINVAL and "delta_itp" in msg and word in msg, (word, msg)
        del kr, kd
    with FeatureEngine(w, h, bit_depth=bpc, n_planes=1, features=N.FEAT_PSNR) as mono:
        rc = mono.lib.pqa_delta_itp(mono._ctx, C.byref(itp.native_spec(sp)), rp, C.byref(rs), dp, C.byref(ds), 1, out.ctypes.data)
        msg = mono.lib.pqa_last_error(mono._ctx).decode()
        assert rc == N.PQA_EINVAL and "delta_itp" in msg and "n_planes must be 3" in msg


# ---- the pipeline -------------------------------------------------------------------------------------------------
def test_score_files_columns_and_two_ranks(tmp_path):
    import socket
    from pqa2_amd import synth, yuvio
    w, h, n, bpc = 64, 48, 5, 10
    frames = [_planes(w, h, bpc, 1, 1, seed=20 + i) for i in range(n)]
    refs, diss = [f[0] for f in frames], [f[1] for f in frames]
    info = synth.clip_info(w, h, bpc, chroma=True)
    rp, dp = str(tmp_path / "r.y4m"), str(tmp_path / "d.y4m")
    yuvio.write_y4m(rp, refs, info)
    yuvio.write_y4m(dp, diss, info)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, PYTHONPATH=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0")
    outs = {}
    for tag, launcher in (("one", []), ("two", ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                                                 "--master-addr", "127.0.0.1", "--master-port", str(port)])):
        j = str(tmp_path / f"{tag}.json")
        cmd = [sys.executable] + launcher + ["-m", "pqa2_amd.score", rp, dp, "--json", j, "--batch", "2", "--delta-itp", "pq"]
        if launcher:
            cmd += ["--backend", "gloo", "--share-device"]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        d = json.load(open(j))
        d.pop("fps", None)
        outs[tag] = d
    assert outs["one"] == outs["two"]
    log = outs["one"]
    ref_spec = R.make_spec("pq", bit_depth=bpc)
    tol = _tol("pq", bpc)
    assert log["delta_itp"]["spec"]["transfer"] == "pq" and len(log["delta_itp"]["spec"]["yuv_to_rgb"]) == 12
    assert np.abs(np.array(log["delta_itp"]["spec"]["yuv_to_rgb"]) - ref_spec["yuv_to_rgb"].ravel()).max() <= 1e-7
    means = []
    for i, fr in enumerate(log["frames"]):
        de, _, _ = R.frame_de(refs[i], diss[i], ref_spec, 1, 1)
        m = fr["metrics"]
        assert abs(m["delta_e_itp"] - de.mean()) <= 2 * tol + 5e-7
        assert abs(m["delta_e_itp_max"] - de.max()) <= 2 * tol + 5e-7
        assert (de > 1 + 2 * tol).mean() - 5e-7 <= m["itp_above_jnd"] <= (de > 1 - 2 * tol).mean() + 5e-7
        means.append(de.mean())
    assert abs(log["pooled_metrics"]["delta_e_itp"]["mean"] - np.mean(means)) <= 2 * tol + 1e-6
    assert abs(log["delta_itp"]["summary"]["mean"] - np.mean(means)) <= 2 * tol
    assert log["delta_itp"]["summary"]["kind"] in ("luminance", "chroma", "mixed")
