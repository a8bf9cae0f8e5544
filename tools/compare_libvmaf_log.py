#!/usr/bin/env python3
"""One-command pinning of this repo's restatements against a real libvmaf run.

Nothing in this repo can run libvmaf (no ffmpeg / vmaf binary in the image, none on the GPU box), so parity with
libvmaf is UNPINNED.  Whoever has a box with a libvmaf-enabled ffmpeg can close that in two
commands, using the clips committed under tests/golden/clips/:

    ffmpeg -i tests/golden/clips/c352x288_8_dist.y4m -i tests/golden/clips/c352x288_8_ref.y4m \\
           -lavfi "libvmaf=log_fmt=json:log_path=lv.json:model=version=vmaf_v0.6.1:n_threads=4" -f null -
    python tools/compare_libvmaf_log.py lv.json tests/golden/clips/c352x288_8_ref.y4m tests/golden/clips/c352x288_8_dist.y4m

(the same filter line the reference builds, app/vmaf_analyzer.py:373-419: input 0 = distorted, input 1 = reference).
For the float extractors use model=version=vmaf_float_v0.6.1 (metric keys without the integer_ prefix); a `vmaf`
CLI JSON (--json, --feature float_vif ...) has the same per-frame schema and works as well.

For every per-frame metric of the log that this repo computes, the tool prints the largest absolute difference
against (a) the f32 restatement oracle/vmaf_oracle.c with the border rule the key implies, (b) the fixed-point
restatement oracle/vmaf_int_oracle.c for integer_* keys, (c) with --gpu, the HIP kernels (f32 path, and the
fixed-point mode for integer_* keys), and names the VERIFY items of the restatements each mismatch implicates.
Exit code 0 when every compared metric is inside its bar (the log prints %.6f: bar 2e-6 for exact restatements,
--tol for the f32 ones), 1 otherwise.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# metric family -> what a mismatch implicates (file:line of the VERIFY item in the restatements)
IMPLICATES = {
    "vif_scale0": ["float: border rule of vif_tools.c convolution (oracle/vmaf_oracle.c:47-57 mirror), 17-tap table "
                   "(:gaussian taps), vif_statistic_s branch order (:154-191)",
                   "integer: reflect-101 padding (oracle/vmaf_int_oracle.c:37 [VERIFY]), MAX(sigma2_sq,0) (:187 [VERIFY]), "
                   "Q formats / log2 LUT of the scale-0 path (:11 header)"],
    "vif_scale1": ["decimation phase: filter with THIS scale's kernel then keep even samples (oracle/vmaf_oracle.c:209-218)",
                   "integer: shifts of the deeper-scale path, rounding constants (oracle/vmaf_int_oracle.c:11)"],
    "vif_scale2": ["as vif_scale1"], "vif_scale3": ["as vif_scale1"],
    "adm2": ["sum-of-scales epilogue and the numden limit (pqa2_amd/model.py metrics_from_records)"],
    "adm_scale0": ["db2 taps / mirror (oracle/vmaf_oracle.c:241-342), Watson CSF factors, decouple cos^2(1deg) test, "
                   "3x3 CM with the extra centre weight (:397-418), crop (int)(w*0.1-0.5) (:347-353)",
                   "integer: range normalisation (oracle/vmaf_int_oracle.c:337 [VERIFY]), literal rfactor constants "
                   "(:533 [VERIFY]), div_lookup table, cube-accumulator shifts"],
    "adm_scale1": ["as adm_scale0 (int32 band path at scales 1-3 for integer_*)"],
    "adm_scale2": ["as adm_scale1"], "adm_scale3": ["as adm_scale1"],
    "motion": ["5-tap blur table and border; SAD normalisation (oracle/vmaf_oracle.c motion); integer: Q8 rounding "
               "after each pass (oracle/vmaf_int_oracle.c motion)"],
    "motion2": ["min(motion_i, motion_{i+1}) rule and frame-0 / last-frame handling (pqa2_amd/model.py:195-200)"],
    "vmaf": ["SVM predict / score clip (pqa2_amd/model.py:40-80) if every feature matches; otherwise a consequence"],
}
FAMILIES = ["vif_scale0", "vif_scale1", "vif_scale2", "vif_scale3", "adm2", "adm_scale0", "adm_scale1", "adm_scale2",
            "adm_scale3", "motion", "motion2"]


# the SSIM family (libvmaf float_ssim / float_ms_ssim; tests/ssim_family_ref.py states the definition) -> VERIFY items
SSIM_IMPLICATES = {
    "float_ssim": ["f = max(1, round(min(w,h)/256)), box window [x - f//2, x - f//2 + f), sample offset 0, ceil size and "
                   "half-sample symmetric border of iqa's _iqa_decimate (tests/ssim_family_ref.py box_decimate [VERIFY])",
                   "11x11 Gaussian sigma 1.5 over the valid region; literal (rounded) taps in libvmaf? (gaussian_taps [VERIFY])",
                   "s / 2^(bpc-8) sample conversion (to_float [VERIFY]); sqrt(max(sx2,0)*max(sy2,0)) clamp (lcs_maps [VERIFY])"],
    "float_ms_ssim": ["9/7 low-pass taps, half-sample symmetric border, keep samples 0,2,4,... -> ceil(n/2) "
                      "(lpf97_decimate [VERIFY])",
                      "separate means of c and s per scale rather than the mean of c*s (ms_combine [VERIFY])",
                      "weights 0.0448/0.2856/0.3001/0.2363/0.1333, l only at the 5th scale (MS_WEIGHTS [VERIFY])",
                      "as float_ssim: Gaussian taps, sample conversion, clamp"],
}


def ssim_family_columns(ref_path, dis_path, want_fs, want_ms, use_gpu, n):
    """{tag: {key: per-frame column}} of float_ssim / float_ms_ssim (+ the l/c/s means under libvmaf's enable_lcs names)
    from the restatement and, with use_gpu, from the HIP kernels (pqa_collect_ext)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ssim_family_ref as SR
    from pqa2_amd.yuvio import open_video
    rr, dr = open_video(ref_path), open_video(dis_path)
    info = rr.info
    refs = [rr.frame(i)[0] for i in range(n)]
    diss = [dr.frame(i)[0] for i in range(n)]

    def cols(ext):
        c = {}
        if want_fs:
            c["float_ssim"] = ext[:, 0]
            for j, k in enumerate("lcs"):
                c[f"float_ssim_{k}"] = ext[:, 1 + j]
        if want_ms:
            c["float_ms_ssim"] = ext[:, 4]
            for j, k in enumerate("lcs"):
                for s in range(5):
                    c[f"float_ms_ssim_{k}_scale{s}"] = ext[:, 5 + 5 * j + s]
        return c
    out = {"f64 restatement (tests/ssim_family_ref.py)":
           cols(np.stack([SR.ext_record(refs[i], diss[i], info.bit_depth, want_fs, want_ms) for i in range(n)]))}
    if use_gpu:
        from pqa2_amd import _native as N
        from pqa2_amd.engine import FeatureEngine
        feats = (N.FEAT_FLOAT_SSIM if want_fs else 0) | (N.FEAT_MS_SSIM if want_ms else 0)
        with FeatureEngine(info.width, info.height, bit_depth=info.bit_depth, features=feats) as eng:
            for i in range(n):
                eng.submit(i, [refs[i]], [diss[i]])
            out["HIP kernels (csrc/ssim_family.hip)"] = cols(eng.collect_ext(0, n)[1])
    return out

# libvmaf ciede (log key ciede2000; tests/ciede_ref.py states the definition, every constant in its CONST table) -> VERIFY items
SSIM_IMPLICATES["ciede2000"] = [
    "chroma upsampled to luma size by replication (tests/ciede_ref.py upsample [VERIFY])",
    "Y = y/(255 s), U = u/(255 s) - 0.5 with s = 2^(bpc-8): chroma centred at 0.5 or at 128/255 (CONST chroma_offset [VERIFY])",
    "BT.709 analog Y'UV matrix R = Y + 1.28033 V, G = Y - 0.21482 U - 0.38059 V, B = Y + 2.12798 U, no clamp (CONST [VERIFY])",
    "sRGB transfer c > 0.04045 ? ((c + 0.055) / 1.055)^2.4 : c / 12.92, x 100",
    "4-digit D65 sRGB -> XYZ matrix vs the 7-digit one (CONST xyz [VERIFY])",
    "Lab white (95.047, 100, 108.883), f(t) = t > 0.008856 ? cbrt(t) : 7.787 t + 16/116",
    "dE00 with kL = kC = kH = 1, Sharma's hue-mean rule, h' = 0 where a' = b = 0",
    "score 45 - 20 log10(mean dE00), and what libvmaf writes at mean 0 (here +inf) [VERIFY]",
]


def ciede_columns(ref_path, dis_path, use_gpu, n):
    """{tag: {"ciede2000": per-frame column}} from the f64 restatement and, with use_gpu, from the HIP kernel."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ciede_ref as CR
    from pqa2_amd.yuvio import open_video
    rr, dr = open_video(ref_path), open_video(dis_path)
    info = rr.info
    if info.mono:
        raise SystemExit("ciede2000 in the log but the clips are monochrome")
    refs = [rr.frame(i) for i in range(n)]
    diss = [dr.frame(i) for i in range(n)]
    out = {"f64 restatement (tests/ciede_ref.py)":
           {"ciede2000": np.array([CR.frame_slots(refs[i], diss[i], info.bit_depth, info.hshift, info.vshift)[0]
                                   for i in range(n)])}}
    if use_gpu:
        from pqa2_amd import _native as N
        from pqa2_amd.engine import FeatureEngine
        with FeatureEngine(info.width, info.height, bit_depth=info.bit_depth, n_planes=3, chroma_shift=(info.hshift, info.vshift),
                           features=N.FEAT_CIEDE) as eng:
            for i in range(n):
                eng.submit(i, refs[i], diss[i])
            out["HIP kernel (csrc/ciede.hip)"] = {"ciede2000": eng.collect_ext(0, n)[1][:, N.EXT_CIEDE2000]}
    return out


# libvmaf cambi (log keys cambi, cambi_source, cambi_full_reference; tests/cambi_ref.py, every constant in CONST) -> VERIFY
CAMBI_KEYS = ("cambi", "cambi_source", "cambi_full_reference")
SSIM_IMPLICATES["cambi"] = [
    "8-bit samples x 4 with no 2x2 anti-dithering average (tests/cambi_ref.py preprocess [VERIFY])",
    "spatial mask: 7x7 sum of D > 24, T fixed rather than resolution-dependent (CONST mask_threshold [VERIFY])",
    "window ws = ((65 (W + H)) // 375) >> 4, r = ws >> 1 (CONST ws_* [VERIFY rounding])",
    "mode filter: min of three distinct values, rows 0 / h-1 keep their decimated samples (mode3 [VERIFY])",
    "TVI: BT.1886 EOTF Lw = 300, Lb = 0.01, Weber threshold 0.019 (CONST eotf_*, tvi_threshold [VERIFY])",
    "contrast weights {1, 2, 3, 4} (CONST contrast_weights [VERIFY])",
    "top-k pooling k = clamp(int(0.6 N), 1, N), unmasked zeros included (CONST topk [VERIFY truncation])",
    "cambi_full_reference = max(cambi - cambi_source, 0) (full_reference [VERIFY])",
]


def cambi_columns(ref_path, dis_path, use_gpu, n):
    """{tag: {key: per-frame column}} of the three cambi keys from the restatement and, with use_gpu, the HIP kernels."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cambi_ref as KR
    from pqa2_amd.yuvio import open_video
    rr, dr = open_video(ref_path), open_video(dis_path)
    info = rr.info
    if info.bit_depth not in KR.CONST["bit_depths"]:
        raise SystemExit(f"cambi in the log but the clips are {info.bit_depth}-bit (cambi is defined at 8 and 10 bit here)")
    refs = [rr.frame(i)[0] for i in range(n)]
    diss = [dr.frame(i)[0] for i in range(n)]

    def cols(dis, src):
        return {"cambi": dis, "cambi_source": src,
                "cambi_full_reference": np.array([KR.full_reference(a, b) for a, b in zip(dis, src)])}
    out = {"restatement (tests/cambi_ref.py)": cols(np.array([KR.cambi(d, info.bit_depth) for d in diss]),
                                                    np.array([KR.cambi(r, info.bit_depth) for r in refs]))}
    if use_gpu:
        from pqa2_amd import _native as N
        from pqa2_amd.engine import FeatureEngine
        with FeatureEngine(info.width, info.height, bit_depth=info.bit_depth,
                           features=N.FEAT_CAMBI | N.FEAT_CAMBI_FULL_REF) as eng:
            for i in range(n):
                eng.submit(i, [refs[i]], [diss[i]])
            ext = eng.collect_ext(0, n)[1]
        out["HIP kernels (csrc/cambi.hip)"] = cols(ext[:, N.EXT_CAMBI], ext[:, N.EXT_CAMBI_SOURCE])
    return out


# libvmaf psnr_hvs (log keys psnr_hvs_y / _cb / _cr, psnr_hvs; tests/psnr_hvs_ref.py, every constant in CONST) -> VERIFY
PSNR_HVS_KEYS = ("psnr_hvs_y", "psnr_hvs_cb", "psnr_hvs_cr", "psnr_hvs")
SSIM_IMPLICATES["psnr_hvs"] = [
    "samples as raw codes with max = 2^bpc - 1, or libvmaf's float copy scaled to 8 bit and truncated to int16 at "
    "10 / 12 bit (tests/psnr_hvs_ref.py blocks_of, db [VERIFY])",
    "od_bin_fdct8 lifting constants and the rounding of OD_DCT_RSHIFT (CONST lifts, _rshift [VERIFY])",
    "coef^2 of the mask formed in int or in float (exact either way below 2^31 here; f32 rounding above 2^24) [VERIFY]",
    "the 4:2:0 chroma CSF tables used for 4:2:2 and 4:4:4 too (CONST csf_cb420 / csf_cr420 [VERIFY])",
    "psnr_hvs from 0.8 mse_Y + 0.1 (mse_Cb + mse_Cr) before the dB step (CONST weights [VERIFY])",
    "the value written at mse 0 (here +inf, as psnr's inf) [VERIFY]",
]


def psnr_hvs_columns(ref_path, dis_path, use_gpu, n):
    """{tag: {key: per-frame column}} of the four psnr_hvs keys from the restatement and, with use_gpu, the HIP kernel."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import psnr_hvs_ref as HR
    from pqa2_amd.yuvio import open_video
    rr, dr = open_video(ref_path), open_video(dis_path)
    info = rr.info
    if info.mono:
        raise SystemExit("psnr_hvs in the log but the clips are monochrome (psnr_hvs needs the chroma planes)")
    frames = [(rr.frame(i), dr.frame(i)) for i in range(n)]
    res = [HR.psnr_hvs(r, d, info.bit_depth) for r, d in frames]
    out = {"restatement (tests/psnr_hvs_ref.py)": {k: np.array([x[k] for x in res]) for k in PSNR_HVS_KEYS}}
    if use_gpu:
        from pqa2_amd import _native as N
        from pqa2_amd.engine import FeatureEngine
        with FeatureEngine(info.width, info.height, bit_depth=info.bit_depth, n_planes=3,
                           chroma_shift=(info.hshift, info.vshift), features=N.FEAT_PSNR_HVS) as eng:
            for i, (r, d) in enumerate(frames):
                eng.submit(i, r, d)
            ext2 = eng.collect_blocks(0, n, [1])[1][1]
        out["HIP kernel (csrc/psnr_hvs.hip)"] = {k: ext2[:, s] for k, s in zip(
            PSNR_HVS_KEYS, (N.EXT2_PSNR_HVS_Y, N.EXT2_PSNR_HVS_CB, N.EXT2_PSNR_HVS_CR, N.EXT2_PSNR_HVS))}
    return out


def load_log(path):
    with open(path) as f:
        d = json.load(f)
    frames = sorted(d["frames"], key=lambda fr: fr["frameNum"])
    keys = sorted({k for fr in frames for k in fr["metrics"]})
    cols = {k: np.array([fr["metrics"].get(k, np.nan) for fr in frames], np.float64) for k in keys}
    return [fr["frameNum"] for fr in frames], cols, d


def our_columns(ref_path, dis_path, model_name, integer_keys, use_gpu, frame_nums):
    """dict name -> {metric key -> per-frame array} for each restatement / kernel path that applies."""
    from oracle.oracle import Oracle
    from pqa2_amd import model as M
    from pqa2_amd.yuvio import open_video
    rd, dd = open_video(ref_path), open_video(dis_path)
    info = rd.info
    n = min(len(rd), len(dd))
    refs = [np.asarray(rd.frame(i)[0]) for i in range(n)]
    diss = [np.asarray(dd.frame(i)[0]) for i in range(n)]
    mdl = M.load_model(model_name)
    prefix = "integer_" if integer_keys else ""
    out = {}

    def cols_from(rec17, tag):
        rec = np.zeros((n, 24))
        rec[:, :17] = rec17
        m = M.score_frames(mdl, M.metrics_from_records(rec, info.width, info.height, prefix))
        out[tag] = {k: np.asarray(v)[frame_nums] for k, v in m.items()}

    orc = Oracle("f32")
    cols_from(orc.clip_features(refs, diss, info.bit_depth, vif_gain_limit=mdl.vif_enhn_gain_limit,
                                adm_gain_limit=mdl.adm_enhn_gain_limit, vif_border101=integer_keys),
              "f32 restatement (oracle/vmaf_oracle.c, %s border)" % ("integer_vif.c" if integer_keys else "vif_tools.c"))
    if integer_keys:
        from oracle.int_oracle import IntOracle
        cols_from(IntOracle().clip_features(refs, diss, info.bit_depth, mdl.vif_enhn_gain_limit, mdl.adm_enhn_gain_limit),
                  "fixed-point restatement (oracle/vmaf_int_oracle.c)")
    if use_gpu:
        from pqa2_amd import _native as N
        from pqa2_amd.engine import FeatureEngine
        for tag, fx in (("HIP f32 kernels", 0),) + ((("HIP fixed-point kernels", N.FIXED_ALL),) if integer_keys else ()):
            with FeatureEngine(info.width, info.height, bit_depth=info.bit_depth, vif_border=int(integer_keys),
                               vif_enhn_gain_limit=mdl.vif_enhn_gain_limit, adm_enhn_gain_limit=mdl.adm_enhn_gain_limit,
                               fixed_point=fx) as eng:
                for i in range(n):
                    eng.submit(i, [refs[i]], [diss[i]])
                cols_from(eng.collect(0, n)[:, :17], tag)
    return out, n


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("libvmaf_json")
    ap.add_argument("reference")
    ap.add_argument("distorted")
    ap.add_argument("--model", default=None, help="default: vmaf_v0.6.1 for integer_* logs, vmaf_float_v0.6.1 otherwise")
    ap.add_argument("--gpu", action="store_true", help="also run the HIP kernels (needs an MI355X)")
    ap.add_argument("--tol", type=float, default=2e-5, help="bar for the f32 paths on a feature (default 2e-5)")
    ap.add_argument("--vmaf-tol", type=float, default=0.01, help="bar on the vmaf score (north_star: 0.01)")
    a = ap.parse_args(argv)

    frame_nums, log, raw = load_log(a.libvmaf_json)
    integer_keys = any(k.startswith("integer_") for k in log)
    model = a.model or ("vmaf_v0.6.1" if integer_keys else "vmaf_float_v0.6.1")
    print(f"libvmaf log: version {raw.get('version', '?')}, {len(frame_nums)} frames, "
          f"{'integer_*' if integer_keys else 'float'} feature keys; model {model}")
    ours, n = our_columns(a.reference, a.distorted, model, integer_keys, a.gpu, frame_nums)
    if max(frame_nums, default=-1) >= n:
        print(f"error: the log has frame {max(frame_nums)} but the clips hold {n} frames", file=sys.stderr)
        return 2
    prefix = "integer_" if integer_keys else ""
    bad = False
    for tag, cols in ours.items():
        exact = tag.startswith("fixed-point") or tag.startswith("HIP fixed")
        print(f"\n== {tag} ==")
        print(f"{'metric':28s} {'max |ours - libvmaf|':>22s} {'at frame':>9s}   bar     verdict")
        for fam in FAMILIES + ["vmaf"]:
            key = fam if fam == "vmaf" else prefix + fam
            if key not in log or key not in cols:
                continue
            d = np.abs(cols[key] - log[key])
            j = int(np.nanargmax(d)) if d.size else 0
            bar = a.vmaf_tol if fam == "vmaf" else (2e-6 if exact else a.tol)
            ok = bool(np.nanmax(d) <= bar) if d.size else True
            print(f"{key:28s} {np.nanmax(d) if d.size else 0.0:22.3e} {frame_nums[j] if d.size else 0:9d}   {bar:.0e}   "
                  f"{'ok' if ok else 'MISMATCH'}")
            if not ok:
                bad = True
                for line in IMPLICATES.get(fam, []):
                    if ("integer:" in line) and not integer_keys:
                        continue
                    print(f"{'':28s}   -> check: {line}")
    want_fs, want_ms = "float_ssim" in log, "float_ms_ssim" in log
    if want_fs or want_ms:
        for tag, cols in ssim_family_columns(a.reference, a.distorted, want_fs, want_ms, a.gpu, n).items():
            print(f"\n== SSIM family: {tag} ==")
            for key in sorted(k for k in cols if k in log):
                d = np.abs(cols[key][frame_nums] - log[key])
                j = int(np.nanargmax(d)) if d.size else 0
                ok = bool(np.nanmax(d) <= a.tol) if d.size else True
                print(f"{key:28s} {np.nanmax(d) if d.size else 0.0:22.3e} {frame_nums[j] if d.size else 0:9d}   "
                      f"{a.tol:.0e}   {'ok' if ok else 'MISMATCH'}")
                if not ok:
                    bad = True
                    fam = "float_ms_ssim" if key.startswith("float_ms_ssim") else "float_ssim"
                    for line in SSIM_IMPLICATES[fam]:
                        print(f"{'':28s}   -> check: {line}")
    if "ciede2000" in log:
        for tag, cols in ciede_columns(a.reference, a.distorted, a.gpu, n).items():
            print(f"\n== ciede2000: {tag} ==")
            d = np.abs(cols["ciede2000"][frame_nums] - log["ciede2000"])
            d = np.where(np.isinf(cols["ciede2000"][frame_nums]) & (cols["ciede2000"][frame_nums] == log["ciede2000"]), 0.0, d)
            j = int(np.nanargmax(d)) if d.size else 0
            ok = bool(np.nanmax(d) <= a.tol) if d.size else True
            print(f"{'ciede2000':28s} {np.nanmax(d) if d.size else 0.0:22.3e} {frame_nums[j] if d.size else 0:9d}   "
                  f"{a.tol:.0e}   {'ok' if ok else 'MISMATCH'}")
            if not ok:
                bad = True
                for line in SSIM_IMPLICATES["ciede2000"]:
                    print(f"{'':28s}   -> check: {line}")
    if any(k in log for k in CAMBI_KEYS):
        for tag, cols in cambi_columns(a.reference, a.distorted, a.gpu, n).items():
            print(f"\n== cambi: {tag} ==")
            for key in (k for k in CAMBI_KEYS if k in log):
                d = np.abs(cols[key][frame_nums] - log[key])
                j = int(np.nanargmax(d)) if d.size else 0
                ok = bool(np.nanmax(d) <= a.tol) if d.size else True
                print(f"{key:28s} {np.nanmax(d) if d.size else 0.0:22.3e} {frame_nums[j] if d.size else 0:9d}   "
                      f"{a.tol:.0e}   {'ok' if ok else 'MISMATCH'}")
                if not ok:
                    bad = True
                    for line in SSIM_IMPLICATES["cambi"]:
                        print(f"{'':28s}   -> check: {line}")
    if any(k in log for k in PSNR_HVS_KEYS):
        for tag, cols in psnr_hvs_columns(a.reference, a.distorted, a.gpu, n).items():
            print(f"\n== psnr_hvs: {tag} ==")
            for key in (k for k in PSNR_HVS_KEYS if k in log):
                d = np.abs(cols[key][frame_nums] - log[key])
                d = np.where(np.isinf(cols[key][frame_nums]) & (cols[key][frame_nums] == log[key]), 0.0, d)
                j = int(np.nanargmax(d)) if d.size else 0
                ok = bool(np.nanmax(d) <= a.tol) if d.size else True
                print(f"{key:28s} {np.nanmax(d) if d.size else 0.0:22.3e} {frame_nums[j] if d.size else 0:9d}   "
                      f"{a.tol:.0e}   {'ok' if ok else 'MISMATCH'}")
                if not ok:
                    bad = True
                    for line in SSIM_IMPLICATES["psnr_hvs"]:
                        print(f"{'':28s}   -> check: {line}")
    missing = [prefix + f for f in FAMILIES if prefix + f not in log]
    if missing:
        print(f"\nnot in the log (not compared): {', '.join(missing)}")
    print("\nRESULT:", "MISMATCH -- see the implicated VERIFY items above" if bad else
          "every compared metric inside its bar: this log pins the restatement(s) listed above for these clips")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
