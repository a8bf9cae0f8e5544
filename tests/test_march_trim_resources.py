"""The instruction trims of the march kernels, read off the compiler's own listings (hipcc cross-compiles without a GPU;
flags as in csrc/build.sh), each against its partner built with the trim's compile-time switch off:

  PQA_SPLIT_FUSED_LO          vif_s0_march_kernel: the lo pieces come from v_fma_mixlo_f16 / v_fma_mixhi_f16 (residual and
                              rounding in one instruction): half the packed f32 -> f16 conversions, no v_fma_mix_f32 left
  PQA_MOTION_DPP_TAPS,        motion_march_kernel: no wave-shift move and no row-weight select in the marching loops, every
  PQA_MOTION_ROW_WEIGHT_PEEL  shifted operand is the DPP source of its own multiply / FMA
  PQA_ADM_SIGNED_BYTES        adm_pyramid_kernel<u8>: no packed add of -128 behind the dword loads of the fast path

and the register budgets that keep the kernels' occupancy.  The motion switches are on by default; the split's and the ADM
loader's are off (bit-identical, shorter, not faster: DESIGN.md section 10) and are compiled on here, so that the variants
stay buildable for a later measurement."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pqa2_amd", "csrc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only"]
BUILDS = {   # name -> (file, per-file flags of build.sh, switches)
    "vif": ("vif_march.hip", [], ["-DPQA_SPLIT_FUSED_LO=1"]),
    "vif_off": ("vif_march.hip", [], ["-DPQA_SPLIT_FUSED_LO=0"]),
    "motion": ("motion_march.hip", ["-fno-slp-vectorize"], []),
    "motion_off": ("motion_march.hip", ["-fno-slp-vectorize"], ["-DPQA_MOTION_DPP_TAPS=0", "-DPQA_MOTION_ROW_WEIGHT_PEEL=0"]),
    "adm": ("adm_pyramid.hip", ["-fno-slp-vectorize"], ["-DPQA_ADM_SIGNED_BYTES=1"]),
    "adm_off": ("adm_pyramid.hip", ["-fno-slp-vectorize"], ["-DPQA_ADM_SIGNED_BYTES=0"]),
}


@pytest.fixture(scope="module")
def listings(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("march_trim")
    procs = {n: subprocess.Popen([hipcc, *FLAGS, *per_file, *sw, os.path.join(CSRC, f), "-o", str(d / (n + ".s"))],
                                 stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
             for n, (f, per_file, sw) in BUILDS.items()}
    for n, p in procs.items():
        err = p.communicate()[1]
        assert p.returncode == 0, (n, err.decode()[-2000:])
    return {n: (d / (n + ".s")).read_text() for n in BUILDS}


def _functions(text):
    """mangled name -> the lines of its body"""
    return {m.group(1): m.group(2).split("\n") for m in re.finditer(r"^(_Z\S+):[^\n]*\n(.*?)^\.Lfunc_end", text, re.S | re.M)}


def _resources(text):
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^; Occupancy: (\d+)", text, re.S | re.M):
        body = m.group(2)
        out[m.group(1)] = {"vgprs": int(re.search(r"^; TotalNumVgprs: (\d+)", body, re.M).group(1)),
                           "scratch": int(re.search(r"^; ScratchSize: (\d+)", body, re.M).group(1)),
                           "occupancy": int(m.group(3))}
    return out


def _one(d, key):
    hit = [v for n, v in d.items() if key in n]
    assert len(hit) == 1, (key, sorted(d))
    return hit[0]


def _count(lines, pattern):
    return sum(1 for l in lines if re.search(pattern, l))


def _loops(lines):
    """[(first, last)] line ranges from a label to the LAST branch back to it (natural loops as the listing lays them out)"""
    labels = {m.group(1): i for i, l in enumerate(lines) for m in [re.match(r"^(\.LBB\d+_\d+):", l)] if m}
    loops = {}
    for i, l in enumerate(lines):
        m = re.search(r"\bs_c?branch\w*\s+(\.LBB\d+_\d+)", l)
        if m and labels.get(m.group(1), i) < i:
            loops[m.group(1)] = (labels[m.group(1)], i)
    return [lines[a:b + 1] for a, b in loops.values()]


# <uint8_t, false>, <uint16_t, false> (10 bit) and <uint16_t, true> (12 bit) as the Itanium ABI spells them
@pytest.mark.parametrize("inst", ["vif_s0_march_kernelIhLb0E", "vif_s0_march_kernelItLb0E", "vif_s0_march_kernelItLb1E"])
def test_split_lo_pieces_are_fused(listings, inst):
    new, old = _one(_functions(listings["vif"]), inst), _one(_functions(listings["vif_off"]), inst)
    cvt_new, cvt_old = _count(new, r"\bv_cvt_pk_f16_f32\b"), _count(old, r"\bv_cvt_pk_f16_f32\b")
    mix_new, mix_old = _count(new, r"\bv_fma_mix(lo|hi)_f16\b"), _count(old, r"\bv_fma_mix_f32\b")
    print(f"{inst}: v_cvt_pk_f16_f32 {cvt_old} -> {cvt_new}, v_fma_mix_f32 {mix_old} -> mixlo + mixhi {mix_new}")
    assert cvt_old > 0 and cvt_old % 2 == 0 and cvt_new * 2 == cvt_old
    assert mix_old > 0 and mix_new == mix_old
    assert _count(new, r"\bv_fma_mix_f32\b") == 0 and _count(old, r"\bv_fma_mix(lo|hi)_f16\b") == 0
    # a mixhi keeps the half its mixlo wrote: both write the same register
    assert _count(new, r"\bv_fma_mixlo_f16\b") == _count(new, r"\bv_fma_mixhi_f16\b")
    r = _one(_resources(listings["vif"]), inst)
    print(f"{inst}: {r}")
    assert r["vgprs"] <= 168 and r["scratch"] == 0 and r["occupancy"] >= 3, r


# the fast path loads a lane's two samples at once: a halfword of 8-bit samples, a dword of 16-bit ones (the edge path of
# the 16-bit instance is the one with halfword loads)
@pytest.mark.parametrize("inst,fast_load", [("motion_march_kernelIhE", "buffer_load_ushort"), ("motion_march_kernelItE", "buffer_load_dword")])
def test_motion_loops_have_no_wave_shift_moves_and_no_row_weight(listings, inst, fast_load):
    new, old = _one(_functions(listings["motion"]), inst), _one(_functions(listings["motion_off"]), inst)
    fast = [l for l in _loops(new) if _count(l, fast_load)]
    fast_old = [l for l in _loops(old) if _count(l, fast_load)]
    assert len(fast) == 1 and len(fast_old) == 1, (len(fast), len(fast_old))
    # the partner's loop is the one this looks for: it has the 16 moves and the 4 selects
    assert _count(fast_old[0], r"\bv_mov_b32_dpp\b") == 16 and _count(fast_old[0], r"\bv_cndmask_b32") == 4
    marching = [l for l in _loops(new) if _count(l, r"\bbuffer_load_")]   # fast path and edge path
    assert len(marching) == 2
    for loop in marching:
        fused_fma, fused_mul = _count(loop, r"\bv_fmac_f32_dpp\b"), _count(loop, r"\bv_mul_f32_dpp\b")
        valu = _count(loop, r"^\s+v_")
        print(f"{inst}: loop of {valu} vector instructions, {fused_fma} v_fmac_f32_dpp + {fused_mul} v_mul_f32_dpp")
        assert _count(loop, r"\bv_mov_b32_dpp\b") == 0 and _count(loop, r"\bv_cndmask_b32") == 0
        # per completed row three shifted operands per output column: two open a chain (a multiply), four extend one
        assert fused_fma + fused_mul >= 24 and fused_fma >= 16
    # -20 per step and lane: 16 moves, 4 selects (the |.|-accumulating FMAs become adds, one for one)
    assert _count(fast[0], r"^\s+v_") <= _count(fast_old[0], r"^\s+v_") - 20
    r = _one(_resources(listings["motion"]), inst)
    print(f"{inst}: {r}")
    assert r["vgprs"] <= 64 and r["scratch"] == 0, r


def test_adm_fast_path_converts_signed_bytes(listings):
    new, old = _one(_functions(listings["adm"]), "adm_pyramid_kernelIhE"), _one(_functions(listings["adm_off"]), "adm_pyramid_kernelIhE")

    def fast_loops(lines):   # the march loops behind the fast path's dword loads (the edge path loads byte by byte)
        return [l for l in _loops(lines) if _count(l, r"\bbuffer_load_dword\b") and not _count(l, r"\bbuffer_load_ubyte\b")]
    assert fast_loops(new) and len(fast_loops(new)) == len(fast_loops(old))
    for a, b in zip(fast_loops(new), fast_loops(old)):
        valu_new, valu_old = _count(a, r"^\s+v_"), _count(b, r"^\s+v_")
        print(f"adm_pyramid_kernel<u8> fast loop: v_pk_add_f32 {_count(b, 'v_pk_add_f32')} -> {_count(a, 'v_pk_add_f32')}, "
              f"vector instructions {valu_old} -> {valu_new}")
        # the only packed adds of these loops were the -128 of the sample conversion (the constant sits in an SGPR pair, so
        # the instruction itself does not show it: the partner's count says which adds they were)
        assert _count(b, r"\bv_pk_add_f32\b") > 0 and _count(a, r"\bv_pk_add_f32\b") == 0
        assert _count(a, r"^\s+v_") < _count(b, r"^\s+v_")
    assert _count(new, "0x80808080") > 0
    r = _one(_resources(listings["adm"]), "adm_pyramid_kernelIhE")
    print(f"adm_pyramid_kernel<u8>: {r}")
    assert r["vgprs"] <= 168 and r["scratch"] == 0 and r["occupancy"] >= 3, r
    # the 16-bit instance does not see the switch: instruction for instruction what it was
    u16_new, u16_old = _one(_functions(listings["adm"]), "adm_pyramid_kernelItE"), _one(_functions(listings["adm_off"]), "adm_pyramid_kernelItE")
    strip = lambda lines: [re.sub(r"\s+", " ", l.split(";")[0]).strip() for l in lines if re.match(r"^\s+[sv]_|^\s+(buffer|ds|global)_", l)]
    assert strip(u16_new) == strip(u16_old)
