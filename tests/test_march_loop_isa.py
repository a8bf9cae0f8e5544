"""What the march loops of vif_s0_march_kernel and adm_pyramid_kernel no longer carry, read off the compiler's own gfx950
listing (hipcc cross-compiles without a GPU; same command lines as tests/test_abi.py):

  scale 0   the next-scale store's address is formed once per segment and moved by one 64-bit add per block (of the parent's
            six v_mad_u64_u32 the four of the store are gone; the two of the mirrored-row load path are not part of this
            change and are pinned where they are), mu * mu enters the packed FMAs through
            neg_lo / neg_hi (no v_xor_b32 with the sign bit), the ballot is an OR of the compares' scalar masks (no
            v_cndmask_b32 / v_cmp_ne_u32 pair).  The prefetch registers that alternate with the loop's halves were measured
            and taken out again (profiles/r21a_march_loops_ab.txt B), so the v_mov_b64 of the hand-over
            are still there, printed and not asserted on;
  pyramid   the 8-bit instance runs two scale-1 rows per trip, so that window rows, pending sets and the prefetch queue swap
            by name: fewer register-to-register moves in a loop that is now TWO rows long.

A loop is every basic block the listing marks as belonging to the loop of one `Inner Loop Header` (block placement moves the
back-branch around, the marks do not care).  The parent's figures below are this file's own counts on the commit before
(9ae55e5, same compiler): the listing then had, per instance, the numbers in PARENT_*."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (v_mad_u64_u32, v_xor_b32, v_mov_b64, v_cmp_ne_u32) in the march loop of vif_s0_march_kernel<S, B12> on the parent commit
PARENT_S0 = {"ItLb1E": (6, 12, 14, 2), "ItLb0E": (6, 12, 16, 2), "IhLb0E": (6, 12, 10, 2)}   # 12-, 10-, 8-bit instance
# VGPR-to-VGPR v_mov_b32 / v_mov_b64 in the two march loops (edge stripes, inner stripes) of adm_pyramid_kernel<uint8_t> on
# the parent commit, one scale-1 row per trip; the second figure is the 19 moves at the back-edge of the inner-stripe loop
PARENT_PYRAMID_U8 = (11, 19)


def _listing(tmp_path, name, *flags):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "pqa2_amd", "csrc", name + ".hip")
    out = tmp_path / (name + ".s")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", *flags, "-S", "--cuda-device-only", src, "-o", str(out)],
                   check=True, capture_output=True)
    return out.read_text()


def loop_blocks(text):
    """[(function, [(label or None, instruction before the block in the listing, [instruction lines])])] for every innermost
    loop, blocks in the order of the listing; the header block's label is the one `Inner Loop Header` names"""
    func, cur, prev, found, order = None, None, None, {}, []
    for line in text.split("\n"):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            func, cur = m.group(1), None
            continue
        if re.match(r"^(\.LBB\d+_\d+:|; %bb\.\d+:)", line):
            label = re.match(r"^\.(LBB\d+_\d+):", line)
            head = label and "Inner Loop Header" in line
            inside = re.search(r"in Loop: Header=(BB\d+_\d+)", line)
            key = (func, label.group(1)[1:]) if head else (func, inside.group(1)) if inside else None
            cur = None
            if key:
                if key not in found:
                    found[key] = []
                    order.append(key)
                cur = (label.group(1) if label else None, prev, [])
                found[key].append(cur)
            continue
        if re.match(r"^\s+[a-z]", line):
            prev = line.strip()
            if cur:
                cur[2].append(prev)
    return [(k[0], "L" + k[1], found[k]) for k in order]


def loops(text):
    """[(function, [instruction lines])]: the same loops, blocks run together"""
    return [(f, [l for _, _, b in blocks for l in b]) for f, _, blocks in loop_blocks(text)]


def count(lines, mnemonic):
    return sum(1 for l in lines if re.match(mnemonic + r"(_e32|_e64)?\b", l))


def reg_moves(lines):
    return sum(1 for l in lines if re.match(r"v_mov_b(32|64)(_e32)? v[\[\d:\]]+, v[\[\d:\]]+$", l))


def test_scale0_march_loop_lost_its_address_math_negations_and_ballot_round_trip(tmp_path):
    text = _listing(tmp_path, "vif_march")
    seen = set()
    for inst, (mad0, xor0, mov0, cne0) in PARENT_S0.items():
        mine = [b for f, b in loops(text) if "vif_s0_march_kernel" + inst in f]
        assert mine, inst
        march = max(mine, key=len)                      # (the other loop of the kernel copies the tap table into LDS)
        assert sum(1 for l in march if l.startswith("v_mfma_f32_16x16x32_f16")) == 76, inst   # two blocks of 38
        mad, xor, mov, cne = (count(march, m) for m in ("v_mad_u64_u32", "v_xor_b32", "v_mov_b64", "v_cmp_ne_u32"))
        print(inst, "v_mad_u64_u32", mad0, "->", mad, " v_xor_b32", xor0, "->", xor, " v_cmp_ne_u32", cne0, "->", cne, " v_mov_b64", mov0, "->", mov)
        # The issue asked for none.  Four of the parent's six built the store's address and are gone; the other two belong to the
        # load path of blocks whose rows are mirrored (my * pitch for the second image, one per half of the loop body), which
        # this change does not touch: exactly two, each in a block that issues buffer loads and stores nothing, and no block
        # that stores to the next scale's planes multiplies
        assert mad == 2, (inst, mad)
        blocks = [b for _, _, b in max([bl for f, _, bl in loop_blocks(text) if "vif_s0_march_kernel" + inst in f],
                                       key=lambda bl: sum(len(b) for _, _, b in bl))]
        with_mad = [b for b in blocks if count(b, "v_mad_u64_u32")]
        assert len(with_mad) == 2, inst
        for b in with_mad:
            assert count(b, "v_mad_u64_u32") == 1 and any(l.startswith("buffer_load") for l in b), inst
            assert not any(l.startswith("global_store") for l in b), inst
        storing = [b for b in blocks if any(l.startswith("global_store") for l in b)]
        assert storing and not any(l.startswith(("v_mad_u64_u32", "v_mul_lo_u32", "v_mul_hi_u32", "v_mad_i64_i32")) for b in storing for l in b), inst
        assert xor < xor0 and xor == 0, (inst, xor)
        assert cne < cne0 and cne == 0, (inst, cne)
        seen.add(inst)
    assert len(seen) == 3


def test_pyramid_march_loop_swaps_names_instead_of_copying(tmp_path):
    """Both loops of the 8-bit instance hold two scale-1 rows per trip and fewer moves than one row did.  The inner-stripe loop
    is held to the claim itself: register moves and `s_waitcnt vmcnt(0)` exist only in a block that is entered by a branch
    taken after the first row of a trip (the trip that ends there, at most once per segment) -- a full trip meets neither.
    (The edge-stripe loop packs its byte-wise loads at the end of a trip and still waits for all of them there.)"""
    text = _listing(tmp_path, "adm_pyramid", "-fno-slp-vectorize")
    mine = [(head, blocks) for f, head, blocks in loop_blocks(text)
            if "adm_pyramid_kernelIhE" in f and sum(len(b) for _, _, b in blocks) > 300]
    assert len(mine) == 2, len(mine)
    for (head, blocks), before in zip(mine, PARENT_PYRAMID_U8):
        body = [l for _, _, b in blocks for l in b]
        rows = sum(1 for l in body if l.startswith("buffer_store_dword")) // 2    # one pair of approximation stores per scale-1 row
        moves = reg_moves(body)
        print("adm_pyramid_kernel<u8>: scale-1 rows per trip", rows, " register moves", before, "->", moves)
        assert rows == 2
        assert moves < before, (moves, before)           # fewer in all, over twice the rows
    head, blocks = mine[1]                               # inner stripes: one four-sample load per lane, image and row
    h = [i for i, (label, _, _) in enumerate(blocks) if label == head]
    assert len(h) == 1
    from_header = [l for _, _, b in blocks[h[0]:] for l in b]
    off_path = 0
    for label, before_it, b in blocks:
        if not (reg_moves(b) or any("vmcnt(0)" in l for l in b)):
            continue
        off_path += 1
        assert label and label != head, b[:3]
        assert before_it.startswith(("s_branch", "s_endpgm", "s_setpc")), (label, before_it)   # nothing falls into it
        jumps = [i for i, l in enumerate(from_header) if re.match(r"s_cbranch_\w+ \." + label + r"$", l)]
        assert jumps and not any(re.match(r"s_branch \." + label + r"$", l) for l in body), label
        for i in jumps:   # after the first row's pair of stores, before the second row's
            assert sum(1 for l in from_header[:i] if l.startswith("buffer_store_dword")) == 2, label
    print("adm_pyramid_kernel<u8>, inner stripes: blocks with moves or vmcnt(0), all off the full trip's path:", off_path)
    assert off_path <= 1
