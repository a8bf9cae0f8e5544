// What the plane-scan kernels share (tile_moments, temporal_moments, band_moments, edge_profiles, line_profiles, level_stats;
// flow_moments and colour_moments take a piece each): they read one or two planes once, keep integer sums per lane, reduce them
// in the wave and in LDS and write uint64 words.  Device: the two row loads and the exact wave sums.  Host: the load-width
// rule, its dispatch, and the head of the argument structs with its validation.  It lives beside pqa_device.h and not in it
// because that file is part of the source hash the committed counters of the VIF and ADM kernels are tied to (bench.py,
// kernel_source_hash).
#pragma once
#include <algorithm>
#include <type_traits>

#include "kernels.h"
#include "pqa_device.h"

namespace pqa {

// ---- device: 16 bytes of a row as four packed dwords ---------------------------------------------------------------------
struct PackedQuad {
  unsigned d[4];
};

enum QuadTail { kTailZeros, kTailRepeat };   // what a sample past the end of the row reads as: zero, or the row's last sample

// the S = 16 / sizeof(T) samples x ... x + S - 1 of a row that ends before x1 as four packed dwords.  VB: bytes of one load
// where the whole 16 bytes lie inside the row; otherwise sample by sample, nothing past the row's last sample is touched.
// kTailRepeat: a sample past the end is read as the row's last one: it is a real address (band_moments: no coefficient that
// counts sees it).
template <typename T, int VB, QuadTail TAIL>
__device__ __forceinline__ PackedQuad quad_load(const T* row, int x, int x1) {
  constexpr int S = 16 / (int)sizeof(T), PER = 4 / (int)sizeof(T), BITS = 8 * (int)sizeof(T);
  PackedQuad q;
  if (x + S <= x1 && VB == 16) {
    const uint4 v = *reinterpret_cast<const uint4*>(row + x);
    q.d[0] = v.x; q.d[1] = v.y; q.d[2] = v.z; q.d[3] = v.w;
  } else if (x + S <= x1 && VB == 4) {
#pragma unroll
    for (int k = 0; k < 4; ++k) q.d[k] = *reinterpret_cast<const unsigned*>(row + x + k * PER);
  } else if constexpr (TAIL == kTailZeros) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      unsigned v = 0u;
#pragma unroll
      for (int s = 0; s < PER; ++s) {
        const int xx = x + k * PER + s;
        if (xx < x1) v |= (unsigned)row[xx] << (BITS * s);
      }
      q.d[k] = v;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      unsigned u = 0u;
#pragma unroll 1   // rolled: unrolled, every sample's address is live at once
      for (int s = PER - 1; s >= 0; --s) {
        const int xx = x + k * PER + s;
        u = (u << BITS) | (unsigned)row[xx < x1 ? xx : x1 - 1];
      }
      q.d[k] = u;
    }
  }
  return q;
}

// ---- device: V samples of a row as a vector ---------------------------------------------------------------------------------
template <typename T, int V>
struct alignas(sizeof(T) * V) SampleVec {
  T s[V];
};

// the samples x ... x + V - 1 of a row that ends before x1, none above top (u16; by default as they are); zeros past the end
template <typename T, int V>
__device__ __forceinline__ SampleVec<T, V> vec_load(const T* row, int x, int x1, unsigned top = 0xffffffffu) {
  SampleVec<T, V> v;
  if (x + V <= x1) {
    v = *reinterpret_cast<const SampleVec<T, V>*>(row + x);
  } else {
#pragma unroll
    for (int k = 0; k < V; ++k) v.s[k] = x + k < x1 ? row[x + k] : (T)0;
  }
  if constexpr (sizeof(T) > 1) {
#pragma unroll
    for (int k = 0; k < V; ++k) v.s[k] = (T)min((unsigned)v.s[k], top);
  }
  return v;
}

// ---- device: exact wave sums ---------------------------------------------------------------------------------------------
// Wave64 sums of one 32-bit value per lane, exact, returned wave-uniform in 64 bits; the DPP controls of wave_sum_f32
// (pqa_device.h) with an integer add in place of dpp_add's float one.  Every lane of the wave must be active.
template <int CTRL>
__device__ __forceinline__ unsigned dpp_iadd(unsigned v) {
  return v + (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true);
}
// unsigned: four steps leave the sum of each row of 16 lanes in its lane 15 -- every one of them must fit 32 bits -- and the four
// row sums are read and added in 64 bits
__device__ __forceinline__ unsigned long long wave_sum_u32(unsigned v) {
  v = dpp_iadd<0xb1>(v);    // quad_perm:[1,0,3,2]
  v = dpp_iadd<0x4e>(v);    // quad_perm:[2,3,0,1]
  v = dpp_iadd<0x114>(v);   // row_shr:4
  v = dpp_iadd<0x118>(v);   // row_shr:8   -> lane 15 of each row holds the row sum
  return (unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)v, 15) + (unsigned)__builtin_amdgcn_readlane((int)v, 31) +
         (unsigned)__builtin_amdgcn_readlane((int)v, 47) + (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}
// signed: three steps leave the sum of lanes 16 r ... 16 r + 7 in lane 16 r + 7 and of lanes 16 r + 8 ... 16 r + 15 in lane
// 16 r + 15 (two's complement adds: the unsigned add above is the signed one); each must fit int32.  edge_profiles: 8 lanes of
// at most 16 top^2 in magnitude, 128 * 4095^2 = 2 146 435 200 <= 2^31 - 1.  One step more (256 * 4095^2) would not.
__device__ __forceinline__ long long wave_sum_i32(int s) {
  unsigned v = (unsigned)s;
  v = dpp_iadd<0xb1>(v);
  v = dpp_iadd<0x4e>(v);
  v = dpp_iadd<0x114>(v);   // lanes 4 ... 15 of a row: their quad and the one before
  long long t = 0;
#pragma unroll
  for (int l = 7; l < 64; l += 8) t += (long long)__builtin_amdgcn_readlane((int)v, l);
  return t;
}

// adds to a uint64 word of LDS (ds_add_u64, no return)
__device__ __forceinline__ void lds_add(unsigned long long* p, unsigned long long v) {
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// ---- host: the head of the argument structs --------------------------------------------------------------------------------
struct PairPlanes {
  const void* ref;
  const void* dis;
  int64_t ref_rp, ref_fp, dis_rp, dis_fp;   // elements
  int w, h;
};

// what every launcher asks of its planes: samples of 8, 10 or 12 bits in the container that goes with them, 1 ... max_wh each way
inline bool scan_shape_ok(Elem elem, int bits, int w, int h, int max_wh = 8192) {
  return (bits == 8 || bits == 10 || bits == 12) && (elem == ELEM_U8) == (bits == 8) && w >= 1 && h >= 1 && w <= max_wh &&
         h <= max_wh;
}

// fills p from a launcher's arguments; false (p untouched) when scan_shape_ok says no
inline bool pair_planes(PairPlanes& p, Elem elem, int bits, const void* ref, int64_t ref_row_pitch, int64_t ref_frame_pitch,
                        const void* dis, int64_t dis_row_pitch, int64_t dis_frame_pitch, int w, int h, int max_wh = 8192) {
  if (!scan_shape_ok(elem, bits, w, h, max_wh)) return false;
  p = PairPlanes{ref, dis, ref_row_pitch, ref_frame_pitch, dis_row_pitch, dis_frame_pitch, w, h};
  return true;
}

// ---- host: the load width --------------------------------------------------------------------------------------------------
// bytes of one load (16, 4 or a sample's, u8 / u16): the widest every lane is aligned to whatever the row and frame, given that
// a lane starts a multiple of 16 bytes into its row.  Pitches in elements.
inline int load_bytes(Elem elem, const void* base, int64_t row_pitch, int64_t frame_pitch) {
  const int es = elem == ELEM_U8 ? 1 : 2;
  const uint64_t bits = (uint64_t)(uintptr_t)base | (uint64_t)((row_pitch | frame_pitch) * es);
  return bits % 16 == 0 ? 16 : bits % 4 == 0 ? 4 : es;
}
// two planes read by the same lanes: what BOTH allow
inline int load_bytes(Elem elem, const PairPlanes& p) {
  return std::min(load_bytes(elem, p.ref, p.ref_rp, p.ref_fp), load_bytes(elem, p.dis, p.dis_rp, p.dis_fp));
}

// calls f(T(), std::integral_constant<int, VB>()) with the sample type of `elem` (u8 / u16) and VB = vb where that is 16 or 4,
// sizeof(T) otherwise: the template arguments of the caller's launch_v
template <typename F>
hipError_t dispatch(Elem elem, int vb, F&& f) {
  const auto with = [&](auto t) {
    if (vb == 16) return f(t, std::integral_constant<int, 16>());
    if (vb == 4) return f(t, std::integral_constant<int, 4>());
    return f(t, std::integral_constant<int, (int)sizeof(t)>());
  };
  if (elem == ELEM_U8) return with(uint8_t());
  if (elem == ELEM_U16) return with(uint16_t());
  return hipErrorInvalidValue;
}

}  // namespace pqa
