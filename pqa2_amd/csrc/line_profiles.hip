// Active-picture detection: the row and column profiles of the planes of one clip (pqa_line_profiles /
// pqa_line_profiles_device; restated in tests/profile_ref.py; the solver is pqa2_amd/align.py, active_picture).  For one plane
// of w x h samples v (a sample above top = 2^bits - 1, which a u16 container can hold, is read as top):
//
//   rows[f][y][0] = sum_x v[y][x]     rows[f][y][1] = sum_x v[y][x]^2
//   cols[f][x][0] = sum_y v[y][x]     cols[f][x][1] = sum_y v[y][x]^2
//
// exact uint64; out[f] holds the h row pairs, then the w column pairs.
//
// Work.  A workgroup of 256 threads owns one stripe of kProfStripe = 1024 columns and one band of kProfBand = 64 rows of one
// plane, and reads every sample of it ONCE for both profiles.  Wave wv takes the rows wv, wv + 4, ... of the band; a lane owns
// kProfLane = 16 columns of the stripe whatever the load width: with loads of V samples (16 bytes, 4 bytes or one sample,
// whichever base address and pitches allow; the host decides once per launch) load j of a row covers the columns
// x0 + (64 j + lane) V ... + V - 1, j < 16 / V.  A load that would cross the end of the row is read sample by sample, so
// nothing beyond the row's last sample is touched; a larger pitch or an odd base only selects the load width.  A wave loads
// kProfRows = 4 of its rows before it adds them up, to keep that many loads in flight.
// Columns.  The 16 column pairs of a lane live in 32 uint32 registers while the wave walks down the band.  They are widened --
// added to the workgroup's uint64 table in LDS (ds_add_u64) and cleared -- after at most `flush` rows,
//   flush = floor((2^32 - 1) / top^2):  66 051 rows at 8 bit, 4 104 at 10 bit, 256 at 12 bit
// (a column of 8192 rows of 4095 sums to 8192 * 4095^2 > 2^36 in its squares: 32 bits do not hold it), which the launcher
// derives from the bit depth; a wave walks kProfBand / 4 = 16 rows of a band, so today one widening at the end of the band is
// all there is.  After a barrier the workgroup adds the non-zero entries of its table to the zeroed output with 64-bit integer
// global atomics: the bands of a stripe meet there.
// Rows.  A lane adds the 16 samples of its columns and their squares in uint32 (16 top^2 <= 16 * 4095^2 < 2^29), the wave adds
// the lanes with the DPP steps of pqa_device.h's wave sum (wave_sum_u32 below: the sums of 16 lanes, 256 samples, stay below 256 * 4095^2
// = 4 292 870 400 < 2^32; the four of them are added in 64 bits), and one lane adds the pair to the output with 64-bit
// atomics: the stripes of a row meet there.  Every lane of a wave runs every row step: the DPP steps read all 64 lanes.
// Integer sums do not depend on order: the result is independent of scheduling, base address, pitch and tail.  No floating
// point anywhere.  Output: a plane of 8192 x 8192 samples of 4095 keeps a line's squares below 2^13 * 2^24 = 2^37.
#include "kernels.h"
#include "pqa_device.h"

namespace pqa {
namespace {

constexpr int kProfLane = kProfStripe / 64;   // columns of a lane
constexpr int kProfRows = 4;                  // rows a wave loads before it adds them

struct ProfArgs {
  const void* base;
  int64_t rp, fp;   // elements
  int w, h, flush;
  unsigned top;
  unsigned long long* out;   // [frame][h + w][2], zeroed
};

template <typename T, int V>
struct alignas(sizeof(T) * V) ProfVec {
  T s[V];
};

// the samples x ... x + V - 1 of a row that ends before x1; zeros past the end
template <typename T, int V>
__device__ __forceinline__ ProfVec<T, V> prof_load(const T* row, int x, int x1) {
  ProfVec<T, V> v;
  if (x + V <= x1) {
    v = *reinterpret_cast<const ProfVec<T, V>*>(row + x);
  } else {
#pragma unroll
    for (int k = 0; k < V; ++k) v.s[k] = x + k < x1 ? row[x + k] : (T)0;
  }
  return v;
}

// Wave64 sum of one uint32 per lane, exact, returned wave-uniform in 64 bits: the first four DPP steps of wave_sum_f32
// (pqa_device.h; the same controls, an integer add in place of dpp_add's float one) leave the sum of each row of 16 lanes in
// its lane 15 -- every one of them must fit 32 bits -- and the four row sums are read and added in 64 bits.  Every lane of the
// wave must be active.  It lives here and not beside wave_sum_f32 because pqa_device.h is part of the source hash the
// committed counters of the VIF and ADM kernels are tied to (bench.py, kernel_source_hash).
template <int CTRL>
__device__ __forceinline__ unsigned dpp_add_u32(unsigned v) {
  return v + (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true);
}
__device__ __forceinline__ unsigned long long wave_sum_u32(unsigned v) {
  v = dpp_add_u32<0xb1>(v);    // quad_perm:[1,0,3,2]
  v = dpp_add_u32<0x4e>(v);    // quad_perm:[2,3,0,1]
  v = dpp_add_u32<0x114>(v);   // row_shr:4
  v = dpp_add_u32<0x118>(v);   // row_shr:8   -> lane 15 of each row holds the row sum
  return (unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)v, 15) + (unsigned)__builtin_amdgcn_readlane((int)v, 31) +
         (unsigned)__builtin_amdgcn_readlane((int)v, 47) + (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

__device__ __forceinline__ void prof_lds_add(unsigned long long* p, unsigned long long v) {
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// VB: bytes of one load
template <typename T, int VB>
__global__ __launch_bounds__(kBlock) void line_profiles_kernel(const ProfArgs a) {
  __shared__ unsigned long long tab[2 * kProfStripe];   // [column of the stripe][sum, sum of squares]
  constexpr int V = VB / (int)sizeof(T), NL = kProfLane / V, kWaves = kBlock / 64;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, f = blockIdx.z;
  for (int i = tid; i < 2 * kProfStripe; i += kBlock) tab[i] = 0ull;
  __syncthreads();

  const int x0 = blockIdx.x * kProfStripe, x1 = min(a.w, x0 + kProfStripe);
  const int y0 = blockIdx.y * kProfBand, y1 = min(a.h, y0 + kProfBand);
  const T* plane = (const T*)a.base + (int64_t)f * a.fp;
  unsigned long long* rows = a.out + (int64_t)f * (a.h + a.w) * 2;
  unsigned long long* cols = rows + (int64_t)a.h * 2;

  unsigned cs[kProfLane], cq[kProfLane];
#pragma unroll
  for (int i = 0; i < kProfLane; ++i) cs[i] = cq[i] = 0u;
  const auto widen = [&] {
#pragma unroll
    for (int j = 0; j < NL; ++j)
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const int col = (j * 64 + lane) * V + k;   // < kProfStripe
        prof_lds_add(tab + 2 * col, cs[j * V + k]);
        prof_lds_add(tab + 2 * col + 1, cq[j * V + k]);
        cs[j * V + k] = cq[j * V + k] = 0u;
      }
  };

  int since = 0;   // rows in the uint32 column sums
  for (int y = y0 + wv; y < y1; y += kWaves * kProfRows) {   // wave-uniform
    ProfVec<T, V> v[kProfRows][NL];
#pragma unroll
    for (int r = 0; r < kProfRows; ++r) {
      const int yy = y + kWaves * r;
      const T* row = plane + (int64_t)yy * a.rp;
#pragma unroll
      for (int j = 0; j < NL; ++j) {
        if (yy < y1) v[r][j] = prof_load<T, V>(row, x0 + (j * 64 + lane) * V, x1);
        else v[r][j] = ProfVec<T, V>{};
      }
    }
#pragma unroll
    for (int r = 0; r < kProfRows; ++r) {
      const int yy = y + kWaves * r;
      unsigned s = 0u, q = 0u;
#pragma unroll
      for (int j = 0; j < NL; ++j)
#pragma unroll
        for (int k = 0; k < V; ++k) {
          unsigned val = v[r][j].s[k];
          if constexpr (sizeof(T) > 1) val = min(val, a.top);
          const unsigned sq = val * val;
          s += val;
          q += sq;
          cs[j * V + k] += val;
          cq[j * V + k] += sq;
        }
      const unsigned long long S = wave_sum_u32(s), Q = wave_sum_u32(q);
      if (lane == 0 && yy < y1) {
        atomicAdd(rows + 2 * (int64_t)yy, S);
        atomicAdd(rows + 2 * (int64_t)yy + 1, Q);
      }
    }
    since += kProfRows;
    if (since + kProfRows > a.flush) {
      widen();
      since = 0;
    }
  }
  widen();
  __syncthreads();

  for (int i = tid; i < x1 - x0; i += kBlock) {
    const unsigned long long S = tab[2 * i];
    if (S) {   // a black bar adds nothing
      atomicAdd(cols + 2 * (int64_t)(x0 + i), S);
      atomicAdd(cols + 2 * (int64_t)(x0 + i) + 1, tab[2 * i + 1]);
    }
  }
}

template <typename T, int VB>
hipError_t launch_v(hipStream_t stream, const ProfArgs& a, int n_frames) {
  const dim3 grid((a.w + kProfStripe - 1) / kProfStripe, (a.h + kProfBand - 1) / kProfBand, n_frames);
  hipLaunchKernelGGL((line_profiles_kernel<T, VB>), grid, dim3(kBlock), 0, stream, a);
  return hipGetLastError();
}

template <typename T>
hipError_t launch_t(hipStream_t stream, const ProfArgs& a, int n_frames) {
  constexpr int64_t es = sizeof(T);
  // the widest load every row start is aligned to; a stripe starts a multiple of 16 bytes into its row
  const uint64_t bits = (uint64_t)(uintptr_t)a.base | (uint64_t)(a.rp * es) | (uint64_t)(a.fp * es);
  if (bits % 16 == 0) return launch_v<T, 16>(stream, a, n_frames);
  if (bits % 4 == 0) return launch_v<T, 4>(stream, a, n_frames);
  return launch_v<T, (int)es>(stream, a, n_frames);
}

}  // namespace

size_t profile_out_bytes(int w, int h, int n_frames) {
  return (size_t)(n_frames > 0 ? n_frames : 0) * ((size_t)w + (size_t)h) * 2 * sizeof(unsigned long long);
}

int profile_flush_rows(int bit_depth) {
  const uint64_t top = (1ull << bit_depth) - 1ull;
  return (int)(0xffffffffull / (top * top));
}

hipError_t launch_line_profiles(hipStream_t stream, Elem elem, int bit_depth, const void* base, int64_t row_pitch,
                                int64_t frame_pitch, int n_frames, int w, int h, unsigned long long* out) {
  if (n_frames <= 0) return hipSuccess;
  if (w < 1 || h < 1 || w > 8192 || h > 8192 || (bit_depth != 8 && bit_depth != 10 && bit_depth != 12) ||
      (elem == ELEM_U8) != (bit_depth == 8))
    return hipErrorInvalidValue;
  const hipError_t e = hipMemsetAsync(out, 0, profile_out_bytes(w, h, n_frames), stream);
  if (e != hipSuccess) return e;
  ProfArgs a{};
  a.base = base; a.rp = row_pitch; a.fp = frame_pitch; a.w = w; a.h = h; a.out = out;
  a.top = (1u << bit_depth) - 1u;
  a.flush = profile_flush_rows(bit_depth);   // >= 256 > kProfRows
  if (elem == ELEM_U8) return launch_t<uint8_t>(stream, a, n_frames);
  if (elem == ELEM_U16) return launch_t<uint16_t>(stream, a, n_frames);
  return hipErrorInvalidValue;
}

}  // namespace pqa
