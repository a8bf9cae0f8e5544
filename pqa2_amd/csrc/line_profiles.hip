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
// the lanes with the DPP steps of pqa_device.h's wave sum (wave_sum_u32 of plane_scan.h: the sums of 16 lanes, 256 samples, stay below 256 * 4095^2
// = 4 292 870 400 < 2^32; the four of them are added in 64 bits), and one lane adds the pair to the output with 64-bit
// atomics: the stripes of a row meet there.  Every lane of a wave runs every row step: the DPP steps read all 64 lanes.
// Integer sums do not depend on order: the result is independent of scheduling, base address, pitch and tail.  No floating
// point anywhere.  Output: a plane of 8192 x 8192 samples of 4095 keeps a line's squares below 2^13 * 2^24 = 2^37.
#include "plane_scan.h"

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
        lds_add(tab + 2 * col, cs[j * V + k]);
        lds_add(tab + 2 * col + 1, cq[j * V + k]);
        cs[j * V + k] = cq[j * V + k] = 0u;
      }
  };

  int since = 0;   // rows in the uint32 column sums
  for (int y = y0 + wv; y < y1; y += kWaves * kProfRows) {   // wave-uniform
    SampleVec<T, V> v[kProfRows][NL];
#pragma unroll
    for (int r = 0; r < kProfRows; ++r) {
      const int yy = y + kWaves * r;
      const T* row = plane + (int64_t)yy * a.rp;
#pragma unroll
      for (int j = 0; j < NL; ++j) {
        if (yy < y1) v[r][j] = vec_load<T, V>(row, x0 + (j * 64 + lane) * V, x1);
        else v[r][j] = SampleVec<T, V>{};
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
  if (!scan_shape_ok(elem, bit_depth, w, h)) return hipErrorInvalidValue;
  const hipError_t e = hipMemsetAsync(out, 0, profile_out_bytes(w, h, n_frames), stream);
  if (e != hipSuccess) return e;
  ProfArgs a{};
  a.base = base; a.rp = row_pitch; a.fp = frame_pitch; a.w = w; a.h = h; a.out = out;
  a.top = (1u << bit_depth) - 1u;
  a.flush = profile_flush_rows(bit_depth);   // >= 256 > kProfRows
  // a stripe starts a multiple of 16 bytes into its row
  return dispatch(elem, load_bytes(elem, base, row_pitch, frame_pitch),
                  [&](auto t, auto vb) { return launch_v<decltype(t), decltype(vb)::value>(stream, a, n_frames); });
}

}  // namespace pqa
