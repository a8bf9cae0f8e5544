// Coding-grid detection: the gradient energy per line of a clip pair (pqa_edge_profiles / pqa_edge_profiles_device; restated
// in tests/edge_ref.py; the solver is pqa2_amd/grid.py).  For the planes R (reference) and D (captured) of w x h samples (a
// sample above top = 2^bits - 1, which a u16 container can hold, is read as top):
//
//   column line x = 1 ... w - 1, the boundary between the columns x - 1 and x:
//     a = R[y][x] - R[y][x-1], b = D[y][x] - D[y][x-1]:   cols[f][x] = (sum_y a^2, sum_y b^2, sum_y a b)
//   row line y = 1 ... h - 1, the boundary between the rows y - 1 and y:
//     a = R[y][x] - R[y-1][x], b = D[y][x] - D[y-1][x]:   rows[f][y] = (sum_x a^2, sum_x b^2, sum_x a b)
//
// line 0 of each axis is zero; words 0 and 1 uint64, word 2 int64 as two's complement; out[f] holds the h row triples, then the
// w column triples.
//
// Work.  A workgroup of 256 threads owns one stripe of kEdgeStripe = 1024 columns and one band of kEdgeBand = 64 rows of one
// frame pair.  Wave wv takes the RUN of kEdgeBand / 4 = 16 consecutive rows wv * 16 ... of the band and keeps the previous row
// of both planes in registers, so a vertical difference costs no load of its own; before its first row it loads the row above
// its run (the row itself at the top of the plane: the differences of row line 0 are then zero).  A lane owns kEdgeLane = 16
// columns of the stripe whatever the load width: with loads of V samples (16 bytes, 4 bytes or one sample, whichever the base
// addresses and pitches of BOTH clips allow -- load_bytes of plane_scan.h; the host decides once per launch) load j of a
// row covers the columns x0 + (64 j + lane) V ... + V - 1, j < 16 / V.  A load that would cross the end of the row is read
// sample by sample and takes zeros past the end, so nothing beyond a row's last sample is touched.  A wave loads kEdgeRows = 2
// rows of both planes before it works on them.
// The sample left of a load's first column comes from the lane below, which holds it as the last sample of its load j (one
// ds_bpermute_b32 for both planes: the two samples travel in one dword); lane 0 has no lane below and reads it from memory,
// column x0 + 64 j V - 1, when that column exists, and takes its own first sample at column 0 of the plane (column line 0 is
// then zero).
// Read amplification: one extra row per run of 16 (17 / 16 of the rows), one extra sample per load group of lane 0 and row
// (16 / V of them per stripe of 1024 columns, 1 / 1024 ... 1 / 64 of the samples); both were read a moment before by the
// neighbouring wave or workgroup.
// Tails need no mask.  The horizontal differences feed only the column sums, the vertical ones only the row sums.  Past the end
// of the row both rows of a vertical difference are zero, so it adds nothing; a horizontal difference at a column >= w lands in
// a column accumulator that is never written out.
// Columns.  The 16 column triples of a lane live in 48 32-bit registers while the wave walks down its run.  They are widened --
// added to the workgroup's 64-bit table in LDS (ds_add_u64; the cross term sign-extended) and cleared -- after at most
//   flush_u = floor((2^32 - 1) / top^2):  66 051 rows at 8 bit, 4 104 at 10 bit, 256 at 12 bit   (sum a^2, sum b^2)
//   flush_s = floor((2^31 - 1) / top^2):  33 025 rows at 8 bit, 2 052 at 10 bit, 128 at 12 bit   (sum a b, |a b| <= top^2)
// rows, which the launcher derives from the bit depth; a wave walks 16 rows, so today one widening at the end of the run is all
// there is.  After a barrier the workgroup adds the non-zero entries of its table to the zeroed output with 64-bit integer
// global atomics: the bands of a stripe meet there.
// Rows.  A lane adds the products of its 16 columns in 32 bits (16 top^2 <= 16 * 4095^2 < 2^29).  The two unsigned sums go
// through the DPP steps of wave_sum_u32 (plane_scan.h): 16 lanes, 256 products, stay below 256 * 4095^2 = 4 292 870 400 < 2^32.
// The signed sum does NOT fit that way (256 * 4095^2 > 2^31): it stops one DPP step earlier, at the sums of 8 lanes,
// 128 * 4095^2 = 2 146 435 200 <= 2^31 - 1 = 2 147 483 647 in magnitude, and the eight of them are read and added in 64 bits.
// One lane adds the triple to the output with 64-bit atomics: the stripes of a row meet there.  Every lane of a wave runs every
// row step: the DPP steps read all 64 lanes.
// Products.  |a|, |b| <= top < 2^12 and a^2, |a b| <= top^2 < 2^24: every product with its addition is one v_mad_i32_i24
// (__mul24 and an add; the squares too); see DESIGN.md section 5 for why not the packed dot products.
// Integer sums do not depend on order: the result is independent of scheduling, base address, pitch and tail.  No floating
// point anywhere.  Output: a line of 8192 samples of +-4095 keeps |sum| <= 2^13 * 4095^2 < 2^37.
#include "plane_scan.h"

namespace pqa {
namespace {

constexpr int kEdgeLane = kEdgeStripe / 64;   // columns of a lane
constexpr int kEdgeRows = 2;                  // rows of both planes a wave loads before it works on them
constexpr int kEdgeRun = kEdgeBand / (kBlock / 64);   // consecutive rows of a wave

struct EdgeArgs : PairPlanes {
  int flush_u, flush_s;
  unsigned top;
  unsigned long long* out;   // [frame][h + w][3], zeroed
};

// VB: bytes of one load
template <typename T, int VB>
__global__ __launch_bounds__(kBlock) void edge_profiles_kernel(const EdgeArgs a) {
  __shared__ unsigned long long tab[kEdgeSums * kEdgeStripe];   // [column of the stripe][sum a^2, sum b^2, sum a b]
  constexpr int V = VB / (int)sizeof(T), NL = kEdgeLane / V;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, f = blockIdx.z;
  for (int i = tid; i < kEdgeSums * kEdgeStripe; i += kBlock) tab[i] = 0ull;
  __syncthreads();

  const int x0 = blockIdx.x * kEdgeStripe, x1 = min(a.w, x0 + kEdgeStripe);
  const int y0 = blockIdx.y * kEdgeBand, y1 = min(a.h, y0 + kEdgeBand);
  const int ya = y0 + wv * kEdgeRun, yb = min(y1, ya + kEdgeRun);   // this wave's run; wave-uniform
  const T* ref = (const T*)a.ref + (int64_t)f * a.ref_fp;
  const T* dis = (const T*)a.dis + (int64_t)f * a.dis_fp;
  unsigned long long* rows = a.out + (int64_t)f * (a.h + a.w) * kEdgeSums;
  unsigned long long* cols = rows + (int64_t)a.h * kEdgeSums;

  unsigned ca[kEdgeLane], cb[kEdgeLane];
  int cx[kEdgeLane];
#pragma unroll
  for (int i = 0; i < kEdgeLane; ++i) {
    ca[i] = cb[i] = 0u;
    cx[i] = 0;
  }
  const auto col_of = [&](int j, int k) { return (j * 64 + lane) * V + k; };   // < kEdgeStripe
  const auto widen_u = [&] {
#pragma unroll
    for (int j = 0; j < NL; ++j)
#pragma unroll
      for (int k = 0; k < V; ++k) {
        lds_add(tab + kEdgeSums * col_of(j, k), ca[j * V + k]);
        lds_add(tab + kEdgeSums * col_of(j, k) + 1, cb[j * V + k]);
        ca[j * V + k] = cb[j * V + k] = 0u;
      }
  };
  const auto widen_s = [&] {
#pragma unroll
    for (int j = 0; j < NL; ++j)
#pragma unroll
      for (int k = 0; k < V; ++k) {
        lds_add(tab + kEdgeSums * col_of(j, k) + 2, (unsigned long long)(long long)cx[j * V + k]);
        cx[j * V + k] = 0;
      }
  };

  SampleVec<T, V> pr[NL], pd[NL];   // the row above the one in work
  if (ya < yb) {
    const int yp = max(ya - 1, 0);
    const T *rrow = ref + (int64_t)yp * a.ref_rp, *drow = dis + (int64_t)yp * a.dis_rp;
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      pr[j] = vec_load<T, V>(rrow, x0 + col_of(j, 0), x1, a.top);
      pd[j] = vec_load<T, V>(drow, x0 + col_of(j, 0), x1, a.top);
    }
  }

  int since_u = 0, since_s = 0;   // rows in the 32-bit column sums
  for (int y = ya; y < yb; y += kEdgeRows) {   // wave-uniform
    SampleVec<T, V> cr[kEdgeRows][NL], cd[kEdgeRows][NL];
    unsigned lr[kEdgeRows][NL], ld[kEdgeRows][NL];   // lane 0: the samples left of its loads
#pragma unroll
    for (int r = 0; r < kEdgeRows; ++r) {
      const int yy = y + r;
      if (yy < yb) {
        const T *rrow = ref + (int64_t)yy * a.ref_rp, *drow = dis + (int64_t)yy * a.dis_rp;
#pragma unroll
        for (int j = 0; j < NL; ++j) {
          cr[r][j] = vec_load<T, V>(rrow, x0 + col_of(j, 0), x1, a.top);
          cd[r][j] = vec_load<T, V>(drow, x0 + col_of(j, 0), x1, a.top);
          const int xg = x0 + j * 64 * V;   // lane 0's first column of load j
          lr[r][j] = ld[r][j] = 0u;
          if (lane == 0 && xg > 0 && xg <= x1) {   // column xg - 1 < x1 <= w exists
            lr[r][j] = min((unsigned)rrow[xg - 1], a.top);
            ld[r][j] = min((unsigned)drow[xg - 1], a.top);
          }
        }
      }
    }
#pragma unroll
    for (int r = 0; r < kEdgeRows; ++r) {
      const int yy = y + r;
      if (yy >= yb) break;   // wave-uniform
      unsigned sa = 0u, sb = 0u;
      int sx = 0;
#pragma unroll
      for (int j = 0; j < NL; ++j) {
        // the last samples of the lane below: both planes in one dword (a sample is below 2^16)
        const unsigned mine = (unsigned)cr[r][j].s[V - 1] | ((unsigned)cd[r][j].s[V - 1] << 16);
        const unsigned below = (unsigned)__shfl_up((int)mine, 1);
        int left_r = (int)(below & 0xffffu), left_d = (int)(below >> 16);
        if (lane == 0) {
          const bool first = x0 + j * 64 * V == 0;   // column 0 of the plane: line 0 is zero
          left_r = first ? (int)cr[r][j].s[0] : (int)lr[r][j];
          left_d = first ? (int)cd[r][j].s[0] : (int)ld[r][j];
        }
#pragma unroll
        for (int k = 0; k < V; ++k) {
          const int R = (int)cr[r][j].s[k], D = (int)cd[r][j].s[k];
          const int ah = R - left_r, bh = D - left_d;               // |.| <= top < 2^12
          const int av = R - (int)pr[j].s[k], bv = D - (int)pd[j].s[k];
          left_r = R;
          left_d = D;
          ca[j * V + k] += (unsigned)__mul24(ah, ah);
          cb[j * V + k] += (unsigned)__mul24(bh, bh);
          cx[j * V + k] += __mul24(ah, bh);
          sa += (unsigned)__mul24(av, av);
          sb += (unsigned)__mul24(bv, bv);
          sx += __mul24(av, bv);
        }
        pr[j] = cr[r][j];
        pd[j] = cd[r][j];
      }
      const unsigned long long A = wave_sum_u32(sa), B = wave_sum_u32(sb);
      const long long X = wave_sum_i32(sx);
      if (lane == 0 && (A | B)) {   // row line 0 and a flat row add nothing
        atomicAdd(rows + kEdgeSums * (int64_t)yy, A);
        atomicAdd(rows + kEdgeSums * (int64_t)yy + 1, B);
        atomicAdd(rows + kEdgeSums * (int64_t)yy + 2, (unsigned long long)X);
      }
      if (++since_u >= a.flush_u) {
        widen_u();
        since_u = 0;
      }
      if (++since_s >= a.flush_s) {
        widen_s();
        since_s = 0;
      }
    }
  }
  widen_u();
  widen_s();
  __syncthreads();

  for (int i = tid; i < x1 - x0; i += kBlock) {
    const unsigned long long A = tab[kEdgeSums * i], B = tab[kEdgeSums * i + 1];
    if (A | B) {   // a flat column adds nothing; a b != 0 needs a != 0 and b != 0
      atomicAdd(cols + kEdgeSums * (int64_t)(x0 + i), A);
      atomicAdd(cols + kEdgeSums * (int64_t)(x0 + i) + 1, B);
      atomicAdd(cols + kEdgeSums * (int64_t)(x0 + i) + 2, tab[kEdgeSums * i + 2]);
    }
  }
}

template <typename T, int VB>
hipError_t launch_v(hipStream_t stream, const EdgeArgs& a, int n_frames) {
  const dim3 grid((a.w + kEdgeStripe - 1) / kEdgeStripe, (a.h + kEdgeBand - 1) / kEdgeBand, n_frames);
  hipLaunchKernelGGL((edge_profiles_kernel<T, VB>), grid, dim3(kBlock), 0, stream, a);
  return hipGetLastError();
}

}  // namespace

size_t edge_out_bytes(int w, int h, int n_frames) {
  return (size_t)(n_frames > 0 ? n_frames : 0) * ((size_t)w + (size_t)h) * kEdgeSums * sizeof(unsigned long long);
}

int edge_flush_rows(int bit_depth, bool is_signed) {
  const uint64_t top = (1ull << bit_depth) - 1ull;
  return (int)((is_signed ? 0x7fffffffull : 0xffffffffull) / (top * top));
}

hipError_t launch_edge_profiles(hipStream_t stream, Elem elem, int bits, const void* ref, int64_t ref_row_pitch,
                                int64_t ref_frame_pitch, const void* dis, int64_t dis_row_pitch, int64_t dis_frame_pitch,
                                int n_frames, int w, int h, unsigned long long* out) {
  if (n_frames <= 0) return hipSuccess;
  EdgeArgs a{};
  if (!pair_planes(a, elem, bits, ref, ref_row_pitch, ref_frame_pitch, dis, dis_row_pitch, dis_frame_pitch, w, h))
    return hipErrorInvalidValue;
  const hipError_t e = hipMemsetAsync(out, 0, edge_out_bytes(w, h, n_frames), stream);
  if (e != hipSuccess) return e;
  a.out = out;
  a.top = (1u << bits) - 1u;
  a.flush_u = edge_flush_rows(bits, false);   // >= 256
  a.flush_s = edge_flush_rows(bits, true);    // >= 128
  // a stripe starts a multiple of 16 bytes into its row
  return dispatch(elem, load_bytes(elem, a),
                  [&](auto t, auto vb) { return launch_v<decltype(t), decltype(vb)::value>(stream, a, n_frames); });
}

}  // namespace pqa
