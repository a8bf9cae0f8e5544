// Level alignment: the per-level transfer table of frame pairs (pqa_level_stats / pqa_level_stats_device; restated in
// tests/level_ref.py).  For one plane of w x h samples and every reference level v in 0 ... L - 1, L = 2^bit_depth:
//
//   T[f][v][0] = number of pixels with ref == v     T[f][v][1] = sum of dis over them     T[f][v][2] = sum of dis^2 over them
//
// exact uint64.  A reference sample above L - 1 (a u16 container can hold one) is counted in bin L - 1; its captured partner
// enters the sums as it is, so a captured sample may be anything up to 65535 and the bounds below are stated for that.
//
// Work.  A workgroup of 256 threads owns a span of at most kLevelSpan samples: `rows` whole rows of one column segment (a
// segment is at most kLevelSeg samples wide, so rows >= 1 always fits).  Wave wv takes the rows wv, wv + 4, ... of the span,
// a lane one load (16 bytes, 4 bytes or one sample, whichever the addresses and pitches of BOTH planes allow; the host
// decides once per launch) out of every 64 along the row.  A load that would cross the end of the row is read sample by
// sample, so nothing beyond x1 is touched; a row pitch larger than the row and an odd base address only select the load width.
// Table.  LDS holds two uint64 words per level: A[v] = count << 32 | sum d, and B[v] = sum d^2, updated with 64-bit integer
// LDS atomics (ds_add_u64, no return) and merged into the zeroed output with 64-bit integer global atomics, non-empty
// levels only.  Integer sums do not depend on order: the result is independent of scheduling, base address, pitch and tail.
// No floating point anywhere.  LDS: 16 L bytes = 4 KiB / 16 KiB / 64 KiB at 8 / 10 / 12 bit; at 12 bit two workgroups (8
// waves) fit a CU's 160 KiB, which the atomic-bound loop does not need more of.
// Accumulator bounds.  A span has n <= kLevelSpan = 32768 samples, d <= 65535:
//   low half of A: sum d <= 32768 * 65535 < 2^31  -- never carries into the count in the high half (count <= 2^15);
//   B: d^2 < 2^32 a sample, 64 bit;   a lane's run (below): count and sum d as above in u32, sum d^2 in u64.
//   Output: 64-bit; a 2^31-sample plane of 65535 stays below 2^63.
// Contention.  Flat content sends every lane to one LDS address.  A lane therefore keeps the RUN of equal reference level it
// is in (level, count, sum d, sum d^2) in registers, across its loads and rows, and touches LDS only when the level changes
// and once at the end of the span; at the end a wave whose lanes all hold the same level adds them up with shuffles and one
// lane updates LDS.  A flat span costs one update a wave; 64-pixel runs at 8 bit cost one update per lane and load (16
// samples) instead of 16; noise costs one update per sample, on mostly different addresses.
#include <climits>

#include "plane_scan.h"

namespace pqa {
namespace {

constexpr int kLevelSpan = 32768;   // samples of one workgroup: the bound the u32 accumulators rest on
constexpr int kLevelSeg = 16384;    // widest column segment, a multiple of every load width

struct LevelArgs : PairPlanes {
  int L, segs, rows;
  unsigned long long* out;   // [frame][L][3], zeroed
};

struct Run {
  unsigned key = 0, cnt = 0, sd = 0;
  unsigned long long sd2 = 0;
};

__device__ __forceinline__ void run_flush(unsigned long long* tab, int L, const Run& r) {
  lds_add(tab + r.key, ((unsigned long long)r.cnt << 32) | r.sd);
  lds_add(tab + L + r.key, r.sd2);
}

__device__ __forceinline__ void run_step(unsigned long long* tab, int L, Run& r, unsigned ref, unsigned dis) {
  const unsigned b = ref < (unsigned)L ? ref : (unsigned)L - 1u;
  if (b != r.key) {
    if (r.cnt) run_flush(tab, L, r);
    r.key = b; r.cnt = 0; r.sd = 0; r.sd2 = 0;
  }
  r.cnt += 1u;
  r.sd += dis;
  r.sd2 += dis * dis;   // <= 65535^2 < 2^32
}

// VB: bytes of one load
template <typename T, int VB>
__global__ __launch_bounds__(kBlock) void level_stats_kernel(const LevelArgs a) {
  extern __shared__ unsigned long long tab[];   // A[L], B[L]
  constexpr int V = VB / (int)sizeof(T);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, L = a.L;
  for (int i = tid; i < 2 * L; i += kBlock) tab[i] = 0ull;
  __syncthreads();

  const int f = blockIdx.y, seg = blockIdx.x % a.segs, rb = blockIdx.x / a.segs;
  const int x0 = seg * kLevelSeg, x1 = min(a.w, x0 + kLevelSeg);
  const int y0 = rb * a.rows, y1 = min(a.h, y0 + a.rows);
  const T* pr = (const T*)a.ref + (int64_t)f * a.ref_fp;
  const T* pd = (const T*)a.dis + (int64_t)f * a.dis_fp;

  Run run;
  for (int y = y0 + wv; y < y1; y += kBlock / 64) {
    const T* rr = pr + (int64_t)y * a.ref_rp;
    const T* dd = pd + (int64_t)y * a.dis_rp;
    for (int x = x0 + lane * V; x < x1; x += 64 * V) {
      if constexpr (V == 1) {
        run_step(tab, L, run, rr[x], dd[x]);
      } else {
        if (x + V <= x1) {
          using Vec = SampleVec<T, V>;
          const Vec vr = *reinterpret_cast<const Vec*>(rr + x), vd = *reinterpret_cast<const Vec*>(dd + x);
#pragma unroll
          for (int k = 0; k < V; ++k) run_step(tab, L, run, vr.s[k], vd.s[k]);
        } else {
          for (int k = 0; x + k < x1; ++k) run_step(tab, L, run, rr[x + k], dd[x + k]);
        }
      }
    }
  }

  // the runs still open: one update a wave when its lanes agree (every lane of the wave arrives here)
  const bool has = run.cnt != 0u;
  const unsigned long long holders = __ballot(has);
  if (holders) {
    const unsigned k0 = (unsigned)__shfl((int)run.key, __ffsll((long long)holders) - 1, 64);
    if (__all(!has || run.key == k0)) {
      unsigned cnt = has ? run.cnt : 0u, sd = has ? run.sd : 0u;   // a wave's sums obey the span's bounds
      unsigned long long sd2 = has ? run.sd2 : 0ull;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        cnt += __shfl_down(cnt, off, 64);
        sd += __shfl_down(sd, off, 64);
        sd2 += __shfl_down(sd2, off, 64);
      }
      if (lane == 0) {
        Run t;
        t.key = k0; t.cnt = cnt; t.sd = sd; t.sd2 = sd2;
        run_flush(tab, L, t);
      }
    } else if (has) {
      run_flush(tab, L, run);
    }
  }
  __syncthreads();

  unsigned long long* out = a.out + (int64_t)f * L * 3;
  for (int v = tid; v < L; v += kBlock) {
    const unsigned long long A = tab[v];
    if (A) {
      atomicAdd(out + 3 * v, A >> 32);
      atomicAdd(out + 3 * v + 1, A & 0xffffffffull);
      atomicAdd(out + 3 * v + 2, tab[L + v]);
    }
  }
}

template <typename T, int VB>
hipError_t launch_v(hipStream_t stream, const LevelArgs& a, int n_frames) {
  const int row_blocks = (a.h + a.rows - 1) / a.rows;
  const size_t lds = (size_t)2 * a.L * sizeof(unsigned long long);
  if (lds >= 65536) {   // the 12-bit table is the whole default allowance of dynamic LDS: ask for it
    const hipError_t e = hipFuncSetAttribute((const void*)level_stats_kernel<T, VB>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL((level_stats_kernel<T, VB>), dim3(a.segs * row_blocks, n_frames), dim3(kBlock), lds, stream, a);
  return hipGetLastError();
}

}  // namespace

size_t level_out_bytes(int bit_depth, int n_frames) {
  return (size_t)(n_frames > 0 ? n_frames : 0) * ((size_t)3 << bit_depth) * sizeof(unsigned long long);
}

hipError_t launch_level_stats(hipStream_t stream, Elem elem, int bit_depth, const void* ref, int64_t ref_row_pitch,
                              int64_t ref_frame_pitch, const void* dis, int64_t dis_row_pitch, int64_t dis_frame_pitch,
                              int n_frames, int w, int h, unsigned long long* out) {
  if (n_frames <= 0) return hipSuccess;
  LevelArgs a{};
  // no bound on w and h here: a column segment and a span bound what a workgroup sees
  if (!pair_planes(a, elem, bit_depth, ref, ref_row_pitch, ref_frame_pitch, dis, dis_row_pitch, dis_frame_pitch, w, h, INT_MAX))
    return hipErrorInvalidValue;
  const hipError_t e = hipMemsetAsync(out, 0, level_out_bytes(bit_depth, n_frames), stream);
  if (e != hipSuccess) return e;
  a.L = 1 << bit_depth; a.out = out;
  a.segs = (w + kLevelSeg - 1) / kLevelSeg;
  const int seg_w = w < kLevelSeg ? w : kLevelSeg;
  // rows * seg_w <= kLevelSpan samples a workgroup; a quarter of that at 8 bit, where the 256-level table costs little to
  // merge and more workgroups fill the chip on a single frame
  a.rows = (bit_depth == 8 ? kLevelSpan / 4 : kLevelSpan) / seg_w;
  if (a.rows < 1) a.rows = 1;   // seg_w <= kLevelSeg <= kLevelSpan: one row never exceeds the span
  // a segment starts a multiple of 16 bytes into its row
  return dispatch(elem, load_bytes(elem, a),
                  [&](auto t, auto vb) { return launch_v<decltype(t), decltype(vb)::value>(stream, a, n_frames); });
}

}  // namespace pqa
