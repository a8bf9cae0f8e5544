// Capture-integrity reductions (PQA_FEAT_INTEGRITY): what FFmpeg's freezedetect, blackdetect and scdet filters reduce a
// frame to before their host state machines run (libavfilter/vf_freezedetect.c, vf_blackdetect.c, vf_scdet.c,
// scene_sad.c; restated in tests/integrity_ref.py, state machines in pqa2_amd/integrity.py).
//
// Per frame and plane: SAD = sum |cur - prev| over the whole plane, where prev is the frame before it (the per-frame
// record) or one fixed anchor frame (pqa_frame_sad); for the luma plane also the number of samples <= black_threshold.
// Everything is exact unsigned 64-bit integer arithmetic: per-workgroup partials, then a fixed-order second stage; no
// floating point and no atomics, so a row does not depend on the batch it was computed in.
//
// A pure streaming reduction: one wave walks one row at a time with 16-byte loads of both frames (v_sad_u8 / v_sad_u16 on
// the packed samples), ~20 VGPRs, so eight waves per SIMD keep the loads in flight.  A wave per row (not a workgroup per
// row) keeps 60 of 64 lanes busy on the 960-byte chroma rows of 1080p, where a 256-lane sweep would idle three waves.
// Rows or bases that are not 16-byte aligned (odd pitches, sub-rectangles) take the per-sample path.
#include "kernels.h"
#include "pqa_device.h"

namespace pqa {
namespace {

struct IntegrityArgs {
  const void* cur[3];           // frame 0 of the run, per plane
  int64_t row_pitch[3], frame_pitch[3];   // elements
  const void* prev0[3];         // the frame in front of the run (nullable: no SAD for frame 0), or the anchor
  int64_t prev0_pitch[3];       // elements
  int w[3], h[3];
  int anchor;                   // != 0: every frame is compared with prev0 instead of its predecessor
  unsigned black_threshold;
  unsigned long long* partials; // [n_frames][3][kIntegrityBlocks][2] {sad, black count}
};

__device__ __forceinline__ unsigned count_le4(unsigned x, unsigned thr) {
  unsigned c = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) c += ((x >> (8 * i)) & 0xffu) <= thr ? 1u : 0u;
  return c;
}

// rows y = first, first + step, ... of one plane pair, one wave per row; SAD is skipped when pb is null
template <typename T, bool BLACK, bool SAD>
__device__ __forceinline__ void integrity_rows(const T* __restrict__ pa, int64_t pitch_a, const T* __restrict__ pb,
                                               int64_t pitch_b, int w, int h, int first, int step, int lane, unsigned thr,
                                               unsigned long long& sad, unsigned long long& black) {
  constexpr int VEC = 16 / sizeof(T);
  const bool aligned = ((pitch_a * sizeof(T)) % 16 == 0) && ((uintptr_t)pa % 16 == 0) &&
                       (!SAD || (((pitch_b * sizeof(T)) % 16 == 0) && ((uintptr_t)pb % 16 == 0)));
  const int wv = aligned ? w / VEC : 0;   // 16-byte vectors per row
  for (int y = first; y < h; y += step) {
    const T* ra = pa + (int64_t)y * pitch_a;
    const T* rb = SAD ? pb + (int64_t)y * pitch_b : nullptr;
    unsigned rs = 0, rc = 0;   // per row and lane: at most 16384 / 64 * 16 samples of 16 bits, far below 2^32
    for (int v = lane; v < wv; v += 64) {
      const uint4 x = reinterpret_cast<const uint4*>(ra)[v];
      const unsigned xs[4] = {x.x, x.y, x.z, x.w};
      if constexpr (SAD) {
        const uint4 z = reinterpret_cast<const uint4*>(rb)[v];
        const unsigned zs[4] = {z.x, z.y, z.z, z.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if constexpr (sizeof(T) == 1) rs = __builtin_amdgcn_sad_u8(xs[i], zs[i], rs);
          else rs = __builtin_amdgcn_sad_u16(xs[i], zs[i], rs);
        }
      }
      if constexpr (BLACK) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if constexpr (sizeof(T) == 1) rc += count_le4(xs[i], thr);
          else rc += ((xs[i] & 0xffffu) <= thr ? 1u : 0u) + ((xs[i] >> 16) <= thr ? 1u : 0u);
        }
      }
    }
    for (int x = wv * VEC + lane; x < w; x += 64) {
      const unsigned p = ra[x];
      if constexpr (SAD) {
        const unsigned q = rb[x];
        rs += p > q ? p - q : q - p;
      }
      if constexpr (BLACK) rc += p <= thr ? 1u : 0u;
    }
    sad += rs;
    black += rc;
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void integrity_kernel(const IntegrityArgs a) {
  __shared__ unsigned long long red[8];
  const int fr = blockIdx.y, p = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63;
  const T* pa = (const T*)a.cur[p] + (int64_t)fr * a.frame_pitch[p];
  const T* pb;
  int64_t pitch_b;
  if (a.anchor || fr == 0) {
    pb = (const T*)a.prev0[p];
    pitch_b = a.prev0_pitch[p];
  } else {
    pb = pa - a.frame_pitch[p];
    pitch_b = a.row_pitch[p];
  }
  const int first = blockIdx.x * (kBlock / 64) + (tid >> 6), step = gridDim.x * (kBlock / 64);
  unsigned long long sad = 0, black = 0;
  if (p == 0) {
    if (pb) integrity_rows<T, true, true>(pa, a.row_pitch[p], pb, pitch_b, a.w[p], a.h[p], first, step, lane, a.black_threshold, sad, black);
    else integrity_rows<T, true, false>(pa, a.row_pitch[p], pb, pitch_b, a.w[p], a.h[p], first, step, lane, a.black_threshold, sad, black);
  } else if (pb) {
    integrity_rows<T, false, true>(pa, a.row_pitch[p], pb, pitch_b, a.w[p], a.h[p], first, step, lane, 0u, sad, black);
  }
  unsigned long long v[2] = {sad, black};
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[i] += __shfl_down(v[i], off, 64);
    if (lane == 0) red[(tid >> 6) * 2 + i] = v[i];
  }
  __syncthreads();
  if (tid < 2)
    a.partials[(((int64_t)fr * 3 + p) * gridDim.x + blockIdx.x) * 2 + tid] = (red[tid] + red[2 + tid]) + (red[4 + tid] + red[6 + tid]);
}

// Second stage, one workgroup per frame: wave p sums plane p's partials in a fixed order.  ext5 (nullable): SAD of plane p
// into slot p (NaN when no_prev0 and this is frame 0, or p >= n_planes), the black count into slot 3, NaN into slots 4..7
// of ring row (slot_base + f) % capacity.  out (nullable): [n_frames][3] uint64 SADs (0 for p >= n_planes).
__global__ __launch_bounds__(kBlock) void integrity_finalize(const unsigned long long* partials, int n_blocks, int n_planes,
                                                              int no_prev0, double* ext5, int ext_stride, int slot_base,
                                                              int capacity, unsigned long long* out) {
  const int fr = blockIdx.x, tid = threadIdx.x, lane = tid & 63, p = tid >> 6;
  unsigned long long v[2] = {0, 0};
  if (p < n_planes)
    for (int b = lane; b < n_blocks; b += 64) {
      v[0] += partials[(((int64_t)fr * 3 + p) * n_blocks + b) * 2];
      v[1] += partials[(((int64_t)fr * 3 + p) * n_blocks + b) * 2 + 1];
    }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[i] += __shfl_down(v[i], off, 64);
  if (lane != 0) return;
  const double nan = __builtin_nan("");
  if (out && p < 3) out[(int64_t)fr * 3 + p] = p < n_planes ? v[0] : 0ull;
  if (!ext5) return;
  double* row = ext5 + (int64_t)((slot_base + fr) % capacity) * ext_stride;
  if (p < 3) {
    row[p] = (p < n_planes && !(no_prev0 && fr == 0)) ? (double)v[0] : nan;   // exact: below 2^53
    if (p == 0) row[3] = (double)v[1];
  } else {
    for (int s = 4; s < ext_stride; ++s) row[s] = nan;
  }
}

}  // namespace

hipError_t launch_integrity(hipStream_t stream, Elem elem, const PlaneRun cur[3], const void* const prev0[3],
                            const int64_t prev0_pitch[3], const int pw[3], const int ph[3], int n_planes, int n_frames,
                            bool anchor, unsigned black_threshold, unsigned long long* partials, double* ext5,
                            int ext_stride, int slot_base, int capacity, unsigned long long* out) {
  if (n_frames <= 0) return hipSuccess;
  if (n_planes < 1 || n_planes > 3) return hipErrorInvalidValue;
  IntegrityArgs a{};
  for (int p = 0; p < n_planes; ++p) {
    a.cur[p] = cur[p].base; a.row_pitch[p] = cur[p].row_pitch; a.frame_pitch[p] = cur[p].frame_pitch;
    a.prev0[p] = prev0[p]; a.prev0_pitch[p] = prev0_pitch[p];
    a.w[p] = pw[p]; a.h[p] = ph[p];
  }
  if (anchor)
    for (int p = 0; p < n_planes; ++p)
      if (!prev0[p]) return hipErrorInvalidValue;
  a.anchor = anchor ? 1 : 0;
  a.black_threshold = black_threshold;
  a.partials = partials;
  const dim3 grid(kIntegrityBlocks, n_frames, n_planes), block(kBlock);
  switch (elem) {
    case ELEM_U8: hipLaunchKernelGGL((integrity_kernel<uint8_t>), grid, block, 0, stream, a); break;
    case ELEM_U16: hipLaunchKernelGGL((integrity_kernel<uint16_t>), grid, block, 0, stream, a); break;
    default: return hipErrorInvalidValue;
  }
  hipLaunchKernelGGL(integrity_finalize, dim3(n_frames), dim3(kBlock), 0, stream, partials, kIntegrityBlocks, n_planes,
                     (!anchor && !prev0[0]) ? 1 : 0, ext5, ext_stride, slot_base, capacity, out);
  return hipGetLastError();
}

}  // namespace pqa
