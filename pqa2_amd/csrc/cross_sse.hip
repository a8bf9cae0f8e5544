// Temporal alignment: banded cross-frame SSE (pqa_cross_sse / pqa_cross_sse_device; restated in tests/align_ref.py).
//
//   D[i][c] = sum over luma pixels of (ref_i - dis_{i+k})^2,  k = k_lo + c,  UINT64_MAX where i + k is outside the clip.
//
// 8-bit clips, matrix cores.  With x' = x ^ 0x80 read as i8 (x - 128), sum (r - d)^2 = sum r'^2 + sum d'^2 - 2 sum r'd', and
// sum r'd' of 32 reference frames x 32 captured frames over a run of pixels is a chain of v_mfma_i32_32x32x32_i8: lane l
// supplies 16 consecutive pixels of frame l & 31 (A: reference, B: captured), the two lane halves two different 16-pixel
// runs.  The order of k inside an MFMA is irrelevant to a Gram sum as long as the A and B lanes of one MFMA hold the same
// pixels, which they do by construction (both sides use the same (segment, lane half, q) -> pixel rule).  A 128-pixel
// segment of one row is 4 MFMAs: lane half h of MFMA q holds pixels 64 h + 16 q ... + 15, so a lane reads 64 contiguous bytes.
// Reference tile b (frames 32 b ... 32 b + 31) meets the captured tiles that start at 32 b + k_lo + 32 t, t < ceil((31 +
// span) / 32): only frames the band touches.  Row tails, frames outside the clip and partial tiles are zero in the centred
// domain (the operand words are zeroed, not the raw bytes).
// Overflow: |r'd'| <= 2^14, a wave accumulates kXsseSegsPerWave * 128 = 8192 pixels in i32 (< 2^27), the four waves of a
// workgroup are added in i32 (< 2^29), everything after that is 64-bit.  Partials are summed in a fixed order, no atomics.
//
// 10- / 12-bit clips, and 8-bit with PQA_XSSE_MFMA=0: plain integer VALU, (r - d)^2 summed directly in uint64 per (frame,
// offset, row group), the same fixed-order second stage.  Same entry point, same integers.
//
// Addressing: frame f of a clip lives at base + (f % ring) * frame_pitch.  A device-resident clip has ring >= n; the host
// entry keeps one reference tile (ring 32) and a window of captured frames (ring >= 31 + span) on the device.
#include "kernels.h"
#include "pqa_device.h"

namespace pqa {
namespace {

using v4i = __attribute__((ext_vector_type(4))) int;
using v16i = __attribute__((ext_vector_type(16))) int;

constexpr int kSegPixels = 128;        // pixels of one row a wave feeds to 4 MFMAs
constexpr int kWavesPerBlock = 4;

// 16 centred samples of a row starting at x (zero beyond w or when the frame does not exist)
template <bool ALIGNED>
__device__ __forceinline__ v4i load_centred16(const uint8_t* __restrict__ row, int x, int w) {
  v4i v = {0, 0, 0, 0};
  if (!row || x >= w) return v;
  if (ALIGNED && x + 16 <= w) {
    v = *reinterpret_cast<const v4i*>(row + x);
    return v ^ (int)0x80808080;
  }
  const int n = w - x;   // >= 1; samples beyond it stay zero in the centred domain
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    unsigned wd = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b)
      if (4 * q + b < n) wd |= (unsigned)(row[x + 4 * q + b] ^ 0x80u) << (8 * b);
    v[q] = (int)wd;
  }
  return v;
}

struct XsseMfmaArgs {
  XsseClip ref, dis;
  int w, h, k_lo, k_hi, tile0, ntd, segs_per_row, n_segs;
  int* part;   // [pair][blocks][32 rows (reference)][32 cols (captured)]
};

template <bool ALIGNED>
__global__ __launch_bounds__(kWavesPerBlock * 64) void xsse_mfma_kernel(const XsseMfmaArgs a) {
  __shared__ int red[kWavesPerBlock][1024];
  const int pair = blockIdx.x, blk = blockIdx.y;
  const int tile = a.tile0 + pair / a.ntd, t = pair % a.ntd;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, f = lane & 31, hh = lane >> 5;
  const int64_t i = (int64_t)tile * 32 + f;
  const int64_t j = (int64_t)tile * 32 + a.k_lo + 32 * t + f;
  const uint8_t* pr = i < a.ref.n ? (const uint8_t*)a.ref.base + (i % a.ref.ring) * a.ref.frame_pitch : nullptr;
  // captured frames beyond the band of this reference tile (the tail of its last captured tile) are not read at all
  const uint8_t* pd = (j >= 0 && j < a.dis.n && j <= (int64_t)tile * 32 + 31 + a.k_hi) ? (const uint8_t*)a.dis.base + (j % a.dis.ring) * a.dis.frame_pitch : nullptr;
  v16i acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0;
  const int s0 = (blk * kWavesPerBlock + wv) * kXsseSegsPerWave;
  const int s1 = s0 + kXsseSegsPerWave < a.n_segs ? s0 + kXsseSegsPerWave : a.n_segs;
  for (int s = s0; s < s1; ++s) {   // wave-uniform trip count: every lane executes every MFMA
    const int y = s / a.segs_per_row;
    const int x0 = (s - y * a.segs_per_row) * kSegPixels + 64 * hh;
    const uint8_t* rr = pr ? pr + (int64_t)y * a.ref.row_pitch : nullptr;
    const uint8_t* rd = pd ? pd + (int64_t)y * a.dis.row_pitch : nullptr;
    v4i A[4], B[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      A[q] = load_centred16<ALIGNED>(rr, x0 + 16 * q, a.w);
      B[q] = load_centred16<ALIGNED>(rd, x0 + 16 * q, a.w);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(A[q], B[q], acc, 0, 0, 0);
  }
  // C/D map of the 32 x 32 shapes: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
  for (int r = 0; r < 16; ++r) red[wv][((r & 3) + 8 * (r >> 2) + 4 * hh) * 32 + f] = acc[r];
  __syncthreads();
  int* out = a.part + ((int64_t)pair * gridDim.y + blk) * 1024;
#pragma unroll
  for (int m = 0; m < 1024 / (kWavesPerBlock * 64); ++m) {
    const int e = tid + m * kWavesPerBlock * 64;
    out[e] = (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]);
  }
}

// sum of x'^2 of `count` frames starting at frame `first`: norm_part[(first + f) * kXsseNormBlocks + block]
template <bool ALIGNED>
__global__ __launch_bounds__(kBlock) void xsse_norm_kernel(const XsseClip clip, int64_t first, int w, int h,
                                                          unsigned long long* __restrict__ norm_part) {
  __shared__ unsigned long long red[kBlock / 64];
  const int64_t fr = first + blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63;
  const uint8_t* p = (const uint8_t*)clip.base + (fr % clip.ring) * clip.frame_pitch;
  const int wv = ALIGNED ? w / 16 : 0;
  unsigned long long sum = 0;
  for (int y = blockIdx.x; y < h; y += gridDim.x) {
    const uint8_t* row = p + (int64_t)y * clip.row_pitch;
    int rs = 0;   // per row and lane: at most 16384 / 256 * 2^14 = 2^20
    for (int v = tid; v < wv; v += kBlock) {
      const v4i x = *reinterpret_cast<const v4i*>(row + 16 * v) ^ (int)0x80808080;
#pragma unroll
      for (int q = 0; q < 4; ++q) rs = __builtin_amdgcn_sdot4(x[q], x[q], rs, false);
    }
    for (int x = wv * 16 + tid; x < w; x += kBlock) {
      const int c = (int)row[x] - 128;
      rs += c * c;
    }
    sum += (unsigned long long)rs;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
  if (lane == 0) red[tid >> 6] = sum;
  __syncthreads();
  if (tid == 0) {
    unsigned long long s = 0;
    for (int i = 0; i < kBlock / 64; ++i) s += red[i];
    norm_part[fr * kXsseNormBlocks + blockIdx.x] = s;
  }
}

// second stage of the MFMA path, one workgroup per tile pair: D = sum r'^2 + sum d'^2 - 2 sum r'd'
__global__ __launch_bounds__(kBlock) void xsse_mfma_combine(const int* __restrict__ part, int n_blocks, int tile0, int ntd,
                                                            int k_lo, int span, int64_t n_ref, int64_t n_dis,
                                                            const unsigned long long* __restrict__ norm_ref,
                                                            const unsigned long long* __restrict__ norm_dis,
                                                            unsigned long long* __restrict__ out) {
  const int pair = blockIdx.x, tile = tile0 + pair / ntd, t = pair % ntd;
  for (int e = threadIdx.x; e < 1024; e += kBlock) {
    const int row = e >> 5, col = e & 31;
    const int c = 32 * t + col - row;
    const int64_t i = (int64_t)tile * 32 + row;
    if (c < 0 || c >= span || i >= n_ref) continue;
    const int64_t j = i + k_lo + c;
    unsigned long long d = ~0ull;
    if (j >= 0 && j < n_dis) {
      long long g = 0;
      for (int b = 0; b < n_blocks; ++b) g += part[((int64_t)pair * n_blocks + b) * 1024 + e];
      unsigned long long s = 0;
      for (int b = 0; b < kXsseNormBlocks; ++b) s += norm_ref[i * kXsseNormBlocks + b];
      for (int b = 0; b < kXsseNormBlocks; ++b) s += norm_dis[j * kXsseNormBlocks + b];
      d = (unsigned long long)((long long)s - 2 * g);
    }
    out[i * span + c] = d;
  }
}

// ---- plain VALU path ------------------------------------------------------------------------------------------------------
struct XsseValuArgs {
  XsseClip ref, dis;
  int w, h, k_lo, span, tile0;
  unsigned long long* part;   // [frame of the launch][span][kXsseValuBlocks]
};

template <typename T, bool ALIGNED>
__global__ __launch_bounds__(kBlock) void xsse_valu_kernel(const XsseValuArgs a) {
  __shared__ unsigned long long red[kBlock / 64];
  const int64_t i = (int64_t)a.tile0 * 32 + blockIdx.y;
  if (i >= a.ref.n) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const T* pr = (const T*)a.ref.base + (i % a.ref.ring) * a.ref.frame_pitch;
  const int wq = ALIGNED ? a.w / 4 : 0;   // groups of four samples
  for (int c = 0; c < a.span; ++c) {
    const int64_t j = i + a.k_lo + c;
    if (j < 0 || j >= a.dis.n) continue;   // uniform over the workgroup
    const T* pd = (const T*)a.dis.base + (j % a.dis.ring) * a.dis.frame_pitch;
    unsigned long long sum = 0;
    for (int y = blockIdx.x; y < a.h; y += gridDim.x) {
      const T* rr = pr + (int64_t)y * a.ref.row_pitch;
      const T* rd = pd + (int64_t)y * a.dis.row_pitch;
      for (int v = tid; v < wq; v += kBlock) {
        unsigned rs = 0;   // four squares of at most 4095^2
        if constexpr (sizeof(T) == 1) {
          const unsigned x = reinterpret_cast<const unsigned*>(rr)[v], z = reinterpret_cast<const unsigned*>(rd)[v];
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            const int d = (int)((x >> (8 * b)) & 0xffu) - (int)((z >> (8 * b)) & 0xffu);
            rs += (unsigned)(d * d);
          }
        } else {
          const uint2 x = reinterpret_cast<const uint2*>(rr)[v], z = reinterpret_cast<const uint2*>(rd)[v];
          const unsigned xs[2] = {x.x, x.y}, zs[2] = {z.x, z.y};
#pragma unroll
          for (int b = 0; b < 2; ++b) {
            const int d0 = (int)(xs[b] & 0xffffu) - (int)(zs[b] & 0xffffu), d1 = (int)(xs[b] >> 16) - (int)(zs[b] >> 16);
            rs += (unsigned)(d0 * d0) + (unsigned)(d1 * d1);
          }
        }
        sum += rs;
      }
      for (int x = wq * 4 + tid; x < a.w; x += kBlock) {
        const int d = (int)rr[x] - (int)rd[x];
        sum += (unsigned)(d * d);
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
    if (lane == 0) red[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) {
      unsigned long long s = 0;
      for (int k = 0; k < kBlock / 64; ++k) s += red[k];
      a.part[((int64_t)blockIdx.y * a.span + c) * gridDim.x + blockIdx.x] = s;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kBlock) void xsse_valu_combine(const unsigned long long* __restrict__ part, int n_blocks, int tile0,
                                                            int n_frames, int k_lo, int span, int64_t n_ref, int64_t n_dis,
                                                            unsigned long long* __restrict__ out) {
  const int e = blockIdx.x * kBlock + threadIdx.x;
  if (e >= n_frames * span) return;
  const int fl = e / span, c = e - fl * span;
  const int64_t i = (int64_t)tile0 * 32 + fl;
  if (i >= n_ref) return;
  const int64_t j = i + k_lo + c;
  unsigned long long d = ~0ull;
  if (j >= 0 && j < n_dis) {
    d = 0;
    for (int b = 0; b < n_blocks; ++b) d += part[(int64_t)e * n_blocks + b];
  }
  out[i * span + c] = d;
}

bool aligned_to(const XsseClip& c, int esize, int bytes) {
  return (uintptr_t)c.base % bytes == 0 && (c.row_pitch * esize) % bytes == 0 && (c.frame_pitch * esize) % bytes == 0;
}

}  // namespace

int xsse_dis_tiles(int span) { return (31 + span + 31) / 32; }

int xsse_blocks(int w, int h) {
  const int64_t segs = (int64_t)((w + kSegPixels - 1) / kSegPixels) * h;
  const int64_t per_block = (int64_t)kWavesPerBlock * kXsseSegsPerWave;
  return (int)((segs + per_block - 1) / per_block);
}

size_t xsse_part_bytes(bool mfma, int w, int h, int span, int n_tiles) {
  if (mfma) return (size_t)n_tiles * xsse_dis_tiles(span) * xsse_blocks(w, h) * 1024 * sizeof(int);
  return (size_t)n_tiles * 32 * span * kXsseValuBlocks * sizeof(unsigned long long);
}

hipError_t launch_xsse_norms(hipStream_t stream, const XsseClip& clip, int64_t first, int count, int w, int h,
                             unsigned long long* norm_part) {
  if (count <= 0) return hipSuccess;
  const dim3 grid(kXsseNormBlocks, count), block(kBlock);
  if (aligned_to(clip, 1, 16)) hipLaunchKernelGGL((xsse_norm_kernel<true>), grid, block, 0, stream, clip, first, w, h, norm_part);
  else hipLaunchKernelGGL((xsse_norm_kernel<false>), grid, block, 0, stream, clip, first, w, h, norm_part);
  return hipGetLastError();
}

hipError_t launch_cross_sse(hipStream_t stream, Elem elem, bool mfma, const XsseClip& ref, const XsseClip& dis, int w, int h,
                            int k_lo, int span, int tile0, int n_tiles, void* part, const unsigned long long* norm_ref,
                            const unsigned long long* norm_dis, unsigned long long* out) {
  if (n_tiles <= 0 || ref.n <= 0) return hipSuccess;
  if (span < 1 || ref.ring < 1 || dis.ring < 1) return hipErrorInvalidValue;
  if (mfma) {
    if (elem != ELEM_U8 || !norm_ref || !norm_dis) return hipErrorInvalidValue;
    XsseMfmaArgs a{};
    a.ref = ref; a.dis = dis; a.w = w; a.h = h; a.k_lo = k_lo; a.k_hi = k_lo + span - 1; a.tile0 = tile0;
    a.ntd = xsse_dis_tiles(span);
    a.segs_per_row = (w + kSegPixels - 1) / kSegPixels;
    a.n_segs = a.segs_per_row * h;
    a.part = (int*)part;
    const int nb = xsse_blocks(w, h), pairs = n_tiles * a.ntd;
    const dim3 grid(pairs, nb), block(kWavesPerBlock * 64);
    if (aligned_to(ref, 1, 16) && aligned_to(dis, 1, 16)) hipLaunchKernelGGL((xsse_mfma_kernel<true>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((xsse_mfma_kernel<false>), grid, block, 0, stream, a);
    hipLaunchKernelGGL(xsse_mfma_combine, dim3(pairs), dim3(kBlock), 0, stream, (const int*)part, nb, tile0, a.ntd, k_lo, span,
                       ref.n, dis.n, norm_ref, norm_dis, out);
    return hipGetLastError();
  }
  XsseValuArgs a{};
  a.ref = ref; a.dis = dis; a.w = w; a.h = h; a.k_lo = k_lo; a.span = span; a.tile0 = tile0;
  a.part = (unsigned long long*)part;
  const int n_frames = n_tiles * 32;
  const dim3 grid(kXsseValuBlocks, n_frames), block(kBlock);
  if (elem == ELEM_U8) {
    if (aligned_to(ref, 1, 4) && aligned_to(dis, 1, 4)) hipLaunchKernelGGL((xsse_valu_kernel<uint8_t, true>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((xsse_valu_kernel<uint8_t, false>), grid, block, 0, stream, a);
  } else if (elem == ELEM_U16) {
    if (aligned_to(ref, 2, 8) && aligned_to(dis, 2, 8)) hipLaunchKernelGGL((xsse_valu_kernel<uint16_t, true>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((xsse_valu_kernel<uint16_t, false>), grid, block, 0, stream, a);
  } else {
    return hipErrorInvalidValue;
  }
  hipLaunchKernelGGL(xsse_valu_combine, dim3((n_frames * span + kBlock - 1) / kBlock), dim3(kBlock), 0, stream,
                     (const unsigned long long*)part, kXsseValuBlocks, tile0, n_frames, k_lo, span, ref.n, dis.n, out);
  return hipGetLastError();
}

}  // namespace pqa
