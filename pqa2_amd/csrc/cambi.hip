// libvmaf's cambi feature (banding index) of one luma plane per frame.  The definition, its constants and its unpinned
// items: tests/cambi_ref.py and DESIGN.md sections 1 and 5.
//
// Kernels, per pass of up to cambi_sb frames:
//   cambi_prep_kernel<T>       samples -> 10 bit, the derivative D and its 7 x 7 box sum -> the scale-0 plane and mask
//                              (a 16 x 16 tile with its halo in LDS).
//   cambi_down_kernel          scale s > 0: 2:1 decimation of plane and mask, then the separable 3 x 3 mode filter.
//   cambi_cvalue_kernel<S, P>  the hot path: one wave owns a strip of TW columns and a segment of rows and walks down it
//                              with hist[bin][column] of the masked window counts in LDS (libvmaf's scheme).  Each lane
//                              owns one column of the histogram, so the 2(2r + 1) window updates of a row step are
//                              fire-and-forget ds_add_u32 with no read-back and no conflicts between lanes.  Bins hold
//                              only the values a c-value can read (<= max tvi + 4); 8-bit input (every value a multiple
//                              of 4 at every scale) keeps one bin per 4 values.  P: two 16-bit counters per LDS word
//                              (windows of <= 65535 pixels), else one 32-bit counter per word and 32-column strips.
//   cambi_hist_kernel /        exact top-k: a three-round radix select on the f32 bit patterns (non-negative, so they
//   cambi_select_kernel        order as uint): per-chunk LDS histograms, merged with integer atomics (exact counts), and
//                              a per-(frame, scale) scan for the bin holding the k-th largest value.
//   cambi_sum_kernel /         sum of the c-values above c* per chunk in double (fixed order), then per frame
//   cambi_final_kernel         P_s = (sum + (k - #{c > c*}) c*) / k and cambi = sum_s w_s P_s / pixels_in_window.
// No scalar stores, no floating-point atomics: a frame's value depends on nothing but its samples.
#include <cmath>

#include "../../include/pqa_vmaf.h"
#include "kernels.h"
#include "pqa_device.h"

namespace pqa {
namespace {

// ---- constants (tests/cambi_ref.py CONST) ----------------------------------------------------------------------------
constexpr int kMaskSize = 7, kMaskThreshold = 24;
constexpr int kWsNum = 65, kWsDen = 375, kWsShift = 4;
constexpr double kGamma = 2.4, kLw = 300.0, kLb = 0.01, kTviThreshold = 0.019;
constexpr int kBlack = 64, kWhite = 940;
constexpr int kContrastWeights[kCambiDiffs] = {1, 2, 3, 4};
constexpr double kScaleWeights[kCambiScales] = {16.0, 8.0, 4.0, 2.0, 1.0};
constexpr double kTopk = 0.6;
constexpr int kChunk = 4096;                 // c-values per pooling chunk (256 threads x 16)
constexpr uint16_t kNoBin = 0xffff;          // a sample that feeds no histogram bin
constexpr int kPrepT = 16, kPrepR = kMaskSize / 2;   // prep tile and mask radius
constexpr int kApplyChunk = 16;             // window keys read per batch of histogram adds

double eotf(int v) {
  const double a = std::pow(std::pow(kLw, 1.0 / kGamma) - std::pow(kLb, 1.0 / kGamma), kGamma);
  const double b = std::pow(kLb, 1.0 / kGamma) / (std::pow(kLw, 1.0 / kGamma) - std::pow(kLb, 1.0 / kGamma));
  const double V = (double)(v - kBlack) / (double)(kWhite - kBlack);
  return a * std::pow(std::fmax(V + b, 0.0), kGamma);
}

// ---- preprocessing, derivative and mask ------------------------------------------------------------------------------
struct PrepArgs {
  const void* src;
  int64_t rp, fp;       // source pitches, elements
  int w, h, up;         // up: left shift to 10 bit (2 for 8-bit input)
  int tiles_x;
  uint16_t* plane;      // [frames][fstride] (scale 0 at offset 0, pitch w)
  uint8_t* mask;
  int64_t fstride;
};

template <typename T>
__global__ __launch_bounds__(256) void cambi_prep_kernel(const PrepArgs a) {
  constexpr int E = kPrepT + 2 * kPrepR;          // 22: derivative positions of the tile and its halo
  __shared__ uint16_t v[E + 1][E + 1];            // samples: one more row and column for the derivative
  __shared__ uint8_t d[E][E];
  const int fr = blockIdx.y;
  const int tx0 = (blockIdx.x % a.tiles_x) * kPrepT, ty0 = (blockIdx.x / a.tiles_x) * kPrepT;
  const T* src = (const T*)a.src + (int64_t)fr * a.fp;
  for (int i = threadIdx.x; i < (E + 1) * (E + 1); i += 256) {
    const int yy = ty0 - kPrepR + i / (E + 1), xx = tx0 - kPrepR + i % (E + 1);
    v[i / (E + 1)][i % (E + 1)] = (xx >= 0 && xx < a.w && yy >= 0 && yy < a.h) ? (uint16_t)src[(int64_t)yy * a.rp + xx] : 0;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < E * E; i += 256) {
    const int ly = i / E, lx = i % E;
    const int yy = ty0 - kPrepR + ly, xx = tx0 - kPrepR + lx;
    uint8_t dv = 0;
    if (xx >= 0 && xx < a.w && yy >= 0 && yy < a.h) {
      const uint16_t c = v[ly][lx];
      const bool er = xx == a.w - 1 || c == v[ly][lx + 1];
      const bool ed = yy == a.h - 1 || c == v[ly + 1][lx];
      dv = er && ed;
    }
    d[ly][lx] = dv;
  }
  __syncthreads();
  const int lx = threadIdx.x % kPrepT, ly = threadIdx.x / kPrepT;
  const int x = tx0 + lx, y = ty0 + ly;
  if (x >= a.w || y >= a.h) return;
  int s = 0;
#pragma unroll
  for (int dy = 0; dy < kMaskSize; ++dy)
#pragma unroll
    for (int dx = 0; dx < kMaskSize; ++dx) s += d[ly + dy][lx + dx];
  const int64_t o = (int64_t)fr * a.fstride + (int64_t)y * a.w + x;
  a.plane[o] = (uint16_t)(v[ly + kPrepR][lx + kPrepR] << a.up);
  a.mask[o] = s > kMaskThreshold;
}

// ---- decimation and mode filter --------------------------------------------------------------------------------------
__device__ __forceinline__ uint16_t mode3(uint16_t a, uint16_t b, uint16_t c) {
  if (a == b || a == c) return a;
  if (b == c) return b;
  return min(min(a, b), c);
}

struct DownArgs {
  uint16_t* plane;
  uint8_t* mask;
  int64_t fstride, in_off, out_off;
  int pw, w, h;        // previous scale's row pitch (= its width); this scale's size
};

__global__ __launch_bounds__(256) void cambi_down_kernel(const DownArgs a) {
  const int fr = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)a.w * a.h) return;
  const int x = (int)(i % a.w), y = (int)(i / a.w);
  const uint16_t* in = a.plane + (int64_t)fr * a.fstride + a.in_off;
  const auto X = [&](int yy, int xx) { return in[(int64_t)(2 * yy) * a.pw + 2 * xx]; };
  const auto H = [&](int yy) {
    return (x >= 1 && x <= a.w - 2) ? mode3(X(yy, x - 1), X(yy, x), X(yy, x + 1)) : X(yy, x);
  };
  const uint16_t o = (y >= 1 && y <= a.h - 2) ? mode3(H(y - 1), H(y), H(y + 1)) : X(y, x);
  const int64_t oo = (int64_t)fr * a.fstride + a.out_off + i;
  a.plane[oo] = o;
  a.mask[oo] = a.mask[(int64_t)fr * a.fstride + a.in_off + (int64_t)(2 * y) * a.pw + 2 * x];
}

// ---- c-values --------------------------------------------------------------------------------------------------------
struct CvalArgs {
  const uint16_t* plane;
  const uint8_t* mask;
  float* cmap;
  int64_t fstride, off;
  int w, h, r, rows, strips;   // rows: rows per segment
  int vmax;                    // max tvi: centres above it need no c-value; bins run to vmax + 4
  int tvi[kCambiDiffs], wts[kCambiDiffs];
  int nwords;                  // histogram words per column
};

// SHIFT: 2 for 8-bit input (bin = v / 4), 0 for 10-bit.  PACK: two 16-bit counters per word, 64 columns; else one 32-bit
// counter per word, 32 columns.
template <int SHIFT, bool PACK>
__global__ __launch_bounds__(64) void cambi_cvalue_kernel(const CvalArgs a) {
  constexpr int TW = PACK ? 64 : 32;
  extern __shared__ uint32_t lds[];
  uint32_t* hist = lds;                                        // [nwords][TW]
  uint16_t* buf_in = (uint16_t*)(lds + a.nwords * TW);         // [TW + 2r + kApplyChunk] keys of the row entering the window
  uint16_t* buf_out = buf_in + TW + 2 * a.r + kApplyChunk;     // [TW + 2r + kApplyChunk] keys of the row leaving it
  const int lane = threadIdx.x;
  const int fr = blockIdx.y;
  const int x0 = (blockIdx.x % a.strips) * TW, y0 = (blockIdx.x / a.strips) * a.rows;
  const int y1 = min(a.h, y0 + a.rows);
  const int span = TW + 2 * a.r;
  const uint16_t* P = a.plane + (int64_t)fr * a.fstride + a.off;
  const uint8_t* M = a.mask + (int64_t)fr * a.fstride + a.off;
  float* C = a.cmap + (int64_t)fr * a.fstride + a.off;
  const int vtop = a.vmax + 4;

  for (int i = 0; i < a.nwords; ++i) hist[i * TW + lane] = 0u;   // a lane's own column: no barrier needed
  const auto stage = [&](int yy, uint16_t* buf) {
    for (int i = lane; i < span + kApplyChunk; i += TW) {
      const int xx = x0 - a.r + i;
      uint16_t key = kNoBin;
      if (i < span && yy >= 0 && yy < a.h && xx >= 0 && xx < a.w) {
        const int64_t o = (int64_t)yy * a.w + xx;
        const int v = P[o];
        if (M[o] && v <= vtop) key = (uint16_t)(v >> SHIFT);
      }
      buf[i] = key;
    }
  };
  // keys are read in chunks of kApplyChunk before any of the chunk's adds: LDS runs in order, so a key read behind an add
  // would wait out the add too, and one read per add would make the walk a chain of LDS round trips
  const auto apply = [&](const uint16_t* buf, bool add) {
    const int n = 2 * a.r + 1;
    for (int i0 = 0; i0 < n; i0 += kApplyChunk) {
      uint16_t key[kApplyChunk];
#pragma unroll
      for (int j = 0; j < kApplyChunk; ++j) {
        const uint16_t k = buf[lane + i0 + j];   // in bounds: the buffers carry kApplyChunk spare keys
        key[j] = i0 + j < n ? k : kNoBin;
      }
#pragma unroll
      for (int j = 0; j < kApplyChunk; ++j) {
        if (key[j] != kNoBin) {
          uint32_t word, inc;
          if (PACK) { word = (uint32_t)(key[j] >> 1) * TW + lane; inc = 1u << ((key[j] & 1) * 16); }
          else { word = (uint32_t)key[j] * TW + lane; inc = 1u; }
          __hip_atomic_fetch_add(&hist[word], add ? inc : 0u - inc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
      }
    }
  };
  const auto count = [&](int u) -> int {
    if (u < 0 || u > vtop || (SHIFT && (u & ((1 << SHIFT) - 1)))) return 0;
    const int key = u >> SHIFT;
    if (PACK) {
      const uint32_t wv = __hip_atomic_load(&hist[(key >> 1) * TW + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      return (int)((wv >> ((key & 1) * 16)) & 0xffffu);
    }
    return (int)__hip_atomic_load(&hist[key * TW + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  };

  // the window of row y0 without its last row: rows [y0 - r, y0 + r - 1]
  for (int yy = max(0, y0 - a.r); yy < min(a.h, y0 + a.r); ++yy) {
    stage(yy, buf_in);
    __syncthreads();
    apply(buf_in, true);
    __syncthreads();
  }
  for (int y = y0; y < y1; ++y) {
    const bool enter = y + a.r < a.h, leave = y - a.r >= 0;
    if (enter) stage(y + a.r, buf_in);
    if (leave) stage(y - a.r, buf_out);
    __syncthreads();
    if (enter) apply(buf_in, true);
    const int x = x0 + lane;
    if (lane < TW && x < a.w) {
      const int64_t o = (int64_t)y * a.w + x;
      const int v = P[o];
      float c = 0.0f;
      if (M[o] && v <= a.vmax) {
        const int p0 = count(v);
#pragma unroll
        for (int d = 1; d <= kCambiDiffs; ++d) {
          if (v > a.tvi[d - 1]) continue;
          const int q = max(count(v + d), count(v - d));
          if (p0 + q > 0) {
            const float num = (float)((long long)a.wts[d - 1] * p0 * q);   // integer product, then f32 (RNE)
            c = fmaxf(c, num / (float)(p0 + q));                          // IEEE f32 division
          }
        }
      }
      C[o] = c;
    }
    if (leave) apply(buf_out, false);
    __syncthreads();
  }
}

// ---- exact top-k pooling ---------------------------------------------------------------------------------------------
// radix rounds over the 31 value bits (the sign bit is 0): bits [20, 31), [10, 20), [0, 10)
__host__ __device__ constexpr int round_shift(int rd) { return rd == 0 ? 20 : rd == 1 ? 10 : 0; }
__host__ __device__ constexpr int round_bits(int rd) { return rd == 0 ? 11 : 10; }
constexpr int kHistBins = 2048;
enum { SEL_PREFIX = 0, SEL_KREM = 1, SEL_GT = 2, SEL_ZEROS = 3 };   // radix-select state per (frame, scale)

struct PoolArgs {
  const float* cmap;
  int64_t fstride;
  int64_t off[kCambiScales + 1];
  int chunk[kCambiScales + 1];
  int topk[kCambiScales];
  uint32_t* hist;         // [frames][5][2048]
  int32_t* sel;           // [frames][5][4]
  double* partials;       // [frames][chunk[5]]
  int rd;
  // epilogue
  double* ext;
  int ext_stride, slot, slot_base, slot_step, capacity;
  double inv_piw;
};

__device__ __forceinline__ int chunk_scale(const PoolArgs& a, int c) {
  int s = 0;
  while (s < kCambiScales - 1 && c >= a.chunk[s + 1]) ++s;
  return s;
}

__global__ __launch_bounds__(256) void cambi_hist_kernel(const PoolArgs a) {
  __shared__ uint32_t h[kHistBins];
  const int fr = blockIdx.y, c = blockIdx.x;
  const int s = chunk_scale(a, c);
  const int32_t* st = a.sel + ((int64_t)fr * kCambiScales + s) * 4;
  const int shift = round_shift(a.rd), bits = round_bits(a.rd), hi = shift + bits;
  const uint32_t prefix = a.rd == 0 ? 0u : (uint32_t)st[SEL_PREFIX];
  for (int i = threadIdx.x; i < kHistBins; i += 256) h[i] = 0u;
  __syncthreads();
  const int64_t n = a.off[s + 1] - a.off[s];
  const int64_t b0 = (int64_t)(c - a.chunk[s]) * kChunk;
  const uint32_t* src = (const uint32_t*)(a.cmap + (int64_t)fr * a.fstride + a.off[s]);
  for (int64_t i = b0 + threadIdx.x; i < b0 + kChunk && i < n; i += 256) {
    const uint32_t u = src[i];
    if (u != 0u && (u >> hi) == prefix) atomicAdd(&h[(u >> shift) & ((1u << bits) - 1u)], 1u);   // zeros: counted by the select
  }
  __syncthreads();
  uint32_t* g = a.hist + ((int64_t)fr * kCambiScales + s) * kHistBins;
  for (int i = threadIdx.x; i < (1 << bits); i += 256)
    if (h[i]) atomicAdd(&g[i], h[i]);
}

__global__ __launch_bounds__(256) void cambi_select_kernel(const PoolArgs a) {
  __shared__ int sums[256];
  __shared__ int above[256];
  __shared__ int zadd;
  const int s = blockIdx.x, fr = blockIdx.y, t = threadIdx.x;
  int32_t* st = a.sel + ((int64_t)fr * kCambiScales + s) * 4;
  uint32_t* g = a.hist + ((int64_t)fr * kCambiScales + s) * kHistBins;
  const int bits = round_bits(a.rd), nb = 1 << bits, per = nb / 256;
  const uint32_t prefix = a.rd == 0 ? 0u : (uint32_t)st[SEL_PREFIX];
  const int n = (int)(a.off[s + 1] - a.off[s]);
  const int krem = a.rd == 0 ? a.topk[s] : st[SEL_KREM];
  const int gt = a.rd == 0 ? 0 : st[SEL_GT];
  // thread t owns bins [nb - (t + 1) per, nb - t per): thread 0 the highest
  int cnt[8];
  int sum = 0;
  for (int j = 0; j < per; ++j) {
    const int b = nb - 1 - (t * per + j);
    cnt[j] = (int)g[b];
    sum += cnt[j];
  }
  sums[t] = sum;
  __syncthreads();
  if (t == 0) {
    int tot = 0;
    for (int i = 0; i < 256; ++i) { above[i] = tot; tot += sums[i]; }
    // zeros were left out of the histograms: they sit in bin 0 while every higher bit chosen so far is 0
    const int zeros = a.rd == 0 ? n - tot : st[SEL_ZEROS];
    if (a.rd == 0) st[SEL_ZEROS] = zeros;
    zadd = prefix == 0u ? zeros : 0;
    sums[255] += zadd;   // bin 0 belongs to thread 255
  }
  __syncthreads();
  if (t == 255) cnt[per - 1] += zadd;
  const int ab = above[t];
  if (ab < krem && krem <= ab + sums[t]) {
    int acc = ab;
    for (int j = 0; j < per; ++j) {
      const int b = nb - 1 - (t * per + j);
      if (krem <= acc + cnt[j]) {
        st[SEL_PREFIX] = (int32_t)((prefix << bits) | (uint32_t)b);
        st[SEL_KREM] = krem - acc;
        st[SEL_GT] = gt + acc;
        break;
      }
      acc += cnt[j];
    }
  }
  __syncthreads();
  for (int j = 0; j < per; ++j) g[nb - 1 - (t * per + j)] = 0u;   // ready for the next round
}

__global__ __launch_bounds__(256) void cambi_sum_kernel(const PoolArgs a) {
  __shared__ double red[4];
  const int fr = blockIdx.y, c = blockIdx.x;
  const int s = chunk_scale(a, c);
  const uint32_t cstar = (uint32_t)a.sel[((int64_t)fr * kCambiScales + s) * 4 + SEL_PREFIX];
  const int64_t n = a.off[s + 1] - a.off[s];
  const int64_t b0 = (int64_t)(c - a.chunk[s]) * kChunk;
  const uint32_t* src = (const uint32_t*)(a.cmap + (int64_t)fr * a.fstride + a.off[s]);
  double acc[1] = {0.0};
  for (int64_t i = b0 + threadIdx.x; i < b0 + kChunk && i < n; i += 256) {
    const uint32_t u = src[i];
    if (u > cstar) acc[0] += (double)__uint_as_float(u);
  }
  block_sum<1>(acc, red);
  if (threadIdx.x == 0) a.partials[(int64_t)fr * a.chunk[kCambiScales] + c] = acc[0];
}

__global__ __launch_bounds__(256) void cambi_final_kernel(const PoolArgs a) {
  __shared__ double red[4];
  const int fr = blockIdx.x;
  double score = 0.0;
  for (int s = 0; s < kCambiScales; ++s) {
    double acc[1] = {0.0};
    const double* p = a.partials + (int64_t)fr * a.chunk[kCambiScales];
    for (int c = a.chunk[s] + threadIdx.x; c < a.chunk[s + 1]; c += 256) acc[0] += p[c];
    block_sum<1>(acc, red);
    if (threadIdx.x == 0) {
      const int32_t* st = a.sel + ((int64_t)fr * kCambiScales + s) * 4;
      const double cstar = (double)__uint_as_float((uint32_t)st[SEL_PREFIX]);
      const int k = a.topk[s];
      const double P = (acc[0] + (double)(k - st[SEL_GT]) * cstar) / (double)k;
      score += kScaleWeights[s] * P;
    }
    __syncthreads();   // red is reused by the next scale
  }
  if (threadIdx.x != 0) return;
  const int row = (int)(((int64_t)a.slot_base + (int64_t)fr * a.slot_step) % a.capacity);
  a.ext[(int64_t)row * a.ext_stride + a.slot] = score * a.inv_piw;
}

// The c-value kernel's instance and LDS bytes at a frame size and bit depth.
struct CvalShape {
  int shift, tw, nwords, vmax;
  bool pack;
  size_t lds;
};
CvalShape cval_shape(const CambiParams& prm, int bit_depth) {
  CvalShape c{};
  for (int d = 0; d < kCambiDiffs; ++d) c.vmax = prm.tvi[d] > c.vmax ? prm.tvi[d] : c.vmax;
  c.shift = bit_depth == 8 ? 2 : 0;
  c.pack = prm.piw <= 65535;
  c.tw = c.pack ? 64 : 32;
  const int nbins = ((c.vmax + 4) >> c.shift) + 1;
  c.nwords = c.pack ? (nbins + 1) / 2 : nbins;
  c.lds = (size_t)c.nwords * c.tw * 4 + (size_t)2 * (c.tw + 2 * prm.r + kApplyChunk) * 2;
  return c;
}

template <int SHIFT, bool PACK>
hipError_t launch_cvalue(hipStream_t stream, const CvalArgs& a, int n_frames, int segs, size_t lds) {
  hipLaunchKernelGGL((cambi_cvalue_kernel<SHIFT, PACK>), dim3(a.strips * segs, n_frames), dim3(PACK ? 64 : 32), lds, stream, a);
  return hipGetLastError();
}

}  // namespace

hipError_t cambi_prepare(const CambiParams& prm, int bit_depth) {
  if (bit_depth != 8 && bit_depth != 10) return hipErrorInvalidValue;
  const CvalShape cs = cval_shape(prm, bit_depth);
  if (cs.lds > 163840) return hipErrorInvalidValue;
  // more than 64 KiB of dynamic LDS (10-bit histograms) must be asked for, once per context
  const void* k = cs.shift == 2 ? (cs.pack ? (const void*)cambi_cvalue_kernel<2, true> : (const void*)cambi_cvalue_kernel<2, false>)
                                : (cs.pack ? (const void*)cambi_cvalue_kernel<0, true> : (const void*)cambi_cvalue_kernel<0, false>);
  return hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)cs.lds);
}

CambiParams cambi_params(int w, int h) {
  CambiParams p{};
  p.ws = ((kWsNum * (w + h)) / kWsDen) >> kWsShift;
  p.r = p.ws >> 1;
  p.piw = (2 * p.r + 1) * (2 * p.r + 1);
  p.mask_t = kMaskThreshold;
  for (int d = 1; d <= kCambiDiffs; ++d) {
    int best = kBlack - 1;
    for (int v = kBlack; v <= kWhite - d; ++v)
      if (eotf(v + d) - eotf(v) > kTviThreshold * eotf(v)) best = v;
    p.tvi[d - 1] = best;
    p.weights[d - 1] = kContrastWeights[d - 1];
  }
  int sw = w, sh = h;
  p.off[0] = 0;
  p.chunk[0] = 0;
  for (int s = 0; s < kCambiScales; ++s) {
    p.sw[s] = sw; p.sh[s] = sh;
    const int64_t n = (int64_t)sw * sh;
    p.off[s + 1] = p.off[s] + n;
    p.chunk[s + 1] = p.chunk[s] + (int)((n + kChunk - 1) / kChunk);
    int64_t k = (int64_t)(kTopk * (double)n);
    p.topk[s] = (int)(k < 1 ? 1 : k > n ? n : k);
    sw = (sw + 1) >> 1; sh = (sh + 1) >> 1;
  }
  return p;
}

hipError_t launch_cambi(hipStream_t stream, Elem elem, PlaneRun luma, int n_frames, int w, int h, int bit_depth,
                        const CambiParams& prm, const CambiWork& wk, double* ext, int ext_stride, int slot, int slot_base,
                        int slot_step, int capacity) {
  if (n_frames <= 0) return hipSuccess;
  if ((bit_depth != 8 && bit_depth != 10) || (elem != ELEM_U8 && elem != ELEM_U16)) return hipErrorInvalidValue;
  const int64_t fstride = prm.off[kCambiScales];
  hipError_t e;
  {
    PrepArgs a{};
    a.src = luma.base; a.rp = luma.row_pitch; a.fp = luma.frame_pitch;
    a.w = w; a.h = h; a.up = bit_depth == 8 ? 2 : 0;
    a.tiles_x = (w + kPrepT - 1) / kPrepT;
    a.plane = wk.plane; a.mask = wk.mask; a.fstride = fstride;
    const dim3 grid(a.tiles_x * ((h + kPrepT - 1) / kPrepT), n_frames);
    if (elem == ELEM_U8) hipLaunchKernelGGL(cambi_prep_kernel<uint8_t>, grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(cambi_prep_kernel<uint16_t>, grid, dim3(256), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  for (int s = 1; s < kCambiScales; ++s) {
    DownArgs a{};
    a.plane = wk.plane; a.mask = wk.mask; a.fstride = fstride;
    a.in_off = prm.off[s - 1]; a.out_off = prm.off[s];
    a.pw = prm.sw[s - 1]; a.w = prm.sw[s]; a.h = prm.sh[s];
    const int64_t n = (int64_t)a.w * a.h;
    hipLaunchKernelGGL(cambi_down_kernel, dim3((unsigned)((n + 255) / 256), n_frames), dim3(256), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  const CvalShape cs = cval_shape(prm, bit_depth);
  const int vmax = cs.vmax, shift = cs.shift, TW = cs.tw, nwords = cs.nwords;
  const bool pack = cs.pack;
  const size_t lds = cs.lds;
  if (lds > 163840) return hipErrorInvalidValue;
  for (int s = 0; s < kCambiScales; ++s) {
    CvalArgs a{};
    a.plane = wk.plane; a.mask = wk.mask; a.cmap = wk.cmap;
    a.fstride = fstride; a.off = prm.off[s];
    a.w = prm.sw[s]; a.h = prm.sh[s]; a.r = prm.r;
    a.strips = (a.w + TW - 1) / TW;
    // rows per segment: 8r (a segment's first window costs 2r row additions), halved down to 32 while a frame has fewer
    // than 256 segments -- the deep scales are a few serial walks otherwise
    a.rows = 8 * prm.r > 32 ? 8 * prm.r : 32;
    while (a.rows > 32 && a.strips * ((a.h + a.rows - 1) / a.rows) < 256) a.rows /= 2;
    a.rows = a.rows < 32 ? 32 : a.rows;
    a.vmax = vmax;
    for (int d = 0; d < kCambiDiffs; ++d) { a.tvi[d] = prm.tvi[d]; a.wts[d] = prm.weights[d]; }
    a.nwords = nwords;
    const int segs = (a.h + a.rows - 1) / a.rows;
    if (shift == 2) e = pack ? launch_cvalue<2, true>(stream, a, n_frames, segs, lds) : launch_cvalue<2, false>(stream, a, n_frames, segs, lds);
    else e = pack ? launch_cvalue<0, true>(stream, a, n_frames, segs, lds) : launch_cvalue<0, false>(stream, a, n_frames, segs, lds);
    if (e != hipSuccess) return e;
  }
  PoolArgs pa{};
  pa.cmap = wk.cmap; pa.fstride = fstride;
  for (int s = 0; s <= kCambiScales; ++s) { pa.off[s] = prm.off[s]; pa.chunk[s] = prm.chunk[s]; }
  for (int s = 0; s < kCambiScales; ++s) pa.topk[s] = prm.topk[s];
  pa.hist = wk.hist; pa.sel = wk.sel; pa.partials = wk.partials;
  pa.ext = ext; pa.ext_stride = ext_stride; pa.slot = slot;
  pa.slot_base = slot_base; pa.slot_step = slot_step; pa.capacity = capacity;
  pa.inv_piw = 1.0 / (double)prm.piw;
  if ((e = hipMemsetAsync(wk.hist, 0, (size_t)n_frames * kCambiScales * kHistBins * sizeof(uint32_t), stream)) != hipSuccess)
    return e;
  const dim3 cgrid(prm.chunk[kCambiScales], n_frames);
  for (int rd = 0; rd < 3; ++rd) {
    pa.rd = rd;
    hipLaunchKernelGGL(cambi_hist_kernel, cgrid, dim3(256), 0, stream, pa);
    hipLaunchKernelGGL(cambi_select_kernel, dim3(kCambiScales, n_frames), dim3(256), 0, stream, pa);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(cambi_sum_kernel, cgrid, dim3(256), 0, stream, pa);
  hipLaunchKernelGGL(cambi_final_kernel, dim3(n_frames), dim3(256), 0, stream, pa);
  return hipGetLastError();
}

}  // namespace pqa
