// FFmpeg's xpsnr filter (libavfilter/vf_xpsnr.c): PSNR whose luma blocks are weighted by the reference's spatial
// (high-pass) and temporal (difference to the previous one or two reference frames) activity; chroma blocks reuse the
// luma weights.  The definition, its constants and its unpinned items: tests/xpsnr_ref.py and DESIGN.md section 1.
//
// Two kernels:
//   xp_block_kernel<T, BV>  one workgroup per (luma block, frame).  Exact integers per block: the luma SSE, the spatial
//                           activity sa (|high-pass| summed over the block minus its picture-edge margins), the temporal
//                           activity ta (gamma * sum |o - o1| or |o - 2 o1 + o2|, on 2 x 2 sums when BV = 2) and the SSE
//                           of chroma block k of U and V.  The block is walked in strips of kXpStrip rows; each strip's
//                           reference rows plus a 2-row / 2-column halo are staged in LDS as int16 and the high-pass taps
//                           read them from there (BV = 2: three dword reads per tap row, each a pair of samples).  One wave
//                           per (group) row, lanes along x.  Per-lane 32-bit partials per strip (a strip bounds them:
//                           48 samples of at most 4095^2 per lane), then 64-bit, then a fixed wave / workgroup reduction.
//   xp_finalize_kernel      one wave per frame: the weights in parallel, the minimum smoothing (frames <= 640 x 480) in
//                           one lane, the raster-order double sums, WSSE and dB into the frame's ext3 row.  Built with FP
//                           contraction off, so WSSE equals the restatement bit for bit.
// No atomics: a frame's values do not depend on batch, launch, pitch or alignment.
#include <cmath>

#include "../../include/pqa_vmaf.h"
#include "kernels.h"
#include "pqa_device.h"

namespace pqa {

void xpsnr_geometry(int w, int h, int wc, int hc, int n_planes, int bit_depth, XpsnrGeometry* g) {
  *g = XpsnrGeometry{};
  g->W = w; g->H = h; g->Wc = wc; g->Hc = hc;
  g->n_planes = n_planes;
  g->bit_depth = bit_depth;
  const double r = (double)((uint32_t)w * (uint32_t)h) / (3840.0 * 2160.0);   // vf_xpsnr.c: the UHD ratio
  g->b = 4 * (int)(32.0 * std::sqrt(r) + 0.5);
  g->bv = (int64_t)w * h > 2048ll * 1152ll ? 2 : 1;
  g->smooth = (int64_t)w * h <= 640ll * 480ll ? 1 : 0;
  g->A = std::sqrt(16.0 * (double)(1 << (2 * bit_depth - 9)) / std::sqrt(std::max(0.00001, r)));
  g->plain = g->b < 4 ? 1 : 0;
  if (g->plain) {   // too small for weighting: every plane's WSSE is its SSE; one "block" per plane
    g->bsx = w; g->bsy = h;
    g->cbx = wc; g->cby = hc;
  } else {
    g->bsx = g->bsy = g->b;
    g->cbx = (g->b * wc) / w;
    g->cby = (g->b * hc) / h;
  }
  g->w_blk = (w + g->bsx - 1) / g->bsx;
  g->h_blk = (h + g->bsy - 1) / g->bsy;
  g->n_blk = g->w_blk * g->h_blk;
  if (n_planes == 3 && g->cbx > 0 && g->cby > 0) {
    g->cw_blk = (wc + g->cbx - 1) / g->cbx;
    g->ch_blk = (hc + g->cby - 1) / g->cby;
    g->nc_blk = g->cw_blk * g->ch_blk;
  }
}

namespace {

struct XpBlockArgs {
  const void* ref[3];
  const void* dis[3];
  int rp_r[3], rp_d[3];          // row pitches, elements
  int64_t fp_r[3], fp_d[3];      // frame pitches, elements
  const void* h1;                // reference frame first-1 (nullptr: zero plane)
  const void* h2;                // reference frame first-2
  int hp1, hp2;                  // their row pitches, elements
  int hfr;                       // second-order temporal term
  XpsnrGeometry g;
  unsigned long long* out;       // [n_frames][g.n_blk][kXpBlockVals]
};

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// Two adjacent int16 samples of the staged strip (col even, so the dword is aligned)
__device__ __forceinline__ void lds_pair(const int16_t* s, int idx, int& lo, int& hi) {
  const int v = *(const int*)(s + idx);
  lo = (int)(int16_t)(v & 0xffff);
  hi = v >> 16;
}

template <typename T, int BV>
__global__ __launch_bounds__(kBlock) void xp_block_kernel(const XpBlockArgs a) {
  __shared__ __align__(16) int16_t so[(kXpStrip + 4) * kXpLdsCols];
  __shared__ unsigned long long red[4][kXpBlockVals];
  const XpsnrGeometry& g = a.g;
  const int k = blockIdx.x, f = blockIdx.y;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int x0 = (k % g.w_blk) * g.bsx, y0 = (k / g.w_blk) * g.bsy;
  const int bw = min(g.bsx, g.W - x0), bh = min(g.bsy, g.H - y0);
  const int rpo = a.rp_r[0], rpd = a.rp_d[0];
  const T* o = (const T*)a.ref[0] + (int64_t)f * a.fp_r[0];
  const T* r = (const T*)a.dis[0] + (int64_t)f * a.fp_d[0];
  // the predecessors: frames of this batch, else the history the host resolved (nullptr: zero plane)
  const T* o1 = f >= 1 ? o - a.fp_r[0] : (const T*)a.h1;
  const int p1 = f >= 1 ? rpo : a.hp1;
  const T* o2 = f >= 2 ? o - 2 * a.fp_r[0] : f == 1 ? (const T*)a.h1 : (const T*)a.h2;
  const int p2 = f >= 2 ? rpo : f == 1 ? a.hp1 : a.hp2;
  // picture-edge margins of the high-pass (vf_xpsnr.c calc_squared_error_and_weight)
  const int xa = x0 == 0 ? BV : 0, wa = x0 + bw >= g.W ? bw - BV : bw;
  const int ya = y0 == 0 ? BV : 0, ha = y0 + bh >= g.H ? bh - BV : bh;
  const bool act = !g.plain && wa > xa && ha > ya;   // otherwise: SSE only, weight 1
  const int LC = bw + 4;
  unsigned long long sse = 0, sa = 0, ta = 0;

  for (int s0 = 0; s0 < bh; s0 += kXpStrip) {
    const int sr = min(kXpStrip, bh - s0);
    unsigned sse_l = 0, sa_l = 0, ta_l = 0;
    if (act) {
      __syncthreads();   // the previous strip's taps are read
      for (int rr = wv; rr < sr + 4; rr += 4) {
        const int yy = y0 + s0 + rr - 2;
        const bool yin = yy >= 0 && yy < g.H;
        for (int cc = lane; cc < LC; cc += 64) {
          const int xx = x0 + cc - 2;
          so[rr * LC + cc] = (yin && xx >= 0 && xx < g.W) ? (int16_t)o[(int64_t)yy * rpo + xx] : (int16_t)0;
        }
      }
      __syncthreads();
      const int ylo = max(s0, ya), yhi = min(s0 + sr, ha);
      if (BV == 1) {
        for (int y = ylo + wv; y < yhi; y += 4) {
          const int16_t* c = so + (y - s0 + 2) * LC + 2;
          for (int x = xa + lane; x < wa; x += 64) {
            const int fv = 12 * c[x] - 2 * (c[x - 1] + c[x + 1] + c[x - LC] + c[x + LC]) -
                           (c[x - LC - 1] + c[x - LC + 1] + c[x + LC - 1] + c[x + LC + 1]);
            sa_l += (unsigned)abs(fv);
          }
        }
      } else {
        // group rows y (even, relative to the block) split over the waves; ylo is even (s0, ya are)
#pragma unroll 1
        for (int y = ylo + 2 * wv; y < yhi; y += 8) {
          const int16_t* c = so + (y - s0 + 2) * LC + 2;   // c[x] = sample (y, x) of the block
#pragma unroll 1
          for (int x = xa + 2 * lane; x < wa; x += 128) {
            int m2[6], m1[6], z0[6], z1[6], q2[6], q3[6];   // rows y-2 .. y+3, columns x-2 .. x+3
            lds_pair(c, -2 * LC + x - 2, m2[0], m2[1]); lds_pair(c, -2 * LC + x, m2[2], m2[3]); lds_pair(c, -2 * LC + x + 2, m2[4], m2[5]);
            lds_pair(c, -LC + x - 2, m1[0], m1[1]); lds_pair(c, -LC + x, m1[2], m1[3]); lds_pair(c, -LC + x + 2, m1[4], m1[5]);
            lds_pair(c, x - 2, z0[0], z0[1]); lds_pair(c, x, z0[2], z0[3]); lds_pair(c, x + 2, z0[4], z0[5]);
            lds_pair(c, LC + x - 2, z1[0], z1[1]); lds_pair(c, LC + x, z1[2], z1[3]); lds_pair(c, LC + x + 2, z1[4], z1[5]);
            lds_pair(c, 2 * LC + x - 2, q2[0], q2[1]); lds_pair(c, 2 * LC + x, q2[2], q2[3]); lds_pair(c, 2 * LC + x + 2, q2[4], q2[5]);
            lds_pair(c, 3 * LC + x - 2, q3[0], q3[1]); lds_pair(c, 3 * LC + x, q3[2], q3[3]); lds_pair(c, 3 * LC + x + 2, q3[4], q3[5]);
            const int fv = 12 * (z0[2] + z0[3] + z1[2] + z1[3]) -
                           3 * (m1[2] + m1[3] + q2[2] + q2[3]) -
                           3 * (z0[1] + z1[1] + z0[4] + z1[4]) -
                           2 * (m1[1] + m1[4] + q2[1] + q2[4]) -
                           (m2[1] + m2[2] + m2[3] + m2[4] + q3[1] + q3[2] + q3[3] + q3[4] +
                            m1[0] + z0[0] + z1[0] + q2[0] + m1[5] + z0[5] + z1[5] + q2[5]);
            sa_l += (unsigned)abs(fv);
          }
        }
      }
    }
    // SSE over every sample of the strip; the temporal term over the whole block (samples, or 2 x 2 sums when BV = 2)
    for (int y = s0 + wv; y < s0 + sr; y += 4) {
      const T* orow = o + (int64_t)(y0 + y) * rpo + x0;
      const T* rrow = r + (int64_t)(y0 + y) * rpd + x0;
      for (int x = lane; x < bw; x += 64) {
        const int d = (int)orow[x] - (int)rrow[x];
        sse_l += (unsigned)(d * d);
      }
    }
    if (act && BV == 1) {
      for (int y = s0 + wv; y < s0 + sr; y += 4) {
        const T* orow = o + (int64_t)(y0 + y) * rpo + x0;
        const T* prow1 = o1 ? o1 + (int64_t)(y0 + y) * p1 + x0 : nullptr;
        const T* prow2 = o2 ? o2 + (int64_t)(y0 + y) * p2 + x0 : nullptr;
        for (int x = lane; x < bw; x += 64) {
          const int v0 = orow[x], v1 = prow1 ? (int)prow1[x] : 0;
          int t = v0 - v1;
          if (a.hfr) t = v0 - 2 * v1 + (prow2 ? (int)prow2[x] : 0);
          ta_l += (unsigned)abs(t);
        }
      }
    } else if (act) {
      for (int y = s0 + 2 * wv; y < s0 + sr; y += 8) {
        const T* oa = o + (int64_t)(y0 + y) * rpo + x0;
        const T* pa1 = o1 ? o1 + (int64_t)(y0 + y) * p1 + x0 : nullptr;
        const T* pa2 = o2 ? o2 + (int64_t)(y0 + y) * p2 + x0 : nullptr;
        for (int x = 2 * lane; x < bw; x += 128) {
          const int s_0 = (int)oa[x] + (int)oa[x + 1] + (int)oa[rpo + x] + (int)oa[rpo + x + 1];
          const int s_1 = pa1 ? (int)pa1[x] + (int)pa1[x + 1] + (int)pa1[p1 + x] + (int)pa1[p1 + x + 1] : 0;
          int t = s_0 - s_1;
          if (a.hfr) t = s_0 - 2 * s_1 + (pa2 ? (int)pa2[x] + (int)pa2[x + 1] + (int)pa2[p2 + x] + (int)pa2[p2 + x + 1] : 0);
          ta_l += (unsigned)abs(t);
        }
      }
    }
    sse += sse_l; sa += sa_l; ta += ta_l;
  }

  // chroma block k of U and V (the chroma grid is never larger than the luma grid: pqa_create checks it)
  unsigned long long sse_c[2] = {0, 0};
  if (g.n_planes == 3 && k < g.nc_blk) {
    const int cx0 = (k % g.cw_blk) * g.cbx, cy0 = (k / g.cw_blk) * g.cby;
    const int cw = min(g.cbx, g.Wc - cx0), ch = min(g.cby, g.Hc - cy0);
#pragma unroll
    for (int p = 1; p < 3; ++p) {
      const T* oc = (const T*)a.ref[p] + (int64_t)f * a.fp_r[p];
      const T* rc = (const T*)a.dis[p] + (int64_t)f * a.fp_d[p];
      unsigned long long acc = 0;
      for (int y = wv; y < ch; y += 4) {
        const T* orow = oc + (int64_t)(cy0 + y) * a.rp_r[p] + cx0;
        const T* rrow = rc + (int64_t)(cy0 + y) * a.rp_d[p] + cx0;
        for (int x = lane; x < cw; x += 64) {
          const int d = (int)orow[x] - (int)rrow[x];
          acc += (unsigned)(d * d);
        }
      }
      sse_c[p - 1] = acc;
    }
  }

  unsigned long long v[kXpBlockVals] = {sse, sa, kXpGamma * ta, sse_c[0], sse_c[1]};
#pragma unroll
  for (int i = 0; i < kXpBlockVals; ++i) v[i] = wave_sum_u64(v[i]);
  if (lane == 0)
#pragma unroll
    for (int i = 0; i < kXpBlockVals; ++i) red[wv][i] = v[i];
  __syncthreads();
  if (threadIdx.x < kXpBlockVals) {
    const int i = threadIdx.x;
    a.out[((int64_t)f * g.n_blk + k) * kXpBlockVals + i] = red[0][i] + red[1][i] + red[2][i] + red[3][i];
  }
}

// The restatement's weight of luma block k from its exact sums (tests/xpsnr_ref.py block_weight)
__device__ double xp_weight(const XpsnrGeometry& g, int k, unsigned long long sa, unsigned long long ta) {
#pragma clang fp contract(off)
  const int x0 = (k % g.w_blk) * g.bsx, y0 = (k / g.w_blk) * g.bsy;
  const int bw = min(g.bsx, g.W - x0), bh = min(g.bsy, g.H - y0);
  const int xa = x0 == 0 ? g.bv : 0, wa = x0 + bw >= g.W ? bw - g.bv : bw;
  const int ya = y0 == 0 ? g.bv : 0, ha = y0 + bh >= g.H ? bh - g.bv : bh;
  if (wa <= xa || ha <= ya) return 1.0;   // ms_act = 1
  double ms = (double)sa / ((double)(wa - xa) * (double)(ha - ya));
  ms += (double)ta / ((double)bw * (double)bh);
  const double lo = (double)(1 << (g.bit_depth - 6));
  if (ms < lo) ms = lo;
  ms *= ms;
  return 1.0 / sqrt(ms);
}

__device__ double xp_db(unsigned long long wsse, int w, int h, int bit_depth) {
  if (wsse == 0) return __builtin_inf();
  const unsigned long long mx = (1ull << bit_depth) - 1;
  const unsigned long long num = mx * mx * (unsigned long long)w * (unsigned long long)h;
  return 10.0 * log10((double)num / (double)wsse);
}

__global__ __launch_bounds__(64) void xp_finalize_kernel(const XpFinalizeArgs a) {
#pragma clang fp contract(off)
  const XpsnrGeometry& g = a.g;
  const int f = blockIdx.x;
  const unsigned long long* blk = a.blk + (int64_t)f * g.n_blk * kXpBlockVals;
  double* w = a.wbuf + (int64_t)f * g.n_blk;
  if (!g.plain)
    for (int k = threadIdx.x; k < g.n_blk; k += 64) w[k] = xp_weight(g, k, blk[k * kXpBlockVals + 1], blk[k * kXpBlockVals + 2]);
  __syncthreads();
  if (threadIdx.x != 0) return;
  const int row = (int)(((int64_t)a.slot_base + f) % a.capacity);
  double* e = a.ext3 + (int64_t)row * a.ext_stride;
  unsigned long long wsse[3] = {0, 0, 0};
  if (g.plain) {
    for (int p = 0; p < g.n_planes; ++p) wsse[p] = blk[p == 0 ? 0 : 2 + p];
  } else {
    if (g.smooth) {   // in-line minimum smoothing (vf_xpsnr.c get_wsse), sequential in raster order
      const int b = g.b, wb = g.w_blk;
      int k = 0;
      for (int y = 0; y < g.H; y += b)
        for (int x = 0; x < g.W; x += b, ++k) {
          double p = x == 0 ? (k > 1 ? w[k - 2] : 0.0) : (x > b ? fmax(w[k - 2], w[k]) : w[k]);
          if (k > wb) p = fmax(p, w[k - 1 - wb]);
          if (k > 0 && w[k - 1] > p) w[k - 1] = p;
          if (x + b >= g.W && y + b >= g.H && k > wb) {
            p = fmax(w[k - 1], w[k - wb]);
            if (w[k] > p) w[k] = p;
          }
        }
    }
    double s = 0.0;
    for (int k = 0; k < g.n_blk; ++k) s += (double)blk[k * kXpBlockVals] * w[k];
    wsse[0] = s <= 0.0 ? 0ull : (unsigned long long)(s * g.A + 0.5);
    for (int p = 1; p < g.n_planes; ++p) {
      double sc = 0.0;
      for (int k = 0; k < g.nc_blk; ++k) sc += (double)blk[k * kXpBlockVals + 2 + p] * w[k];
      wsse[p] = sc <= 0.0 ? 0ull : (unsigned long long)(sc * g.A + 0.5);
    }
  }
  for (int p = 0; p < 3; ++p) {
    if (p < g.n_planes) {
      e[PQA_EXT3_XPSNR_Y + p] = xp_db(wsse[p], p ? g.Wc : g.W, p ? g.Hc : g.H, g.bit_depth);
      e[PQA_EXT3_WSSE + p] = (double)wsse[p];
    } else {
      e[PQA_EXT3_XPSNR_Y + p] = __builtin_nan("");
      e[PQA_EXT3_WSSE + p] = __builtin_nan("");
    }
  }
}

template <typename T, int BV>
hipError_t launch_xp_t(hipStream_t stream, const dim3 grid, const XpBlockArgs& a) {
  hipLaunchKernelGGL((xp_block_kernel<T, BV>), grid, dim3(kBlock), 0, stream, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_xpsnr_blocks(hipStream_t stream, Elem elem, const PlaneRun ref[3], const PlaneRun dis[3], int n_frames,
                               const void* h1, int64_t h1_pitch, const void* h2, int64_t h2_pitch, bool hfr,
                               const XpsnrGeometry& geo, unsigned long long* out) {
  if (n_frames <= 0) return hipSuccess;
  if (geo.n_blk <= 0 || geo.bsx + 4 > kXpLdsCols || geo.nc_blk > geo.n_blk) return hipErrorInvalidValue;
  if (geo.bv == 2 && ((geo.W | geo.H) & 1)) return hipErrorInvalidValue;   // the 2 x 2 loops would leave the block
  XpBlockArgs a{};
  for (int p = 0; p < geo.n_planes; ++p) {
    if (ref[p].row_pitch >= (1ll << 31) || dis[p].row_pitch >= (1ll << 31)) return hipErrorInvalidValue;
    a.ref[p] = ref[p].base; a.dis[p] = dis[p].base;
    a.rp_r[p] = (int)ref[p].row_pitch; a.fp_r[p] = ref[p].frame_pitch;
    a.rp_d[p] = (int)dis[p].row_pitch; a.fp_d[p] = dis[p].frame_pitch;
  }
  if (h1_pitch >= (1ll << 31) || h2_pitch >= (1ll << 31)) return hipErrorInvalidValue;
  a.h1 = h1; a.hp1 = (int)h1_pitch;
  a.h2 = h2; a.hp2 = (int)h2_pitch;
  a.hfr = hfr ? 1 : 0;
  a.g = geo;
  a.out = out;
  const dim3 grid(geo.n_blk, n_frames);
  const bool u8 = elem == ELEM_U8;
  if (elem != ELEM_U8 && elem != ELEM_U16) return hipErrorInvalidValue;
  if (geo.bv == 2) return u8 ? launch_xp_t<uint8_t, 2>(stream, grid, a) : launch_xp_t<uint16_t, 2>(stream, grid, a);
  return u8 ? launch_xp_t<uint8_t, 1>(stream, grid, a) : launch_xp_t<uint16_t, 1>(stream, grid, a);
}

hipError_t launch_xpsnr_finalize(hipStream_t stream, const XpFinalizeArgs& args) {
  if (args.n_frames <= 0) return hipSuccess;
  hipLaunchKernelGGL(xp_finalize_kernel, dim3(args.n_frames), dim3(64), 0, stream, args);
  return hipGetLastError();
}

}  // namespace pqa
