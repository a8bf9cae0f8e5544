// VIF (4-scale separable-Gaussian pyramid + local mean/variance statistic) for gfx950.
//
// Arithmetic follows libvmaf's float extractor (vif.c compute_vif, vif_tools.c vif_filter1d_s /
// vif_filter1d_sq_s / vif_filter1d_xy_s / vif_dec2_s / vif_statistic_s) -- the code behind the
// reference's `libvmaf=` call site, app/vmaf_analyzer.py:373-419 -- restated in oracle/vmaf_oracle.c.
//
// Kernel shape (one workgroup = 4 waves = one TW x 8 output tile of one frame, TW = 240/248/252):
//   1. vertical pass: thread <-> column (TW + N - 1 <= 256 columns).  Each thread streams its column's
//      8 + N - 1 input rows with buffer loads whose row offset is an SGPR (coalesced row segments, zero
//      VALU address math), forms r, d, r*r, d*d, r*d and accumulates 4 row PAIRS x 5 signals with
//      v_pk_fma_f32: acc{2p,2p+1} += {c[k], c[k-1]} * {x, x} (tap pair from SGPRs, input broadcast), in
//      libvmaf's tap order.  The next scale's input (filter with the next kernel, keep even samples) is
//      accumulated from the same rows.  Results go to LDS as float2 = {row 2p, row 2p+1}.
//   2. horizontal pass: lane <-> (row pair, 4-column segment); ds_read_b128 of input pairs, conflict-free
//      by construction (see the lane map below); out{2p,2p+1}[o] += c[k] * in{2p,2p+1}[o+k].
//   3. statistic on the pair, DPP wave sum, one (num, den) double partial per tile; a fixed-order second
//      stage (finalize.hip) keeps a frame's record independent of batch size and rank count.
// HBM traffic: the two input planes once (halo re-reads hit L2) + the half-resolution planes written once.
//
// Which kernel runs where (launch_vif_stat at the bottom): scales 1-3: vif_strip_kernel where the launch is large enough for
// its segment rule (vif_strip_shape): the same tile, marched down a strip with the vertical window carried in registers;
// vif_stat_kernel (VALU) otherwise, and as the strip kernel's test partner (PQA_VIF_STRIP=0);
// scale 0 (8-, 10- and 12-bit clips): vif_s0_march_kernel in vif_march.hip (both filter passes on the f16 matrix cores), with
// vif_stat_kernel as its test partner (PQA_VIF_MFMA=0) and its fallback (no tap table, next-scale planes whose pitches its
// 16-byte stores cannot take).  The round-2 kernel that put only the vertical pass on the matrix cores left the build in
// round 4: tools/experiments/vif_s0_mfma_round2.hip.txt.
#include <cstring>
#include <mutex>
#include <vector>

#include <cstdio>
#include "kernels.h"
#include "pqa_device.h"

namespace pqa {

namespace {

struct Taps {
  float f[17];
};

static Taps gaussian_taps(int n) {
  // N taps, sigma = N/5, normalised in double, stored as float (libvmaf vif_filter1d_table).
  Taps t{};
  double v[17], sum = 0.0;
  const double sigma = n / 5.0;
  for (int k = 0; k < n; ++k) {
    const double d = k - n / 2;
    v[k] = exp(-0.5 * d * d / (sigma * sigma));
    sum += v[k];
  }
  for (int k = 0; k < n; ++k) t.f[k] = (float)(v[k] / sum);
  return t;
}

// Tap table of the packed vertical pass: ct[k] = {c[k], c[k-1]} with c[-1] = c[N] = 0, so one
// v_pk_fma_f32 with the input broadcast updates the two rows of a row pair in libvmaf's tap order.
struct TapPairs {
  f2 vt[18];  // vertical:   {c[k], c[k-1]}
  f2 ht[17];  // horizontal: {c[k], c[k]}  (ready-made SGPR pairs: no splat moves, no op_sel juggling)
  f2 dt[9];   // next scale's taps {c'[k], c'[k]} for the fused decimation
};

static TapPairs tap_pairs(const Taps& t, int n, const Taps* next, int n_next) {
  TapPairs p{};
  if (next)
    for (int k = 0; k < n_next; ++k) p.dt[k] = f2{next->f[k], next->f[k]};
  for (int k = 0; k <= n; ++k) {
    p.vt[k].x = k < n ? t.f[k] : 0.0f;
    p.vt[k].y = k > 0 ? t.f[k - 1] : 0.0f;
  }
  for (int k = 0; k < n; ++k) p.ht[k] = f2{t.f[k], t.f[k]};
  return p;
}

struct VifStatArgs {
  const void* ref;
  const void* dis;
  int64_t row_pitch_r, frame_pitch_r, row_pitch_d, frame_pitch_d;
  int w, h, tiles_x, n_tiles;
  int fold_w, fold_h;  // high-edge fold points of the border rule (pqa_device.h mirror_fold)
  float inv_scale, gain_limit;
  double* partials;
  // fused decimation (scale s -> s+1): filtered with the NEXT scale's taps, even samples kept
  float* dst_ref;
  float* dst_dis;
  int64_t dst_row_pitch_r, dst_frame_pitch_r, dst_row_pitch_d, dst_frame_pitch_d;
  TapPairs taps;
  int uniform;  // 0: every wave takes the general statistic (PQA_VIF_UNIFORM=0, the test partner of the all-high path)
};

constexpr int kP2 = 258;  // LDS row pitch in float2: == 2 (mod 32) -> conflict-free ds_read_b128 (see below)

// FP32 FMA throughput on gfx950 is 64 FLOP/clk/SIMD however it is issued (v_pk_fma_f32 every 4 clocks, plain
// v_fma_f32 every 2 with >= 2 waves per SIMD, f32 MFMA: tools/ubench/pk_vs_plain.hip, mfma_coissue.hip); the packed
// form halves the instruction count.  Everything hot is arranged as float2 = {row 2p, row 2p+1} of one column:
//   vertical pass:   acc{2p,2p+1} += {c[k], c[k-1]} * {x, x}     (tap PAIR from SGPRs, input broadcast)
//   horizontal pass: out{2p,2p+1}[o] += c[k] * in{2p,2p+1}[o+k]  (tap broadcast, input pair from LDS)

// Phases 1b (fused decimation), 2 (horizontal pass) and 3 (statistic + tile partial) of one TW x 8 tile whose
// vertical-pass results are in LDS: sv[signal][row pair][column] = {row 2p, row 2p+1}, sd[even row][column] =
// {ref, dis}.
template <int N, int TW, int ND>
__device__ __forceinline__ void vif_hstat(const VifStatArgs& a, const f2* sv /* [5][TH/2][kP2] */,
                                          const f2* sd /* [TH/2][kP2] */, double* red, int fr, int tile, int x0, int y0) {
  constexpr int R = N / 2, TH = kVifTileH, NSEG = TW / 4, NRP = TH / 2;
  constexpr int RD = ND / 2;
  const int tid = threadIdx.x;
  fr = __builtin_amdgcn_readfirstlane(fr); tile = __builtin_amdgcn_readfirstlane(tile);   // workgroup-uniform: keep
  x0 = __builtin_amdgcn_readfirstlane(x0); y0 = __builtin_amdgcn_readfirstlane(y0);       // the address math scalar
  // ---- 1b. fused decimation: horizontal pass at even columns, written straight to the next scale --
  if (ND) {
    const int ox0 = x0 >> 1, oy0 = y0 >> 1, ow = a.w >> 1, oh = a.h >> 1;
    // the tile's first output sample as a scalar address, the thread's place inside the tile as a 32-bit offset
    // in BYTES (global_store with an SGPR base and a 32-bit VGPR offset: no 64-bit VALU arithmetic; a tile spans 4 rows)
    float* __restrict__ tr = a.dst_ref + ((int64_t)fr * a.dst_frame_pitch_r + (int64_t)oy0 * a.dst_row_pitch_r + ox0);
    float* __restrict__ td = a.dst_dis + ((int64_t)fr * a.dst_frame_pitch_d + (int64_t)oy0 * a.dst_row_pitch_d + ox0);
    const unsigned rp_r = (unsigned)a.dst_row_pitch_r, rp_d = (unsigned)a.dst_row_pitch_d;
#pragma unroll
    for (int round = 0; round < 2; ++round) {
      const int item = tid + round * kBlock;
      const int oc = item & 127, orow = item >> 7;  // 128 slots per row, TW/2 of them used
      if (oc < TW / 2 && (ox0 + oc < ow && oy0 + orow < oh)) {
        f2 acc = f2{0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < ND; ++k) acc = __builtin_elementwise_fma(a.taps.dt[k], sd[orow * kP2 + 2 * oc + (R - RD) + k], acc);
        *reinterpret_cast<float*>(reinterpret_cast<char*>(tr) + ((unsigned)orow * rp_r + (unsigned)oc) * 4u) = acc.x;
        *reinterpret_cast<float*>(reinterpret_cast<char*>(td) + ((unsigned)orow * rp_d + (unsigned)oc) * 4u) = acc.y;
      }
    }
  }

  // ---- 2. horizontal pass + 3. statistic --------------------------------------------------------
  // lane l: row pair rp = l & 3, segment (4 columns) seg = 2*(s&3) + (wave&1) + 8*(s>>2) + 32*(wave>>1)
  // with s = l >> 2.  The row-pair pitch is 129 16-byte chunks (== 1 mod 16) and 2*seg == 4*s + const
  // (mod 16), so a lane's chunk index is l + const (mod 16): consecutive lanes hit consecutive chunks,
  // which is conflict-free for every ds_read_b128 lane group.
  const int wave = tid >> 6, lane = tid & 63;
  const int rp = lane & 3, sl = lane >> 2;
  const int seg = 2 * (sl & 3) + (wave & 1) + 8 * (sl >> 2) + 32 * (wave >> 1);
  float num = 0.0f, den = 0.0f;
  if (seg < NSEG) {
    constexpr int NCOL = 4 + N - 1, NREAD = (NCOL + 1) / 2;
    f2 out[5][4];
#pragma unroll
    for (int s = 0; s < 5; ++s) {
      f2 in[2 * NREAD];
      const f4* p = reinterpret_cast<const f4*>(&sv[(s * NRP + rp) * kP2 + seg * 4]);
#pragma unroll
      for (int q = 0; q < NREAD; ++q) {
        const f4 v = p[q];
        in[2 * q] = f2{v.x, v.y};
        in[2 * q + 1] = f2{v.z, v.w};
      }
      // tap-major order: the four outputs are independent chains, so consecutive v_pk_fma_f32 never
      // depend on each other (a dependent pair costs an s_nop); each output still sums taps 0..N-1 in order
#pragma unroll
      for (int o = 0; o < 4; ++o) out[s][o] = f2{0.0f, 0.0f};
#pragma unroll
      for (int k = 0; k < N; ++k)
#pragma unroll
        for (int o = 0; o < 4; ++o) out[s][o] = __builtin_elementwise_fma(a.taps.ht[k], in[o + k], out[s][o]);
      __builtin_amdgcn_sched_barrier(0);  // one signal's 10 ds_read_b128 in flight at a time, not all 50
    }
    const float sigma_nsq = 2.0f, eps = 1.0e-10f, sigma_max_inv = 4.0f / (255.0f * 255.0f);
    // validity as 0/1 weights folded into the accumulation (an fma instead of an add): no branches, and
    // out-of-image positions of edge tiles still hold finite values (mirrored real pixels)
    const int gyA = y0 + 2 * rp;
    const bool vrow[2] = {gyA < a.h, gyA + 1 < a.h};
    f2 num2 = f2{0.0f, 0.0f}, den2 = f2{0.0f, 0.0f};
    // the log terms of the sigma1_sq >= sigma_nsq branch are summed as the log of a product: per row of
    // the pair the four columns' arguments (each in [2, 2^16]) are multiplied first, so the thread takes
    // 6 v_log_f32 instead of 16 and needs no reciprocal for num's ratio (log a/b = log a - log b)
    f2 pn = f2{1.0f, 1.0f}, qn = f2{1.0f, 1.0f}, pd = f2{1.0f, 1.0f};
    // sigma1_sq of the lane's eight pixels first: one compare each and one ballot tell whether every pixel of the wave's
    // active lanes is inside the image and in the log branch.  Such a wave takes the statistic without its other branch: the
    // general path has s1h = s1 there and gden = s1 + eps IS s1 (eps = 1e-10 is below half an ulp of 2, 1.2e-7); wl = 0 with
    // `low` finite, so num2 and den2 stay +0.  The bits of the general path (tests/test_gpu_vif_uniform.py holds them to ==);
    // textured material is all-high wave by wave, flat sections and the edges between the two pay for both branches.
    // (The matching all-low path was built, is bit-identical too, and did not pay: DESIGN.md section 10.)
    f2 s1v[4];
    bool any_low = false;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      const f2 mu1 = out[0][o];
      s1v[o] = out[2][o] - mu1 * mu1;
      const bool lx = s1v[o].x < sigma_nsq, ly = s1v[o].y < sigma_nsq;
      any_low = any_low || lx || ly;
    }
    const bool cols_in = x0 + seg * 4 + 4 <= a.w;
    const bool rows_in = a.uniform && y0 + TH <= a.h;   // workgroup-uniform
    // (a ballot counts the active lanes only: lanes with seg >= NSEG are not here)
    const bool none_low = __builtin_amdgcn_ballot_w64(!cols_in || any_low) == 0ull;
    if (rows_in && none_low) {
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        const f2 mu1 = out[0][o], mu2 = out[1][o];
        const f2 s1 = s1v[o];
        f2 s2 = out[3][o] - mu2 * mu2;
        const f2 s12 = out[4][o] - mu1 * mu2;
        s2 = f2{fmaxf(s2.x, 0.0f), fmaxf(s2.y, 0.0f)};
        const f2 grcp = f2{fast_rcp(s1.x), fast_rcp(s1.y)};
        f2 g = s12 * grcp;
        g = __builtin_elementwise_fma(__builtin_elementwise_fma(-g, s1, s12), grcp, g);
        f2 sv = s2 - g * s12;
        sv = f2{fmaxf(sv.x, eps), fmaxf(sv.y, eps)};
        g = f2{__builtin_amdgcn_fmed3f(g.x, 0.0f, a.gain_limit), __builtin_amdgcn_fmed3f(g.y, 0.0f, a.gain_limit)};
        const f2 svn = sv + f2{sigma_nsq, sigma_nsq};
        const f2 narg = __builtin_elementwise_fma(g * g, s1, svn);
        const f2 darg = __builtin_elementwise_fma(s1, f2{1.0f / sigma_nsq, 1.0f / sigma_nsq}, f2{1.0f, 1.0f});
        pn *= narg;
        qn *= svn;
        pd *= darg;
        __builtin_amdgcn_sched_barrier(0);  // two pixels' worth of temporaries live at a time
      }
      num = (fast_log2(pn.x) - fast_log2(qn.x)) + (fast_log2(pn.y) - fast_log2(qn.y));
      den = fast_log2(pd.x) + fast_log2(pd.y);
    } else {
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        const bool vcol = (x0 + seg * 4 + o) < a.w;
        // the two rows of the pair go through the statistic together: every add / mul / fma is packed,
        // only max / min / select / rcp / log are per element
        const f2 mu1 = out[0][o], mu2 = out[1][o];
        const f2 s1 = s1v[o];
        f2 s2 = out[3][o] - mu2 * mu2;
        const f2 s12 = out[4][o] - mu1 * mu2;
        s2 = f2{fmaxf(s2.x, 0.0f), fmaxf(s2.y, 0.0f)};
        // validity and the branch choice: out-of-image positions of edge tiles hold finite values (mirrored real
        // pixels); they and the positions of the low branch contribute a factor 1 to the log products and a weight 0 / 1
        // to the low sums.  ONE select does it for all three products: with sigma1_sq replaced by 0 the arguments
        // become narg = svn (cancels against qn's svn) and darg = 1.  (A select costs the VALU as much as a packed FMA.)
        // libvmaf's MAX(sigma1_sq, 0) needs no instruction either: the log branch has sigma1_sq >= 2, everything else
        // continues with 0.
        const bool vx = vcol && vrow[0], vy = vcol && vrow[1];
        const bool hx = vx && !(s1.x < sigma_nsq), hy = vy && !(s1.y < sigma_nsq);
        const bool lx = vx && (s1.x < sigma_nsq), ly = vy && (s1.y < sigma_nsq);
        const f2 s1h = f2{hx ? s1.x : 0.0f, hy ? s1.y : 0.0f};
        // g = sigma12 / (sigma1_sq + eps): v_rcp_f32 plus one Newton correction -- exact 1.0 when the two
        // are equal (identical frames), 2 FMAs instead of a full IEEE division.  (Off the log branch g is sigma12 / eps:
        // large but finite, clamped below, and multiplied by s1h = 0.)
        const f2 gden = s1h + f2{eps, eps};
        const f2 grcp = f2{fast_rcp(gden.x), fast_rcp(gden.y)};
        f2 g = s12 * grcp;
        g = __builtin_elementwise_fma(__builtin_elementwise_fma(-g, gden, s12), grcp, g);
        f2 sv = s2 - g * s12;
        // vif_statistic_s also has `if (sigma1_sq < eps) {g = 0; sv_sq = sigma2_sq; sigma1_sq = 0}` and
        // `if (g < 0) {sv_sq = sigma2_sq; g = 0}`.  Both are dead for the result: the first implies
        // sigma1_sq < sigma_nsq and the second implies sigma12 < 0, and each of those overrides num/den below.
        // Its third override, `if (sigma2_sq < eps) {g = 0; sv_sq = 0}`, changes nothing measurable either: with
        // sigma2_sq < 1e-10 Cauchy-Schwarz bounds |sigma12| <= sqrt(sigma1_sq * 1e-10), so g^2 sigma1_sq <= 1e-10 next to
        // sv_sq + 2 in the log's argument, and sv_sq = sigma2_sq - g sigma12 lies within 1e-10 of 0 and is raised to eps
        // by the max below in both forms.  (Round 1 kept it as two compares and four selects per pixel pair.)
        sv = f2{fmaxf(sv.x, eps), fmaxf(sv.y, eps)};
        // clamp g to [0, gain_limit] with one v_med3_f32: the upper bound is vif_enhn_gain_limit, the lower
        // bound makes g*g = 0 when sigma12 < 0, i.e. num_val = log2(1) = 0 -- libvmaf's `if (sigma12 < 0) num_val = 0`
        g = f2{__builtin_amdgcn_fmed3f(g.x, 0.0f, a.gain_limit), __builtin_amdgcn_fmed3f(g.y, 0.0f, a.gain_limit)};
        const f2 svn = sv + f2{sigma_nsq, sigma_nsq};
        // num_val = log2(1 + g^2 sigma1_sq / (sv_sq + sigma_nsq)) = log2(narg) - log2(svn)
        const f2 narg = __builtin_elementwise_fma(g * g, s1h, svn);
        const f2 darg = __builtin_elementwise_fma(s1h, f2{1.0f / sigma_nsq, 1.0f / sigma_nsq}, f2{1.0f, 1.0f});
        const f2 low = __builtin_elementwise_fma(s2, f2{-sigma_max_inv, -sigma_max_inv}, f2{1.0f, 1.0f});
        pn *= narg;
        qn *= svn;
        pd *= darg;
        const f2 wl = f2{lx ? 1.0f : 0.0f, ly ? 1.0f : 0.0f};
        num2 = __builtin_elementwise_fma(wl, low, num2);
        den2 += wl;
        __builtin_amdgcn_sched_barrier(0);  // two pixels' worth of temporaries live at a time
      }
      num = (num2.x + num2.y) + ((fast_log2(pn.x) - fast_log2(qn.x)) + (fast_log2(pn.y) - fast_log2(qn.y)));
      den = (den2.x + den2.y) + (fast_log2(pd.x) + fast_log2(pd.y));
    }
  }
  {
    const float part[2] = {num, den};
    double v[2];
    block_sum_f32<2>(part, v, red);
    if (tid == 0) {
      double* out = a.partials + ((int64_t)fr * a.n_tiles + tile) * 2;
      out[0] = v[0];
      out[1] = v[1];
    }
  }
}

template <typename T, int N, int TW, int ND>
__global__ __launch_bounds__(kBlock, 3) void vif_stat_kernel(const VifStatArgs a) {
  constexpr int R = N / 2, TH = kVifTileH, COLS = TW + N - 1, NSEG = TW / 4, S = 8, NIN = S + N - 1;
  constexpr int RD = ND / 2;  // ND = taps of the next scale's filter (0: last scale, no decimation)
  static_assert(ND == 0 || RD <= R, "decimation window must sit inside the statistic window");
  static_assert(COLS <= 256 && COLS <= kP2, "one column per thread");
  static_assert(TW % 4 == 0 && NSEG <= 64 && TH == S, "segment map");
  __shared__ f2 sv[5][TH / 2][kP2];  // [signal][row pair][column] = {row 2p, row 2p+1}
  __shared__ f2 sd[ND ? TH / 2 : 1][ND ? kP2 : 1];  // decimation: [even row][column] = {ref, dis}
  __shared__ double red[12];

  const int tile = xcd_remap(blockIdx.x, a.n_tiles);
  const int tx = tile % a.tiles_x, ty = tile / a.tiles_x;
  const int fr = blockIdx.y;
  const T* __restrict__ ref = (const T*)a.ref + (int64_t)fr * a.frame_pitch_r;
  const T* __restrict__ dis = (const T*)a.dis + (int64_t)fr * a.frame_pitch_d;
  const int x0 = tx * TW, y0 = ty * TH;
  const int tid = threadIdx.x;

  // ---- 1. vertical pass: lane <-> column, wave-uniform row addressing ---------------------------
  {
    const int col = tid;   // one column per thread; the 8-row strip is the whole tile: rows are uniform
    constexpr int seg = 0;
    if (col < COLS) {
      const unsigned gx = (unsigned)mirror_fold(x0 - R + col, a.w, a.fold_w);
      const unsigned pitch_r = (unsigned)a.row_pitch_r, pitch_d = (unsigned)a.row_pitch_d;  // planes < 4 G samples
      const auto rsrc_r = make_rsrc(ref, (unsigned)a.h * pitch_r * (unsigned)sizeof(T));
      const auto rsrc_d = make_rsrc(dis, (unsigned)a.h * pitch_d * (unsigned)sizeof(T));
      f2 acc[S / 2][5];
#pragma unroll
      for (int p = 0; p < S / 2; ++p)
#pragma unroll
        for (int s = 0; s < 5; ++s) acc[p][s] = f2{0.0f, 0.0f};
      f2 dacc[S / 2];  // next-scale input at the strip's even rows, {ref, dis}
#pragma unroll
      for (int q = 0; q < S / 2; ++q) dacc[q] = f2{0.0f, 0.0f};
      // Input rows stream through in groups of G: the loads of group g+1 are in flight while group g is
      // consumed; sched_barrier keeps hipcc from hoisting all 2*NIN loads (and their r*r, d*d, r*d) to
      // the top, which costs ~120 VGPRs and a wave of occupancy.
#ifndef PQA_VIF_G
#define PQA_VIF_G 12   /* rows per load group: 2 groups at N = 17 (swept 4/6/8/12 on the box) */
#endif
      constexpr int G = PQA_VIF_G, NG = (NIN + G - 1) / G;
      T rn[G], dn[G];
      auto issue = [&](int g) {
#pragma unroll
        for (int i = 0; i < G; ++i) {
          const int j = g * G + i;
          if (j < NIN) {
            const unsigned gy = (unsigned)mirror_fold(y0 + seg * S - R + j, a.h, a.fold_h);
            // scalar frame base + 32-bit (row * pitch + column) lane offset -> global_load with an SGPR base
            // buffer_load: lane offset (column) in a VGPR, row offset in an SGPR -> no per-load VALU
            rn[i] = buf_load<T>(rsrc_r, gx, gy * pitch_r);
            dn[i] = buf_load<T>(rsrc_d, gx, gy * pitch_d);
          }
        }
      };
      issue(0);
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        T rc[G], dc[G];
#pragma unroll
        for (int i = 0; i < G; ++i) { rc[i] = rn[i]; dc[i] = dn[i]; }
        if (g + 1 < NG) issue(g + 1);
#pragma unroll
        for (int i = 0; i < G; ++i) {
          const int j = g * G + i;
          if (j < NIN) {
            const f2 x = PixIO<T>::pair(rc[i], dc[i], a.inv_scale);  // {r, d} - 128 (one v_pk_add / v_pk_fma)
            const f2 xx = x * x;                                      // {r*r, d*d}   (one v_pk_mul)
            const float r = x.x, d = x.y, rr = xx.x, dd = xx.y, rd = x.x * x.y;
            if (ND) {
#pragma unroll
              for (int q = 0; q < S / 2; ++q) {
                const int kd = j - (2 * q + R - RD);  // even row 2q, tap kd of the next scale's filter
                if (kd >= 0 && kd < ND) dacc[q] = __builtin_elementwise_fma(a.taps.dt[kd], x, dacc[q]);
              }
            }
#pragma unroll
            for (int p = 0; p < S / 2; ++p) {
              const int k = j - 2 * p;  // row 2p takes tap k, row 2p+1 tap k-1: both sum taps in increasing order
              if (k >= 0 && k <= N) {
                const f2 c = a.taps.vt[k];
                acc[p][0] = __builtin_elementwise_fma(c, f2{r, r}, acc[p][0]);
                acc[p][1] = __builtin_elementwise_fma(c, f2{d, d}, acc[p][1]);
                acc[p][2] = __builtin_elementwise_fma(c, f2{rr, rr}, acc[p][2]);
                acc[p][3] = __builtin_elementwise_fma(c, f2{dd, dd}, acc[p][3]);
                acc[p][4] = __builtin_elementwise_fma(c, f2{rd, rd}, acc[p][4]);
              }
            }
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int p = 0; p < S / 2; ++p)
#pragma unroll
        for (int s = 0; s < 5; ++s) sv[s][seg * (S / 2) + p][col] = acc[p][s];
      if (ND) {
#pragma unroll
        for (int q = 0; q < S / 2; ++q) sd[seg * (S / 2) + q][col] = dacc[q];
      }
    }
  }
  __syncthreads();

  vif_hstat<N, TW, ND>(a, &sv[0][0][0], &sd[0][0], red, fr, tile, x0, y0);
}

// ---- strip march (scales 1-3, f32 planes) --------------------------------------------------------
// One input row of the vertical pass in scatter form: row j of the current tile's window (plane row y0 - R + j) goes to every
// row pair it belongs to -- pair p of the current tile takes tap k = j - 2p, pair p of the tile below tap k - 8 -- and to the
// fused decimation's even rows likewise.  j is a constant after unrolling; rows arrive in increasing order, so every pair sees
// the FMAs of vif_stat_kernel in vif_stat_kernel's order (the zero halves at k = 0 and k = N included).
template <int N, int ND>
__device__ __forceinline__ void vif_strip_row(const TapPairs& taps, const int j, f2 x /* {ref, dis} */, f2 (&cur)[4][5],
                                              f2 (&cd)[4], f2 (&nxt)[4][5], f2 (&nd)[4]) {
  constexpr int R = N / 2, RD = ND / 2, S = kVifTileH;
  // the sample pair as ONE 64-bit register, whatever the vectoriser would rather pair up: {r, r}, {d, d} and the products'
  // broadcasts are then op_sel forms of v_pk_fma_f32; from lone 32-bit registers each broadcast costs two v_mov
  asm volatile("" : "+v"(x));
  const f2 xx = x * x;
  const float r = x.x, d = x.y, rr = xx.x, dd = xx.y, rd = x.x * x.y;
  if (ND) {
#pragma unroll
    for (int q = 0; q < S / 2; ++q) {
      const int kd = j - (2 * q + R - RD);
      if (kd >= 0 && kd < ND) cd[q] = __builtin_elementwise_fma(taps.dt[kd], x, cd[q]);
      if (kd - S >= 0 && kd - S < ND) nd[q] = __builtin_elementwise_fma(taps.dt[kd - S], x, nd[q]);
    }
  }
#pragma unroll
  for (int p = 0; p < S / 2; ++p) {
    const int k = j - 2 * p;
    if (k >= 0 && k <= N) {
      const f2 c = taps.vt[k];
      cur[p][0] = __builtin_elementwise_fma(c, f2{r, r}, cur[p][0]);
      cur[p][1] = __builtin_elementwise_fma(c, f2{d, d}, cur[p][1]);
      cur[p][2] = __builtin_elementwise_fma(c, f2{rr, rr}, cur[p][2]);
      cur[p][3] = __builtin_elementwise_fma(c, f2{dd, dd}, cur[p][3]);
      cur[p][4] = __builtin_elementwise_fma(c, f2{rd, rd}, cur[p][4]);
    }
    if (k - S >= 0 && k - S <= N) {
      const f2 c = taps.vt[k - S];
      nxt[p][0] = __builtin_elementwise_fma(c, f2{r, r}, nxt[p][0]);
      nxt[p][1] = __builtin_elementwise_fma(c, f2{d, d}, nxt[p][1]);
      nxt[p][2] = __builtin_elementwise_fma(c, f2{rr, rr}, nxt[p][2]);
      nxt[p][3] = __builtin_elementwise_fma(c, f2{dd, dd}, nxt[p][3]);
      nxt[p][4] = __builtin_elementwise_fma(c, f2{rd, rd}, nxt[p][4]);
    }
  }
}

// One step of the march: the 8 new rows of the window (j = N - 1 ... N + 6) complete the current tile's accumulators and start
// those of the tile below.
template <int N, int ND>
__device__ __forceinline__ void vif_strip_rows(const TapPairs& taps, const f2 (&xc)[8], f2 (&cur)[4][5], f2 (&cd)[4],
                                               f2 (&nxt)[4][5], f2 (&nd)[4]) {
  constexpr int NRP = kVifTileH / 2;
#pragma unroll
  for (int p = 0; p < NRP; ++p) {
#pragma unroll
    for (int s = 0; s < 5; ++s) nxt[p][s] = f2{0.0f, 0.0f};
    nd[p] = f2{0.0f, 0.0f};
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    vif_strip_row<N, ND>(taps, N - 1 + i, xc[i], cur, cd, nxt, nd);
    if (i & 1) __builtin_amdgcn_sched_barrier(0);   // two rows' products live at a time, not all eight
  }
}

// ... and the finished tile's accumulators go to LDS in vif_stat_kernel's layout.
template <int ND>
__device__ __forceinline__ void vif_strip_store(const f2 (&cur)[4][5], const f2 (&cd)[4], f2* sv, f2* sd, const int col) {
  constexpr int NRP = kVifTileH / 2;
#pragma unroll
  for (int p = 0; p < NRP; ++p)
#pragma unroll
    for (int s = 0; s < 5; ++s) sv[(s * NRP + p) * kP2 + col] = cur[p][s];
  if (ND) {
#pragma unroll
    for (int q = 0; q < NRP; ++q) sd[q * kP2 + col] = cd[q];
  }
}

// The kernel's VifStatArgs, read again from the kernel-argument segment (it is the first argument: offset 0).  The march keeps
// 60-odd scalar registers of state of its own; with all 48 tap registers resident beside them through the whole loop -- where
// loop-invariant loads end up -- the compiler spills scalars into lanes of a VGPR and fetches them back one v_readlane at a
// time, 70 VALU instructions a step.  Read through a pointer the optimiser cannot see through, the vertical taps are loaded
// (scalar cache) before the vertical pass and the horizontal ones before vif_hstat, and neither outlives its pass.
__device__ __forceinline__ const VifStatArgs& vif_strip_kernargs() {
  auto p = __builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return *(const VifStatArgs*)p;
}

// A workgroup owns one tile column (a strip) and seg_len consecutive tile rows of one frame and marches down them 8 output
// rows per step.  A step loads only the 8 rows that are new to the window (the first step's N - 1 rows above them are the
// prologue), forms x, x*x, r*d of a row once, and hands the rows the tile below shares to that tile's accumulators -- a second
// register set; the two sets swap roles from step to step, so nothing is copied.  The loads of step t + 1 are issued before
// step t's rows are consumed and fly under its FMAs, its horizontal pass and its statistic.  Everything behind the vertical
// pass is vif_hstat, and a tile's partial lands in vif_stat_kernel's slot: the records are vif_stat_kernel's bit for bit,
// whatever seg_len is (tests/test_gpu_vif_strip.py).
template <int N, int TW, int ND>
__global__ __launch_bounds__(kBlock, 3) void vif_strip_kernel(const VifStatArgs a, const int tiles_y, const int seg_len,
                                                              const int n_segs) {
  constexpr int R = N / 2, TH = kVifTileH, COLS = TW + N - 1, NSEG = TW / 4, S = 8;
  static_assert(ND == 0 || ND / 2 <= R, "decimation window must sit inside the statistic window");
  static_assert(COLS <= 256 && COLS <= kP2, "one column per thread");
  static_assert(TW % 4 == 0 && NSEG <= 64 && TH == S, "segment map");
  static_assert(N - 1 <= S, "the prologue fits one load group; a row feeds at most the tile below");
  __shared__ f2 sv[5][TH / 2][kP2];
  __shared__ f2 sd[ND ? TH / 2 : 1][ND ? kP2 : 1];
  __shared__ double red[12];

  const int wg = xcd_remap(blockIdx.x, a.tiles_x * n_segs);
  const int tx = wg % a.tiles_x, sg = wg / a.tiles_x;
  const int fr = blockIdx.y;
  const int ty0 = sg * seg_len, ty1 = min(ty0 + seg_len, tiles_y);
  const float* __restrict__ ref = (const float*)a.ref + (int64_t)fr * a.frame_pitch_r;
  const float* __restrict__ dis = (const float*)a.dis + (int64_t)fr * a.frame_pitch_d;
  const int x0 = tx * TW;
  // thread <-> column.  (The threads past COLS -- two, at scale 3 -- march along on a mirrored column into LDS columns nobody
  // reads, kP2 > 256: no divergent region, whose merges would keep the finished tile's registers alive across vif_hstat.)
  const int col = threadIdx.x;

  // formed once per segment: the lane's column offset, the row pitches and both descriptors
  const unsigned gx = (unsigned)mirror_fold(x0 - R + col, a.w, a.fold_w);
  const unsigned pitch_r = (unsigned)a.row_pitch_r, pitch_d = (unsigned)a.row_pitch_d;
  const auto rsrc_r = make_rsrc(ref, (unsigned)a.h * pitch_r * (unsigned)sizeof(float));
  const auto rsrc_d = make_rsrc(dis, (unsigned)a.h * pitch_d * (unsigned)sizeof(float));

  f2 accA[S / 2][5], accB[S / 2][5], dA[S / 2], dB[S / 2];
  f2 xn[S];   // the rows in flight, {ref, dis}: each load writes its half of the pair the vertical pass reads
  // the 8 new rows of the tile at y0: plane rows y0 + R ... y0 + R + 7, each folded on the scalar unit.
  // `more` = false (the segment's last step: nobody takes the rows) sends every lane past the end of the buffer instead of
  // branching round the loads: such a load fetches nothing and returns 0, and the step stays one basic block -- with a
  // branch in it the FMAs sink below the loads and the sample pairs cross the block boundary as lone registers.
  auto issue = [&](const int y0, const bool more) __attribute__((always_inline)) {
    const int ylo = y0 + R;
    const unsigned gxs = more ? gx : 0x3fffffffu;
    unsigned ro_r[S], ro_d[S];
    // (the pitches as values of this step: as loop invariants their eight multiples each are hoisted out of the march, and with
    // the taps resident the scalar registers do not hold them -- they come back lane by lane from a spill register)
    unsigned sp_r = pitch_r, sp_d = pitch_d;
    asm volatile("" : "+s"(sp_r), "+s"(sp_d));
#pragma unroll
    for (int i = 0; i < S; ++i) {
      const unsigned gy = (unsigned)mirror_fold(ylo + i, a.h, a.fold_h);   // as vif_stat_kernel folds it: same row, same sample
      ro_r[i] = gy * sp_r; ro_d[i] = gy * sp_d;
    }
#pragma unroll
    for (int i = 0; i < S; ++i) {
      xn[i].x = buf_load<float>(rsrc_r, gxs, ro_r[i]);
      xn[i].y = buf_load<float>(rsrc_d, gxs, ro_d[i]);
      // in the order the next step takes them: its waits then count down row by row, and the one that also covers this
      // step's stores (vmcnt(0): the tile partial of wave 0 among them) comes with the last row, not with the first
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  {
    // prologue: the N - 1 rows above the first step's, into the first tile's accumulators
    f2 px[N - 1];
#pragma unroll
    for (int j = 0; j < N - 1; ++j) {
      const unsigned gy = (unsigned)mirror_fold(ty0 * TH - R + j, a.h, a.fold_h);
      px[j].x = buf_load<float>(rsrc_r, gx, gy * pitch_r);
      px[j].y = buf_load<float>(rsrc_d, gx, gy * pitch_d);
    }
    issue(ty0 * TH, true);
#pragma unroll
    for (int p = 0; p < S / 2; ++p) {
#pragma unroll
      for (int s = 0; s < 5; ++s) accA[p][s] = accB[p][s] = f2{0.0f, 0.0f};
      dA[p] = dB[p] = f2{0.0f, 0.0f};
    }
#pragma unroll
    for (int j = 0; j < N - 1; ++j) vif_strip_row<N, ND>(a.taps, j, px[j], accA, dA, accB, dB);
  }

  auto step = [&](const int ty, f2 (&cur)[S / 2][5], f2 (&cd)[S / 2], f2 (&nxt)[S / 2][5], f2 (&nd)[S / 2]) __attribute__((always_inline)) {
    vif_strip_rows<N, ND>(vif_strip_kernargs().taps, xn, cur, cd, nxt, nd);
    // the next step's rows go into the registers this step's have left: in flight under the LDS hand-over and vif_hstat
    issue((ty + 1) * TH, ty + 1 < ty1);
    // LDS still holds the tile above until every wave is through its vif_hstat.  The wait stands here, behind this step's
    // FMAs, not at the end of the step before: wave 0's tail (the block sum, the tile partial) then runs beside the other
    // waves' vertical pass instead of holding them.
    __syncthreads();
    vif_strip_store<ND>(cur, cd, &sv[0][0][0], &sd[0][0], col);
    __syncthreads();
    // (likewise: what vif_hstat derives from the strip and the frame -- store bases, column predicates -- is formed per tile,
    // as in vif_stat_kernel, not kept in scalar registers through the vertical pass)
    int x0s = x0, frs = fr;
    asm volatile("" : "+s"(x0s), "+s"(frs));
    vif_hstat<N, TW, ND>(vif_strip_kernargs(), &sv[0][0][0], &sd[0][0], red, frs, ty * a.tiles_x + tx, x0s, ty * TH);
  };
  // two steps per trip: the register sets swap roles in the source, so only the set that is being filled for the tile below
  // is live across vif_hstat (one step per trip with a branch on the step's parity keeps both alive and spills)
  for (int ty = ty0; ty < ty1; ty += 2) {
    step(ty, accA, dA, accB, dB);
    if (ty + 1 >= ty1) break;
    step(ty + 1, accB, dB, accA, dA);
  }
}

template <int N, int TW, int ND>
hipError_t launch_strip_n(hipStream_t stream, const VifStatArgs& a, int n_frames, const int (&shape)[4]) {
  const dim3 grid(shape[0] * shape[3], n_frames), block(kBlock);
  hipLaunchKernelGGL((vif_strip_kernel<N, TW, ND>), grid, block, 0, stream, a, shape[1], shape[2], shape[3]);
  return hipGetLastError();
}

template <int N, int TW, int ND>
hipError_t launch_stat_n(hipStream_t stream, Elem elem, const VifStatArgs& a, int n_frames) {
  const dim3 grid(a.n_tiles, n_frames), block(kBlock);
  switch (elem) {
    case ELEM_U8: hipLaunchKernelGGL((vif_stat_kernel<uint8_t, N, TW, ND>), grid, block, 0, stream, a); break;
    case ELEM_U16: hipLaunchKernelGGL((vif_stat_kernel<uint16_t, N, TW, ND>), grid, block, 0, stream, a); break;
    case ELEM_F32: hipLaunchKernelGGL((vif_stat_kernel<float, N, TW, ND>), grid, block, 0, stream, a); break;
  }
  return hipGetLastError();
}

constexpr int kVifN[4] = {17, 9, 5, 3};
constexpr int kVifTW[4] = {240, 248, 252, 252};

}  // namespace

int vif_tile_w(int scale) { return kVifTW[scale]; }

void vif_strip_shape(int scale, int w, int h, int n_frames, int strip_seg, int* out) {
  const int strips = vif_tiles_x(scale, w), tiles_y = vif_tiles_y(h);
  int seg = 0;
  if (scale >= 1 && scale <= 3 && strip_seg > 0) {
    seg = strip_seg < tiles_y ? strip_seg : tiles_y;
  } else if (scale >= 1 && scale <= 3 && strip_seg == 0) {
    // Two costs pull the segment length apart.  A segment's first tile forms the window rows above it again and its last
    // step's hand-over goes to nobody (at scale 1 the prologue's FMAs are a sixth of a step's instructions); and a launch of
    // few long workgroups ends with CUs idle (a round is 3 workgroups on each of 256 CUs, and the last workgroups run alone).
    // Swept from 4 to 34 tile rows at 2160p (profiles/r27a_vif_strip_ab.txt), 9 was the fastest in both sweeps, 7 ... 14
    // within 3 % of it.  So: evenly long segments of at most 9 tile rows, shorter where the launch would otherwise have fewer
    // than eight rounds.  A launch too small for eight rounds of two-row segments keeps vif_stat_kernel.
    constexpr int kSegRows = 9;
    const double round = 3.0 * 256;
    for (int s = tiles_y < kSegRows ? tiles_y : kSegRows; s >= 2 && !seg; --s) {
      const int n = (tiles_y + s - 1) / s;
      if ((tiles_y + n - 1) / n != s) continue;   // as many segments come evenly shorter
      if ((double)strips * n * n_frames >= 8.0 * round) seg = s;
    }
  }
  const int n_segs = seg ? (tiles_y + seg - 1) / seg : 0;
  out[0] = strips; out[1] = tiles_y; out[2] = seg; out[3] = n_segs;
}

hipError_t launch_vif_stat(hipStream_t stream, int scale, Elem elem, PlaneRun ref, PlaneRun dis, int n_frames,
                           int w, int h, float inv_scale, float gain_limit, int border101, double* partials,
                           MutPlaneRun next_ref, MutPlaneRun next_dis, int s0_mode, int* n_partials, int uniform, int strip_seg) {
  if (n_partials) *n_partials = vif_tiles_x(scale, w) * vif_tiles_y(h);
  if (n_frames <= 0) return hipSuccess;
  // (the bit depth of 16-bit elements is recognised by the sample scale: 1/4 = 10 bit, 1/16 = 12 bit)
  const int bits = elem == ELEM_U8 ? 8 : (elem == ELEM_U16 && inv_scale == 0.25f) ? 10 : (elem == ELEM_U16 && inv_scale == 0.0625f) ? 12 : 0;
  if (scale == 0 && bits && s0_mode == VIF_S0_AUTO && next_ref.base && next_dis.base) {
    hipError_t err = hipSuccess;
    if (launch_vif_s0_march(stream, elem, bits, ref, dis, n_frames, w, h, gain_limit, border101, partials, next_ref, next_dis, n_partials, &err, uniform))
      return err;
    if (n_partials) *n_partials = vif_tiles_x(scale, w) * vif_tiles_y(h);
  }
  VifStatArgs a{};
  a.ref = ref.base; a.dis = dis.base;
  a.row_pitch_r = ref.row_pitch; a.frame_pitch_r = ref.frame_pitch;
  a.row_pitch_d = dis.row_pitch; a.frame_pitch_d = dis.frame_pitch;
  a.w = w; a.h = h;
  a.fold_w = 2 * w - (border101 ? 2 : 1); a.fold_h = 2 * h - (border101 ? 2 : 1);
  a.tiles_x = vif_tiles_x(scale, w);
  a.n_tiles = a.tiles_x * vif_tiles_y(h);
  a.inv_scale = inv_scale; a.gain_limit = gain_limit;
  a.uniform = uniform;
  a.partials = partials;
  a.dst_ref = (float*)next_ref.base; a.dst_dis = (float*)next_dis.base;
  a.dst_row_pitch_r = next_ref.row_pitch; a.dst_frame_pitch_r = next_ref.frame_pitch;
  a.dst_row_pitch_d = next_dis.row_pitch; a.dst_frame_pitch_d = next_dis.frame_pitch;
  const Taps cur = gaussian_taps(kVifN[scale]);
  const Taps nxt = scale < 3 ? gaussian_taps(kVifN[scale + 1]) : Taps{};
  a.taps = tap_pairs(cur, kVifN[scale], scale < 3 ? &nxt : nullptr, scale < 3 ? kVifN[scale + 1] : 0);
  if (scale < 3 && (!a.dst_ref || !a.dst_dis)) return hipErrorInvalidValue;
  if (elem == ELEM_F32 && scale >= 1) {
    int shape[4];
    vif_strip_shape(scale, w, h, n_frames, strip_seg, shape);
    if (shape[2]) switch (scale) {
      case 1: return launch_strip_n<9, 248, 5>(stream, a, n_frames, shape);
      case 2: return launch_strip_n<5, 252, 3>(stream, a, n_frames, shape);
      case 3: return launch_strip_n<3, 252, 0>(stream, a, n_frames, shape);
    }
  }
  switch (scale) {
    case 0: return launch_stat_n<17, 240, 9>(stream, elem, a, n_frames);
    case 1: return launch_stat_n<9, 248, 5>(stream, elem, a, n_frames);
    case 2: return launch_stat_n<5, 252, 3>(stream, elem, a, n_frames);
    case 3: return launch_stat_n<3, 252, 0>(stream, elem, a, n_frames);
  }
  return hipErrorInvalidValue;
}

}  // namespace pqa
