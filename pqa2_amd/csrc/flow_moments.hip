// Sub-pixel registration: tile-wise gradient moments (pqa_flow_moments / pqa_flow_moments_device; restated in
// tests/flow_ref.py; definition and bounds: DESIGN.md section 5).  With r = ref, d = dis, a = r + d, e = d - r, at every
// counted pixel 1 <= x <= W - 2, 1 <= y <= H - 2:
//
//   gx = Sobel-x of a,  gy = Sobel-y of a,  dt = (1 2 1) x (1 2 1) smoothing of e (weights sum to 16)
//   out[f][j][i][0..5] = sum over the counted pixels of tile (i, j) of  gx^2, gx gy, gy^2, gx dt, gy dt, dt^2
//
// Tile (i, j) owns the pixels with floor(x / T) = i, floor(y / T) = j, T in {8, 16, 32, 64}: the Lucas-Kanade normal
// equations of every tile, which align.solve_geometry turns into a shift and a scale.
//
// Work.  A workgroup of 256 threads owns a block of 64 x 64 pixels, (64 / T)^2 whole tiles.  It reads the block and its
// one-pixel halo from memory once -- 66 x 66 sample pairs, every index clamped to the plane -- into ONE LDS tile of packed
// dwords: a in the low half (unsigned, <= 2 (2^b - 1) < 2^16), e in the high half (signed, |e| < 2^15).  Lane x of wave w
// then walks column x of the rows 16 w ... 16 w + 15: a row costs three LDS reads (the dwords of x - 1, x, x + 1; consecutive
// lanes read consecutive dwords) and gives the three horizontal terms hd = a[x+1] - a[x-1], hs = a[x-1] + 2 a[x] + a[x+1],
// he = e[x-1] + 2 e[x] + e[x+1]; the three-row window of those lives in registers, and
//   gx = hd[y-1] + 2 hd[y] + hd[y+1],  gy = hs[y+1] - hs[y-1],  dt = he[y-1] + 2 he[y] + he[y+1].
// A pixel that is not counted contributes zeros (its clamped reads are never used by a counted pixel: a counted pixel's
// neighbours all lie inside the plane).
// Reduction, in a fixed order and without atomics: a lane adds the six products over a segment of S = min(T, 16) rows, the
// sums are widened to int64 and added over the T lanes of the tile's columns with xor shuffles, one lane writes the segment's
// six sums to LDS; after a barrier a thread per (tile, moment) adds the tile's T / S segments top to bottom and stores the
// result.  Integer sums: the result does not depend on order, base address, pitch or launch shape anyway.
// Bounds at b bits, m = 2^b - 1: a <= 2 m, |hd| <= 2 m, hs <= 8 m, |he| <= 4 m, |gx|, |gy| <= 8 m, |dt| <= 16 m.
//   8 bit: |gx| <= 2040, |dt| <= 4080, a product <= 4080^2 < 2^24, a lane's 16 of them < 2^28: int32 per lane.
//   12 bit: |gx| <= 32 760, |dt| <= 65 520: gx dt <= 2 146 435 200 < 2^31 but dt^2 = 4 292 870 400 > 2^31: products and lane
//   sums are int64 in the u16 instance (a sample above m is read as m so that the bounds hold).
//   A tile of 64 x 64 pixels sums at most 4096 * 65 520^2 < 2^45.
#include "plane_scan.h"

namespace pqa {
namespace {

constexpr int kFlowBlock = 64;               // pixels a workgroup covers each way
constexpr int kFlowLds = kFlowBlock + 2;     // with the halo
constexpr int kFlowPitch = kFlowLds + 1;     // dwords a row of the LDS tile
constexpr int kFlowRows = kFlowBlock / (kBlock / 64);   // rows a wave walks: 16

struct FlowArgs : PairPlanes {
  int tile, tx, ty, maxv;
  long long* out;   // [frame][ty][tx][6]
};

template <typename T> struct FlowAcc;
template <> struct FlowAcc<uint8_t> { using type = int; };
template <> struct FlowAcc<uint16_t> { using type = long long; };

__device__ __forceinline__ long long group_sum(long long v, int lanes) {
  for (int off = 1; off < lanes; off <<= 1) v += __shfl_xor(v, off, 64);
  return v;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void flow_moments_kernel(const FlowArgs a) {
  using Acc = typename FlowAcc<T>::type;
  __shared__ int px[kFlowLds * kFlowPitch];
  __shared__ long long part[8][8][6];   // [segment][tile column][moment]; T = 8: 8 segments of 8 rows, 8 tile columns
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int bx0 = blockIdx.x * kFlowBlock, by0 = blockIdx.y * kFlowBlock, f = blockIdx.z;
  const T* pr = (const T*)a.ref + (int64_t)f * a.ref_fp;
  const T* pd = (const T*)a.dis + (int64_t)f * a.dis_fp;

  for (int i = tid; i < kFlowLds * kFlowLds; i += kBlock) {
    const int r = i / kFlowLds, c = i - r * kFlowLds;
    const int y = min(max(by0 - 1 + r, 0), a.h - 1), x = min(max(bx0 - 1 + c, 0), a.w - 1);
    const int rv = min((int)pr[(int64_t)y * a.ref_rp + x], a.maxv), dv = min((int)pd[(int64_t)y * a.dis_rp + x], a.maxv);
    px[r * kFlowPitch + c] = ((rv + dv) & 0xffff) | (int)((unsigned)(dv - rv) << 16);
  }
  __syncthreads();

  // LDS row r holds plane row by0 - 1 + r, LDS column c plane column bx0 - 1 + c
  const auto hrow = [&](int r, int& hd, int& hs, int& he) {
    const int* p = px + r * kFlowPitch + lane;
    const int v0 = p[0], v1 = p[1], v2 = p[2];
    const int a0 = v0 & 0xffff, a1 = v1 & 0xffff, a2 = v2 & 0xffff;
    hd = a2 - a0;
    hs = a0 + 2 * a1 + a2;
    he = (v0 >> 16) + 2 * (v1 >> 16) + (v2 >> 16);
  };
  const int x = bx0 + lane, r0 = wv * kFlowRows;
  const bool col_counted = x >= 1 && x <= a.w - 2;
  const int seg_rows = a.tile < kFlowRows ? a.tile : kFlowRows;
  int hd_p, hs_p, he_p, hd_c, hs_c, he_c;
  hrow(r0, hd_p, hs_p, he_p);
  hrow(r0 + 1, hd_c, hs_c, he_c);
  Acc acc[6] = {};
#pragma unroll
  for (int k = 0; k < kFlowRows; ++k) {
    int hd_n, hs_n, he_n;
    hrow(r0 + k + 2, hd_n, hs_n, he_n);
    const int y = by0 + r0 + k;
    const bool counted = col_counted && y >= 1 && y <= a.h - 2;
    const int gx = counted ? hd_p + 2 * hd_c + hd_n : 0;
    const int gy = counted ? hs_n - hs_p : 0;
    const int dt = counted ? he_p + 2 * he_c + he_n : 0;
    acc[0] += (Acc)gx * gx;
    acc[1] += (Acc)gx * gy;
    acc[2] += (Acc)gy * gy;
    acc[3] += (Acc)gx * dt;
    acc[4] += (Acc)gy * dt;
    acc[5] += (Acc)dt * dt;
    hd_p = hd_c; hs_p = hs_c; he_p = he_c;
    hd_c = hd_n; hs_c = hs_n; he_c = he_n;
    if ((k & 7) == 7 && (k == kFlowRows - 1 || seg_rows == 8)) {   // the end of a segment
      const int seg = (r0 + k) / seg_rows;
#pragma unroll
      for (int m = 0; m < 6; ++m) {
        const long long s = group_sum((long long)acc[m], a.tile);
        if ((lane & (a.tile - 1)) == 0) part[seg][lane / a.tile][m] = s;
        acc[m] = 0;
      }
    }
  }
  __syncthreads();

  const int nt = kFlowBlock / a.tile, segs = a.tile / seg_rows;   // tiles each way in the block; segments a tile is high
  for (int i = tid; i < nt * nt * 6; i += kBlock) {   // T = 8: 384 sums
    const int m = i % 6, t = i / 6, ti = t % nt, tj = t / nt;
    const int gi = bx0 / a.tile + ti, gj = by0 / a.tile + tj;
    if (gi < a.tx && gj < a.ty) {
      long long s = 0;
      for (int k = 0; k < segs; ++k) s += part[tj * segs + k][ti][m];
      a.out[(((int64_t)f * a.ty + gj) * a.tx + gi) * 6 + m] = s;
    }
  }
}

}  // namespace

bool flow_tile_ok(int tile) { return tile == 8 || tile == 16 || tile == 32 || tile == 64; }

size_t flow_out_bytes(int w, int h, int tile, int n_frames) {
  return (size_t)n_frames * ((w + tile - 1) / tile) * ((h + tile - 1) / tile) * 6 * sizeof(long long);
}

hipError_t launch_flow_moments(hipStream_t stream, Elem elem, int bits, const void* ref, int64_t ref_row_pitch,
                               int64_t ref_frame_pitch, const void* dis, int64_t dis_row_pitch, int64_t dis_frame_pitch,
                               int n_frames, int w, int h, int tile, long long* out) {
  if (n_frames <= 0) return hipSuccess;
  FlowArgs a{};
  if (!flow_tile_ok(tile) || w < 3 || h < 3 ||
      !pair_planes(a, elem, bits, ref, ref_row_pitch, ref_frame_pitch, dis, dis_row_pitch, dis_frame_pitch, w, h))
    return hipErrorInvalidValue;
  a.tile = tile; a.tx = (w + tile - 1) / tile; a.ty = (h + tile - 1) / tile; a.maxv = (1 << bits) - 1;
  a.out = out;
  const dim3 grid((w + kFlowBlock - 1) / kFlowBlock, (h + kFlowBlock - 1) / kFlowBlock, n_frames);
  if (elem == ELEM_U8) hipLaunchKernelGGL(flow_moments_kernel<uint8_t>, grid, dim3(kBlock), 0, stream, a);
  else hipLaunchKernelGGL(flow_moments_kernel<uint16_t>, grid, dim3(kBlock), 0, stream, a);
  return hipGetLastError();
}

}  // namespace pqa
