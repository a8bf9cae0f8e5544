// Temporal distortion: tile-wise second-order statistics of the frame DIFFERENCES of a clip pair (pqa_temporal_moments /
// pqa_temporal_moments_device; restated in tests/temporal_ref.py; the solver is pqa2_amd/temporal.py).  With R_f the reference
// and D_f the captured plane of frame f (a u16 sample above top = 2^bits - 1 is read as top), for every transition
// k = 1 ... n - 1 and every pixel
//
//   a = R_k - R_{k-1}     b = D_k - D_{k-1}     e = D_k - R_k                    (signed)
//   out[k-1][j][i][0..6] = sum a,  sum b,  sum a^2,  sum b^2,  sum a b,  sum a e,  sum e^2
//
// over the pixels of tile (i, j) of T x T pixels, T in {8, 16, 32, 64}, x / T = i, y / T = j, that exist (edge tiles are
// smaller), exact: words 0, 1, 4, 5 are int64 in two's complement, words 2, 3, 6 uint64.
//
// Work: that of tile_moments.hip with four planes where it has two.  A workgroup of 256 threads owns a block of 64 x 64 pixels
// of one transition at a time, wave w its rows 16 w ... 16 w + 15; a lane owns 16 bytes of one row of the four planes
// R_k, R_{k-1}, D_k, D_{k-1} -- 16 samples of u8, 8 of u16 -- as four packed dwords each: one pass at 8 bit, two at 10 / 12 bit
// (all loaded before any is added up).  The dwords arrive by one 16-byte load, four 4-byte loads or sample by sample, whichever
// the base addresses and pitches of BOTH clips allow (load_bytes of plane_scan.h).  A lane whose 16 bytes would cross
// the end of the row reads sample by sample and takes zeros past the end; a lane below the plane takes zeros.  A zero in all
// four planes adds nothing to any sum, so an edge tile holds the pixels that exist and nothing past a row's last sample is
// touched.
// Which form.  All seven sums are bilinear in the four planes.  This kernel forms the PRODUCTS OF THE RAW SAMPLES and combines
// them afterwards: four plain sums and the ten products R_k R_k, R_k R_{k-1}, R_{k-1} R_{k-1}, D_k D_k, D_k D_{k-1},
// D_{k-1} D_{k-1}, R_k D_k, R_k D_{k-1}, R_{k-1} D_k, R_{k-1} D_{k-1}, 14 v_dot4_u32_u8 (v_dot2_u32_u16) a dword of each plane.
// The other form -- differences first, signed dot products -- loses at 8 bit: a difference of two bytes needs nine bits, so it
// does not fit the i8 lanes of v_dot4_i32_i8; the bytes would be unpacked to i16 pairs (eight moves a dword quadruple), three
// packed subtractions formed and the seven sums taken with 14 v_dot2_i32_i16 -- the same number of dots for HALF the samples
// each, plus the unpacking.  At 10 / 12 bit the differences fit an i16 and that form would issue fewer instructions (four
// v_pk_min_u16, three packed subtractions and seven signed dots a dword of each plane against four minima and 14 dots here);
// it was not built: one form serves every depth with one widening argument, and the 16-byte loads of four planes, not the
// dots, are what a lane waits for.
// Which traversal.  Both were built.  By default blockIdx.z is the transition: a workgroup reads its block of four planes, so a
// frame that two transitions share is read twice (the second time mostly from the L2 / MALL), every launch has as many
// workgroups as tile_moments has a pair, and nothing is carried from one transition to the next.  With PQA_TEMPORAL_WALK=1
// (read at pqa_create; WALK below) blockIdx.z is 0 and a workgroup walks through the launch's transitions with its block of
// the previous pair in registers: two planes a transition, but an eighth of the workgroups and a barrier pair a step.
// Measured on 8 resident pairs at T = 64 (profiles/r23a_temporal_times.txt, two runs): the default takes 8.7 / 9.9 us a
// transition at 1080p (8 / 10 bit) where the walk takes 9.9 / 10.6, and 20.8 / 24.0 us at 2160p where the walk takes 20.0 / 22.6
// -- 10 % ahead at 1080p, 4 ... 6 % behind at 2160p, both 1.14 ... 1.34 times pqa_tile_moments_device on the same planes.  The
// default was kept for every size: it is the simpler one and the one ahead where a launch has the fewest workgroups; the
// walk stays as its A/B partner and returns the same words (tests/test_gpu_temporal_moments.py).
// Widening.  A lane's 14 raw sums are uint32.  Before it hands them on a lane has added n = 16 samples (one row of 16 at
// 8 bit, two rows of 8 at 10 / 12 bit), so a raw sum lies in [0, n top^2] = [0, 1 040 400] at 8 bit, [0, 16 744 464] at 10 bit
// and [0, 268 304 400] < 2^28 at 12 bit.  The lane combines them in int32:
//   sum a = sR_k - sR_{k-1}                                 sum b likewise                 |.| <= n top     < 2^16
//   sum a^2 = R_k R_k - 2 R_k R_{k-1} + R_{k-1} R_{k-1}      sum b^2, sum e^2 likewise      in [0, n top^2], no partial of the
//     evaluation order (x + z) - 2 y leaves [-2 n top^2, 2 n top^2], |.| < 2^30
//   sum a b = (R_k D_k + R_{k-1} D_{k-1}) - (R_k D_{k-1} + R_{k-1} D_k)                    |.| <= n top^2, partials in
//   sum a e = (R_k D_k + R_k R_{k-1}) - (R_k R_k + R_{k-1} D_k)                            [0, 2 n top^2] < 2^30
// so int32 never wraps.  What the lanes add up between them is wider at 10 / 12 bit -- a tile segment of 16 rows x 64 columns of
// 4095^2 is just below 2^34 -- so the u16 instance widens to int64 before the first shuffle; at 8 bit the same segment stays
// within 1024 * 255^2 < 2^26 in magnitude and the shuffles stay int32.
// Reduction, in a fixed order and without atomics, as in tile_moments.hip: a tile is cut into segments of min(T, 16) rows; with
// T = 8 the two halves of a u8 lane belong to two tiles and are reduced separately, otherwise they are added first.  The lanes
// of a segment's columns and rows are added with xor shuffles, one lane writes the segment's seven sums to LDS; after a
// barrier a thread per (tile, sum) adds the tile's segments top to bottom in int64 and stores the word.  Every output word is
// written once: no zeroing.  A whole 64 x 64 tile of 4095^2 is below 2^36.  Integer sums: the result does not depend on order,
// base address, pitch, load width or launch shape.  No floating point.
#include "plane_scan.h"

namespace pqa {
namespace {

constexpr int kTmpBlock = 64;   // pixels a workgroup covers each way
constexpr int kTmpRows = kTmpBlock / (kBlock / 64);   // rows of a wave: 16
constexpr int kTmpRaw = 14;     // raw sums of a lane

struct TemporalArgs : PairPlanes {
  int tile, tx, ty, n_trans;
  unsigned top2;   // top in both halves of a dword
  unsigned long long* out;   // [transition][ty][tx][7]
};

typedef unsigned short tmp_u16x2 __attribute__((ext_vector_type(2)));

template <typename T> struct TmpWide;
template <> struct TmpWide<uint8_t> { using type = int; };
template <> struct TmpWide<uint16_t> { using type = long long; };

// adds the 14 raw sums of one dword of packed samples of each plane to acc: rk / rp: R_k / R_{k-1}, dk / dp: D_k / D_{k-1}
template <typename T>
__device__ __forceinline__ void tmp_add(unsigned (&acc)[kTmpRaw], unsigned rk, unsigned rp, unsigned dk, unsigned dp, unsigned top2) {
  if constexpr (sizeof(T) == 1) {
    acc[0] = __builtin_amdgcn_udot4(rk, 0x01010101u, acc[0], false);
    acc[1] = __builtin_amdgcn_udot4(rp, 0x01010101u, acc[1], false);
    acc[2] = __builtin_amdgcn_udot4(dk, 0x01010101u, acc[2], false);
    acc[3] = __builtin_amdgcn_udot4(dp, 0x01010101u, acc[3], false);
    acc[4] = __builtin_amdgcn_udot4(rk, rk, acc[4], false);
    acc[5] = __builtin_amdgcn_udot4(rk, rp, acc[5], false);
    acc[6] = __builtin_amdgcn_udot4(rp, rp, acc[6], false);
    acc[7] = __builtin_amdgcn_udot4(dk, dk, acc[7], false);
    acc[8] = __builtin_amdgcn_udot4(dk, dp, acc[8], false);
    acc[9] = __builtin_amdgcn_udot4(dp, dp, acc[9], false);
    acc[10] = __builtin_amdgcn_udot4(rk, dk, acc[10], false);
    acc[11] = __builtin_amdgcn_udot4(rk, dp, acc[11], false);
    acc[12] = __builtin_amdgcn_udot4(rp, dk, acc[12], false);
    acc[13] = __builtin_amdgcn_udot4(rp, dp, acc[13], false);
  } else {
    const tmp_u16x2 t = __builtin_bit_cast(tmp_u16x2, top2), one = {1, 1};
    const tmp_u16x2 a = __builtin_elementwise_min(__builtin_bit_cast(tmp_u16x2, rk), t);
    const tmp_u16x2 b = __builtin_elementwise_min(__builtin_bit_cast(tmp_u16x2, rp), t);
    const tmp_u16x2 c = __builtin_elementwise_min(__builtin_bit_cast(tmp_u16x2, dk), t);
    const tmp_u16x2 e = __builtin_elementwise_min(__builtin_bit_cast(tmp_u16x2, dp), t);
    acc[0] = __builtin_amdgcn_udot2(a, one, acc[0], false);
    acc[1] = __builtin_amdgcn_udot2(b, one, acc[1], false);
    acc[2] = __builtin_amdgcn_udot2(c, one, acc[2], false);
    acc[3] = __builtin_amdgcn_udot2(e, one, acc[3], false);
    acc[4] = __builtin_amdgcn_udot2(a, a, acc[4], false);
    acc[5] = __builtin_amdgcn_udot2(a, b, acc[5], false);
    acc[6] = __builtin_amdgcn_udot2(b, b, acc[6], false);
    acc[7] = __builtin_amdgcn_udot2(c, c, acc[7], false);
    acc[8] = __builtin_amdgcn_udot2(c, e, acc[8], false);
    acc[9] = __builtin_amdgcn_udot2(e, e, acc[9], false);
    acc[10] = __builtin_amdgcn_udot2(a, c, acc[10], false);
    acc[11] = __builtin_amdgcn_udot2(a, e, acc[11], false);
    acc[12] = __builtin_amdgcn_udot2(b, c, acc[12], false);
    acc[13] = __builtin_amdgcn_udot2(b, e, acc[13], false);
  }
}

// the seven sums from a lane's 14 raw ones (each below 2^28: the head comment has the intervals)
__device__ __forceinline__ void tmp_combine(const unsigned (&q)[kTmpRaw], int (&v)[kTemporalSums]) {
  const int sRk = (int)q[0], sRp = (int)q[1], sDk = (int)q[2], sDp = (int)q[3];
  const int RkRk = (int)q[4], RkRp = (int)q[5], RpRp = (int)q[6], DkDk = (int)q[7], DkDp = (int)q[8], DpDp = (int)q[9];
  const int RkDk = (int)q[10], RkDp = (int)q[11], RpDk = (int)q[12], RpDp = (int)q[13];
  v[0] = sRk - sRp;
  v[1] = sDk - sDp;
  v[2] = (RkRk + RpRp) - 2 * RkRp;
  v[3] = (DkDk + DpDp) - 2 * DkDp;
  v[4] = (RkDk + RpDp) - (RkDp + RpDk);
  v[5] = (RkDk + RkRp) - (RkRk + RpDk);
  v[6] = (DkDk + RkRk) - 2 * RkDk;
}

// the lane's 16 bytes of its P rows of one frame pair
template <typename T, int VB, int P, int RPW>
__device__ __forceinline__ void tmp_load_pair(const TemporalArgs& a, int f, int y0, int x, PackedQuad (&qr)[P], PackedQuad (&qd)[P]) {
  const T* pr = (const T*)a.ref + (int64_t)f * a.ref_fp;
  const T* pd = (const T*)a.dis + (int64_t)f * a.dis_fp;
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int y = y0 + p * RPW;
    if (y < a.h) {   // y >= 0, x >= 0; quad_load keeps x below w
      qr[p] = quad_load<T, VB, kTailZeros>(pr + (int64_t)y * a.ref_rp, x, a.w);
      qd[p] = quad_load<T, VB, kTailZeros>(pd + (int64_t)y * a.dis_rp, x, a.w);
    } else {
      qr[p] = PackedQuad{};
      qd[p] = PackedQuad{};
    }
  }
}

// VB: bytes of one load.  WALK: the workgroup walks through the launch's transitions with its block of the previous pair in
// registers (blockIdx.z is 0); otherwise blockIdx.z is the transition
template <typename T, int VB, bool WALK>
__global__ __launch_bounds__(kBlock) void temporal_moments_kernel(const TemporalArgs a) {
  using Wide = typename TmpWide<T>::type;
  constexpr int S = 16 / (int)sizeof(T);     // samples of a lane
  constexpr int LPR = kTmpBlock / S;         // lanes a row of the block: 4 / 8
  constexpr int RPW = 64 / LPR;              // rows a wave covers at a time: 16 / 8
  constexpr int P = kTmpRows / RPW;          // passes of a wave: 1 / 2
  constexpr int NH = S / 8;                  // halves of 8 samples a lane: 2 / 1
  constexpr int DPH = 4 / NH;                // dwords a half
  __shared__ long long part[8][8][kTemporalSums];   // [segment][tile column][sum]; T = 8: 8 segments of 8 rows, 8 tile columns
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int bx0 = blockIdx.x * kTmpBlock, by0 = blockIdx.y * kTmpBlock;
  const int lrow = lane / LPR, xc = (lane % LPR) * S;   // the lane's row of a pass, its first column in the block
  const int seg_rows = a.tile < kTmpRows ? a.tile : kTmpRows;
  const int y0 = by0 + wv * kTmpRows + lrow;
  const int tr0 = WALK ? 0 : blockIdx.z, tr1 = WALK ? a.n_trans : tr0 + 1;   // transition tr: frames tr and tr + 1

  PackedQuad qrk[P], qrp[P], qdk[P], qdp[P];
  tmp_load_pair<T, VB, P, RPW>(a, tr0, y0, bx0 + xc, qrp, qdp);
  for (int tr = tr0; tr < tr1; ++tr) {
    tmp_load_pair<T, VB, P, RPW>(a, tr + 1, y0, bx0 + xc, qrk, qdk);

    unsigned acc[NH][kTmpRaw];
#pragma unroll
    for (int hh = 0; hh < NH; ++hh)
#pragma unroll
      for (int m = 0; m < kTmpRaw; ++m) acc[hh][m] = 0u;
#pragma unroll
    for (int p = 0; p < P; ++p) {
#pragma unroll
      for (int k = 0; k < 4; ++k) tmp_add<T>(acc[k / DPH], qrk[p].d[k], qrp[p].d[k], qdk[p].d[k], qdp[p].d[k], a.top2);
      if (p == P - 1 || seg_rows < kTmpRows) {   // the end of a segment (wave-uniform)
        // the block row the lane's sums start at: with segments of 8 rows every pass is its own
        const int rb = wv * kTmpRows + (seg_rows < kTmpRows ? p * RPW : 0) + lrow;
        const int lane_rows = seg_rows < RPW ? seg_rows : RPW;   // rows of a segment that lie in different lanes
        const bool split = NH == 2 && a.tile == 8;               // the halves of a lane are two tiles
        if (NH == 2 && !split) {
#pragma unroll
          for (int m = 0; m < kTmpRaw; ++m) acc[0][m] += acc[NH - 1][m];
        }
#pragma unroll
        for (int hh = 0; hh < NH; ++hh) {
          if (hh == 0 || split) {
            const int x = xc + hh * 8;
            int sums[kTemporalSums];
            tmp_combine(acc[hh], sums);
#pragma unroll
            for (int m = 0; m < kTemporalSums; ++m) {
              Wide v = sums[m];
              for (int off = 1; off * S < a.tile; off <<= 1) v += __shfl_xor(v, off, 64);
              for (int off = LPR; off < LPR * lane_rows; off <<= 1) v += __shfl_xor(v, off, 64);
              if (x % a.tile == 0 && rb % seg_rows == 0) part[rb / seg_rows][x / a.tile][m] = v;
            }
          }
#pragma unroll
          for (int m = 0; m < kTmpRaw; ++m) acc[hh][m] = 0u;
        }
      }
    }
    __syncthreads();

    const int nt = kTmpBlock / a.tile, segs = a.tile / seg_rows;   // tiles each way in the block; segments a tile is high
    for (int i = tid; i < nt * nt * kTemporalSums; i += kBlock) {   // T = 8: 448 sums
      const int m = i % kTemporalSums, t = i / kTemporalSums, ti = t % nt, tj = t / nt;
      const int gi = bx0 / a.tile + ti, gj = by0 / a.tile + tj;
      if (gi < a.tx && gj < a.ty) {
        long long s = 0;
        for (int k = 0; k < segs; ++k) s += part[tj * segs + k][ti][m];
        a.out[(((int64_t)tr * a.ty + gj) * a.tx + gi) * kTemporalSums + m] = (unsigned long long)s;
      }
    }
    if (WALK) {
      __syncthreads();   // the next transition writes `part` again
#pragma unroll
      for (int p = 0; p < P; ++p) {
        qrp[p] = qrk[p];
        qdp[p] = qdk[p];
      }
    }
  }
}

template <typename T, int VB>
hipError_t launch_v(hipStream_t stream, const TemporalArgs& a, bool walk) {
  const dim3 grid((a.w + kTmpBlock - 1) / kTmpBlock, (a.h + kTmpBlock - 1) / kTmpBlock, walk ? 1 : a.n_trans);
  if (walk) hipLaunchKernelGGL((temporal_moments_kernel<T, VB, true>), grid, dim3(kBlock), 0, stream, a);
  else hipLaunchKernelGGL((temporal_moments_kernel<T, VB, false>), grid, dim3(kBlock), 0, stream, a);
  return hipGetLastError();
}

}  // namespace

size_t temporal_out_bytes(int w, int h, int tile, int n_frames) {
  return (size_t)(n_frames > 1 ? n_frames - 1 : 0) * ((w + tile - 1) / tile) * ((h + tile - 1) / tile) * kTemporalSums *
         sizeof(unsigned long long);
}

hipError_t launch_temporal_moments(hipStream_t stream, Elem elem, int bits, const void* ref, int64_t ref_row_pitch,
                                   int64_t ref_frame_pitch, const void* dis, int64_t dis_row_pitch, int64_t dis_frame_pitch,
                                   int n_frames, int w, int h, int tile, bool walk, unsigned long long* out) {
  if (n_frames <= 1) return hipSuccess;
  TemporalArgs a{};
  if (!tile_size_ok(tile) ||
      !pair_planes(a, elem, bits, ref, ref_row_pitch, ref_frame_pitch, dis, dis_row_pitch, dis_frame_pitch, w, h))
    return hipErrorInvalidValue;
  a.tile = tile; a.tx = (w + tile - 1) / tile; a.ty = (h + tile - 1) / tile;
  a.n_trans = n_frames - 1;
  a.top2 = ((1u << bits) - 1u) * 0x00010001u;
  a.out = out;
  return dispatch(elem, load_bytes(elem, a),
                  [&](auto t, auto vb) { return launch_v<decltype(t), decltype(vb)::value>(stream, a, walk); });
}

}  // namespace pqa
