// Distortion map: tile-wise second-order statistics of a frame pair (pqa_tile_moments / pqa_tile_moments_device; restated in
// tests/tile_ref.py; the solver is pqa2_amd/distortion.py).  With r = ref, d = dis (a u16 sample above top = 2^bits - 1 is
// read as top), for every tile (i, j) of T x T pixels, T in {8, 16, 32, 64}, x / T = i, y / T = j:
//
//   out[f][j][i][0..5] = sum r,  sum d,  sum r^2,  sum d^2,  sum r d,  sum |d - r|
//
// over the pixels of the tile that exist (edge tiles are smaller), exact uint64.  SSE = sum r^2 - 2 sum r d + sum d^2 is the
// host's to form.
//
// Work.  A workgroup of 256 threads owns a block of 64 x 64 pixels, (64 / T)^2 whole tiles; wave w owns its rows
// 16 w ... 16 w + 15.  Every sample is used once, so nothing goes through LDS: a lane owns 16 bytes of one row of both
// planes -- S = 16 samples of u8, 8 of u16 -- as four packed dwords each, so a row of the block is 64 / S = 4 (8) lanes and a
// wave covers 16 (8) rows at a time: one pass at 8 bit, two at 10 and 12 bit (both loaded before either is added up).
// The dwords arrive by one 16-byte load, four 4-byte loads or sample by sample, whichever the base addresses and pitches of
// BOTH planes allow (the host decides once per launch; a lane starts a multiple of 16 bytes into its row).  A lane whose 16
// bytes would cross the end of the row reads sample by sample and takes zeros past the end; a lane below the plane takes
// zeros.  A zero pair adds nothing to any of the six sums, so an edge tile holds the pixels that exist, and nothing beyond
// a row's last sample is touched.
// Sums of a lane, per half of 8 samples (a half never straddles a tile: 8 divides T):
//   8 bit:  v_dot4_u32_u8 of the packed bytes with themselves, each other and 0x01010101; v_sad_u8 for sum |d - r|.
//   10 / 12 bit: v_pk_min_u16 against top, then v_dot2_u32_u16 with themselves, each other and 0x00010001; v_sad_u16.
// Widening.  A lane's partial sums are uint32.  The largest is a sum of squares: n samples keep it below 2^32 while
//   n <= floor((2^32 - 1) / top^2) = 66 051 at 8 bit, 4 104 at 10 bit, 256 at 12 bit,
// that is 4 128, 513 and 32 rows of a lane's 16 (8) samples.  A lane adds at most one row at 8 bit and two at 10 / 12 bit
// before it hands its sums on (16 * 4095^2 < 2^28), so it never has to widen on the way.  What the lanes add up between
// them is wider at 10 / 12 bit -- a tile segment of 16 rows x 64 columns of 4095^2 is just below 2^34 -- so the u16 instance
// widens to uint64 before the first shuffle; at 8 bit the same segment stays below 1024 * 255^2 < 2^26 and the shuffles stay
// uint32.
// Reduction, in a fixed order and without atomics: a tile is cut into segments of min(T, 16) rows.  With T = 8 the two
// halves of a u8 lane belong to two tiles and are reduced separately, otherwise they are added first.  The lanes of a
// segment's columns (xor steps below T / S) and rows (xor steps of 64 / S lanes) are added with shuffles, one lane writes the
// segment's six sums to LDS; after a barrier a thread per (tile, sum) adds the tile's T / min(T, 16) segments top to bottom
// in uint64 and stores the result.  Every output word is written once: no zeroing.  A whole 64 x 64 tile of 4095^2 is below
// 2^36.  Integer sums: the result does not depend on order, base address, pitch, load width or launch shape.  No floating point.
#include "plane_scan.h"

namespace pqa {
namespace {

constexpr int kTileBlock = 64;   // pixels a workgroup covers each way
constexpr int kTileRows = kTileBlock / (kBlock / 64);   // rows of a wave: 16

struct TileArgs : PairPlanes {
  int tile, tx, ty;
  unsigned top2;   // top in both halves of a dword
  unsigned long long* out;   // [frame][ty][tx][6]
};

typedef unsigned short tile_u16x2 __attribute__((ext_vector_type(2)));

template <typename T> struct TileWide;
template <> struct TileWide<uint8_t> { using type = unsigned; };
template <> struct TileWide<uint16_t> { using type = unsigned long long; };

// adds the six sums of two dwords of packed samples to acc
template <typename T>
__device__ __forceinline__ void tile_add(unsigned (&acc)[6], unsigned r, unsigned d, unsigned top2) {
  if constexpr (sizeof(T) == 1) {
    acc[0] = __builtin_amdgcn_udot4(r, 0x01010101u, acc[0], false);
    acc[1] = __builtin_amdgcn_udot4(d, 0x01010101u, acc[1], false);
    acc[2] = __builtin_amdgcn_udot4(r, r, acc[2], false);
    acc[3] = __builtin_amdgcn_udot4(d, d, acc[3], false);
    acc[4] = __builtin_amdgcn_udot4(r, d, acc[4], false);
    acc[5] = __builtin_amdgcn_sad_u8(d, r, acc[5]);
  } else {
    const tile_u16x2 t = __builtin_bit_cast(tile_u16x2, top2), one = {1, 1};
    const tile_u16x2 rv = __builtin_elementwise_min(__builtin_bit_cast(tile_u16x2, r), t);
    const tile_u16x2 dv = __builtin_elementwise_min(__builtin_bit_cast(tile_u16x2, d), t);
    acc[0] = __builtin_amdgcn_udot2(rv, one, acc[0], false);
    acc[1] = __builtin_amdgcn_udot2(dv, one, acc[1], false);
    acc[2] = __builtin_amdgcn_udot2(rv, rv, acc[2], false);
    acc[3] = __builtin_amdgcn_udot2(dv, dv, acc[3], false);
    acc[4] = __builtin_amdgcn_udot2(rv, dv, acc[4], false);
    acc[5] = __builtin_amdgcn_sad_u16(__builtin_bit_cast(unsigned, dv), __builtin_bit_cast(unsigned, rv), acc[5]);
  }
}

// VB: bytes of one load
template <typename T, int VB>
__global__ __launch_bounds__(kBlock) void tile_moments_kernel(const TileArgs a) {
  using Wide = typename TileWide<T>::type;
  constexpr int S = 16 / (int)sizeof(T);     // samples of a lane
  constexpr int LPR = kTileBlock / S;        // lanes a row of the block: 4 / 8
  constexpr int RPW = 64 / LPR;              // rows a wave covers at a time: 16 / 8
  constexpr int P = kTileRows / RPW;         // passes of a wave: 1 / 2
  constexpr int NH = S / 8;                  // halves of 8 samples a lane: 2 / 1
  constexpr int DPH = 4 / NH;                // dwords a half
  __shared__ unsigned long long part[8][8][6];   // [segment][tile column][sum]; T = 8: 8 segments of 8 rows, 8 tile columns
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int bx0 = blockIdx.x * kTileBlock, by0 = blockIdx.y * kTileBlock, f = blockIdx.z;
  const T* pr = (const T*)a.ref + (int64_t)f * a.ref_fp;
  const T* pd = (const T*)a.dis + (int64_t)f * a.dis_fp;
  const int lrow = lane / LPR, xc = (lane % LPR) * S;   // the lane's row of a pass, its first column in the block
  const int seg_rows = a.tile < kTileRows ? a.tile : kTileRows;

  PackedQuad qr[P], qd[P];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int y = by0 + wv * kTileRows + p * RPW + lrow;
    if (y < a.h) {   // y >= 0, bx0 + xc >= 0; quad_load keeps x below w
      qr[p] = quad_load<T, VB, kTailZeros>(pr + (int64_t)y * a.ref_rp, bx0 + xc, a.w);
      qd[p] = quad_load<T, VB, kTailZeros>(pd + (int64_t)y * a.dis_rp, bx0 + xc, a.w);
    } else {
      qr[p] = PackedQuad{};
      qd[p] = PackedQuad{};
    }
  }

  unsigned acc[NH][6];
#pragma unroll
  for (int hh = 0; hh < NH; ++hh)
#pragma unroll
    for (int m = 0; m < 6; ++m) acc[hh][m] = 0u;
#pragma unroll
  for (int p = 0; p < P; ++p) {
#pragma unroll
    for (int k = 0; k < 4; ++k) tile_add<T>(acc[k / DPH], qr[p].d[k], qd[p].d[k], a.top2);
    if (p == P - 1 || seg_rows < kTileRows) {   // the end of a segment (wave-uniform)
      // the block row the lane's sums start at: with segments of 8 rows every pass is its own
      const int rb = wv * kTileRows + (seg_rows < kTileRows ? p * RPW : 0) + lrow;
      const int lane_rows = seg_rows < RPW ? seg_rows : RPW;   // rows of a segment that lie in different lanes
      const bool split = NH == 2 && a.tile == 8;               // the halves of a lane are two tiles
      if (NH == 2 && !split) {
#pragma unroll
        for (int m = 0; m < 6; ++m) acc[0][m] += acc[NH - 1][m];
      }
#pragma unroll
      for (int hh = 0; hh < NH; ++hh) {
        if (hh == 0 || split) {
          const int x = xc + hh * 8;
#pragma unroll
          for (int m = 0; m < 6; ++m) {
            Wide v = acc[hh][m];
            for (int off = 1; off * S < a.tile; off <<= 1) v += __shfl_xor(v, off, 64);
            for (int off = LPR; off < LPR * lane_rows; off <<= 1) v += __shfl_xor(v, off, 64);
            if (x % a.tile == 0 && rb % seg_rows == 0) part[rb / seg_rows][x / a.tile][m] = v;
          }
        }
#pragma unroll
        for (int m = 0; m < 6; ++m) acc[hh][m] = 0u;
      }
    }
  }
  __syncthreads();

  const int nt = kTileBlock / a.tile, segs = a.tile / seg_rows;   // tiles each way in the block; segments a tile is high
  for (int i = tid; i < nt * nt * 6; i += kBlock) {   // T = 8: 384 sums
    const int m = i % 6, t = i / 6, ti = t % nt, tj = t / nt;
    const int gi = bx0 / a.tile + ti, gj = by0 / a.tile + tj;
    if (gi < a.tx && gj < a.ty) {
      unsigned long long s = 0ull;
      for (int k = 0; k < segs; ++k) s += part[tj * segs + k][ti][m];
      a.out[(((int64_t)f * a.ty + gj) * a.tx + gi) * 6 + m] = s;
    }
  }
}

template <typename T, int VB>
hipError_t launch_v(hipStream_t stream, const TileArgs& a, int n_frames) {
  const dim3 grid((a.w + kTileBlock - 1) / kTileBlock, (a.h + kTileBlock - 1) / kTileBlock, n_frames);
  hipLaunchKernelGGL((tile_moments_kernel<T, VB>), grid, dim3(kBlock), 0, stream, a);
  return hipGetLastError();
}

}  // namespace

bool tile_size_ok(int tile) { return tile == 8 || tile == 16 || tile == 32 || tile == 64; }

size_t tile_out_bytes(int w, int h, int tile, int n_frames) {
  return (size_t)(n_frames > 0 ? n_frames : 0) * ((w + tile - 1) / tile) * ((h + tile - 1) / tile) * kTileSums *
         sizeof(unsigned long long);
}

hipError_t launch_tile_moments(hipStream_t stream, Elem elem, int bits, const void* ref, int64_t ref_row_pitch,
                               int64_t ref_frame_pitch, const void* dis, int64_t dis_row_pitch, int64_t dis_frame_pitch,
                               int n_frames, int w, int h, int tile, unsigned long long* out) {
  if (n_frames <= 0) return hipSuccess;
  TileArgs a{};
  if (!tile_size_ok(tile) ||
      !pair_planes(a, elem, bits, ref, ref_row_pitch, ref_frame_pitch, dis, dis_row_pitch, dis_frame_pitch, w, h))
    return hipErrorInvalidValue;
  a.tile = tile; a.tx = (w + tile - 1) / tile; a.ty = (h + tile - 1) / tile;
  a.top2 = ((1u << bits) - 1u) * 0x00010001u;
  a.out = out;
  return dispatch(elem, load_bytes(elem, a),
                  [&](auto t, auto vb) { return launch_v<decltype(t), decltype(vb)::value>(stream, a, n_frames); });
}

}  // namespace pqa
