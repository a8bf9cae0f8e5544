// Field alignment: field-against-field squared errors of a clip pair (pqa_field_moments / pqa_field_moments_device; restated
// in tests/field_ref.py; the solver is pqa2_amd/fields.py).  With R_f the reference and D_f the captured plane of frame f (a
// u16 sample above top = 2^bits - 1 is read as top), h2 = floor(h / 2) row pairs (the last row of an odd-height plane is
// counted nowhere) and
//
//   E(A, p, B, q) = sum_{i < h2} sum_{x < w} (A[2 i + p][x] - B[2 i + q][x])^2        p, q in {0, 1}
//
// every transition k = 1 ... n - 1 has 14 exact uint64 words:
//
//   out[k-1][2 p + q]      = E(D_k, p, R_k, q)          the captured field p against the reference field q of the same frame
//   out[k-1][4 + 2 p + q]  = E(D_k, p, R_{k-1}, q)      ... of the PREVIOUS reference frame
//   out[k-1][8 + 2 p + q]  = E(D_{k-1}, p, R_k, q)      the previous captured frame's field against THIS reference frame
//   out[k-1][12]           = E(D_k, 0, D_k, 1)          comb of the captured frame
//   out[k-1][13]           = E(R_k, 0, R_k, 1)          comb of the reference frame
//
// Work.  A workgroup of 256 threads owns a block of kFieldCols = 128 columns by kFieldRows = 128 rows (64 row pairs) of one
// transition (blockIdx.z).  A lane owns 16 bytes -- 16 samples of u8, 8 of u16 -- of a ROW PAIR (rows 2 i and 2 i + 1) of the four
// planes R_k, R_{k-1}, D_k, D_{k-1}: eight packed quads, because the cross-parity products need both rows in one lane.  The
// 128 columns take 8 (u8) / 16 (u16) lanes, so the workgroup covers 32 / 16 row pairs at a time and its block in P = 2 / 4
// passes.  The dwords arrive by one 16-byte load, four 4-byte loads or sample by sample, whichever the base addresses and
// pitches of BOTH clips allow (load_bytes of plane_scan.h).  A lane whose 16 bytes would cross the end of the row reads sample
// by sample and takes zeros past the end; a lane whose row pair is not in the plane takes zeros.  A zero in all eight rows adds
// nothing to any product, so nothing past a row's last sample and no row from 2 h2 on is touched.
// Which form.  All 14 words are bilinear in the eight row vectors.  The kernel forms the PRODUCTS OF THE RAW SAMPLES: the 8
// norms and the 14 cross products D_k[p] R_k[q], D_k[p] R_{k-1}[q], D_{k-1}[p] R_k[q], D_k[0] D_k[1], R_k[0] R_k[1] -- 22
// v_dot4_u32_u8 (v_dot2_u32_u16) a dword column of a row pair, 11 a row where temporal_moments.hip issues 14 -- and every E is
// (|a|^2 + |b|^2) - 2 a.b at the end.
// Overflow bound.  A lane's 22 raw sums are uint32 and are combined in uint32 once, after its last pass.  By then a raw sum
// holds n = P * S samples of one row (S samples a pass: n = 32 at every depth), so it lies in [0, n top^2], and the partial
// |a|^2 + |b|^2 in [0, 2 n top^2] = [0, 1 073 217 600] < 2^30 at 12 bit (4 161 600 at 8 bit); 2 a.b <= |a|^2 + |b|^2, so the
// unsigned subtraction never borrows and E lies in [0, n top^2] < 2^29.  The interval of widening is therefore the lane's
// whole share; a block of up to floor((2^32 - 1) / (2 * 4095^2)) = 128 samples a row and lane would still fit (static_assert
// below).  Between the lanes: at 8 bit the 64 lanes of a wave go through wave_sum_u32, whose rows of 16 lanes hold at most
// 16 * 32 * 255^2 < 2^25; at 10 / 12 bit 16 lanes of 32 * 4095^2 would pass 2^32, so the u16 instance widens to 64 bits BEFORE
// the first lane is added and the wave sum is six 64-bit xor shuffles.
// Reduction.  Lane 0 of each wave adds the wave's 14 sums to the workgroup's 14 words of LDS (ds_add_u64), and after a barrier
// 14 threads add the non-zero ones to the launch's zeroed output with 64-bit integer global atomics: the blocks of a
// transition meet there.  The launch zeroes its own slice of the output first (in stream order), so every output word is
// written by the launch that owns it.  A whole plane of 4096 x 8192 x 4095^2 stays below 2^50.  Integer sums: the result does
// not depend on order, base address, pitch, load width, launch shape or chunking.  No floating point.
// A frame that two transitions share is read twice, the second time mostly from the L2 / MALL, as in temporal_moments.hip.
#include "plane_scan.h"

namespace pqa {
namespace {

constexpr int kFieldRaw = 22;                 // raw sums of a lane: 8 norms, 14 cross products
constexpr int kFieldPairs = kFieldRows / 2;   // row pairs of a workgroup's block

struct FieldArgs : PairPlanes {
  int h2;            // row pairs of the plane
  unsigned top2;     // top in both halves of a dword
  unsigned long long* out;   // [transition][14], zeroed
};

typedef unsigned short fld_u16x2 __attribute__((ext_vector_type(2)));

template <typename T>
__device__ __forceinline__ unsigned fld_dot(unsigned a, unsigned b, unsigned acc) {
  if constexpr (sizeof(T) == 1) return __builtin_amdgcn_udot4(a, b, acc, false);
  else return __builtin_amdgcn_udot2(__builtin_bit_cast(fld_u16x2, a), __builtin_bit_cast(fld_u16x2, b), acc, false);
}

template <typename T>
__device__ __forceinline__ unsigned fld_clamp(unsigned v, unsigned top2) {
  if constexpr (sizeof(T) == 1) return v;
  else return __builtin_bit_cast(unsigned, __builtin_elementwise_min(__builtin_bit_cast(fld_u16x2, v), __builtin_bit_cast(fld_u16x2, top2)));
}

// The raw sums.  Norms 0 ... 7: R_k[0], R_k[1], R_{k-1}[0], R_{k-1}[1], D_k[0], D_k[1], D_{k-1}[0], D_{k-1}[1] (2 * plane +
// parity).  Cross products 8 + word for the words 0 ... 11 (D_k[p] R_k[q], D_k[p] R_{k-1}[q], D_{k-1}[p] R_k[q] at 2 p + q),
// 20: D_k[0] D_k[1], 21: R_k[0] R_k[1].
// adds the 22 raw sums of one dword of packed samples of each of the eight rows: x[plane][parity], planes in the order above
template <typename T>
__device__ __forceinline__ void fld_add(unsigned (&acc)[kFieldRaw], const unsigned (&x)[4][2]) {
  enum { RK, RP, DK, DP };
#pragma unroll
  for (int pl = 0; pl < 4; ++pl)
#pragma unroll
    for (int p = 0; p < 2; ++p) acc[2 * pl + p] = fld_dot<T>(x[pl][p], x[pl][p], acc[2 * pl + p]);
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      acc[8 + 2 * p + q] = fld_dot<T>(x[DK][p], x[RK][q], acc[8 + 2 * p + q]);
      acc[12 + 2 * p + q] = fld_dot<T>(x[DK][p], x[RP][q], acc[12 + 2 * p + q]);
      acc[16 + 2 * p + q] = fld_dot<T>(x[DP][p], x[RK][q], acc[16 + 2 * p + q]);
    }
  acc[20] = fld_dot<T>(x[DK][0], x[DK][1], acc[20]);
  acc[21] = fld_dot<T>(x[RK][0], x[RK][1], acc[21]);
}

// the 14 words of a lane from its 22 raw sums: (|a|^2 + |b|^2) - 2 a.b in uint32 (the head comment has the bound)
__device__ __forceinline__ void fld_combine(const unsigned (&s)[kFieldRaw], unsigned (&e)[kFieldSums]) {
  enum { RK, RP, DK, DP };
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      e[2 * p + q] = (s[2 * DK + p] + s[2 * RK + q]) - 2u * s[8 + 2 * p + q];
      e[4 + 2 * p + q] = (s[2 * DK + p] + s[2 * RP + q]) - 2u * s[12 + 2 * p + q];
      e[8 + 2 * p + q] = (s[2 * DP + p] + s[2 * RK + q]) - 2u * s[16 + 2 * p + q];
    }
  e[12] = (s[2 * DK] + s[2 * DK + 1]) - 2u * s[20];
  e[13] = (s[2 * RK] + s[2 * RK + 1]) - 2u * s[21];
}

// VB: bytes of one load
template <typename T, int VB>
__global__ __launch_bounds__(kBlock) void field_moments_kernel(const FieldArgs a) {
  constexpr int S = 16 / (int)sizeof(T);     // samples of a lane
  constexpr int LPR = kFieldCols / S;        // lanes a row pair of the block: 8 / 16
  constexpr int PPP = kBlock / LPR;          // row pairs the workgroup covers a pass: 32 / 16
  constexpr int P = kFieldPairs / PPP;       // passes: 2 / 4
  // a raw sum holds P * S samples; |a|^2 + |b|^2 of twice as many products of at most 4095^2 must fit 32 bits
  static_assert(2ull * P * S * 4095ull * 4095ull <= 0xffffffffull, "a lane's share is too large for its 32-bit sums");
  static_assert(kFieldPairs % PPP == 0 && kFieldCols % S == 0, "the block is whole passes of whole lanes");
  __shared__ unsigned long long tot[kFieldSums];
  const int tid = threadIdx.x, lane = tid & 63, tr = blockIdx.z;   // transition tr: frames tr and tr + 1
  if (tid < kFieldSums) tot[tid] = 0ull;
  __syncthreads();

  const int x = blockIdx.x * kFieldCols + (tid % LPR) * S;       // the lane's first column
  const int i0 = blockIdx.y * kFieldPairs + tid / LPR;           // its row pair of pass 0
  // planes in the order of fld_add: R_k, R_{k-1}, D_k, D_{k-1}
  const T* const plane[4] = {(const T*)a.ref + (int64_t)(tr + 1) * a.ref_fp, (const T*)a.ref + (int64_t)tr * a.ref_fp,
                             (const T*)a.dis + (int64_t)(tr + 1) * a.dis_fp, (const T*)a.dis + (int64_t)tr * a.dis_fp};

  unsigned acc[kFieldRaw];
#pragma unroll
  for (int m = 0; m < kFieldRaw; ++m) acc[m] = 0u;
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int i = i0 + p * PPP;
    if (i < a.h2 && x < a.w) {   // rows 2 i and 2 i + 1 <= 2 h2 - 1 < h exist; quad_load keeps the columns below w
      PackedQuad q[4][2];
#pragma unroll
      for (int pl = 0; pl < 4; ++pl) {
        const int64_t rp = pl < 2 ? a.ref_rp : a.dis_rp;
        const T* row = plane[pl] + (int64_t)(2 * i) * rp;
        q[pl][0] = quad_load<T, VB, kTailZeros>(row, x, a.w);
        q[pl][1] = quad_load<T, VB, kTailZeros>(row + rp, x, a.w);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        unsigned v[4][2];
#pragma unroll
        for (int pl = 0; pl < 4; ++pl)
#pragma unroll
          for (int r = 0; r < 2; ++r) v[pl][r] = fld_clamp<T>(q[pl][r].d[k], a.top2);
        fld_add<T>(acc, v);
      }
    }
  }

  unsigned e[kFieldSums];
  fld_combine(acc, e);
#pragma unroll
  for (int m = 0; m < kFieldSums; ++m) {   // every lane of the wave is here: the wave sums read all 64
    unsigned long long s;
    if constexpr (sizeof(T) == 1) {
      s = wave_sum_u32(e[m]);
    } else {
      long long v = (long long)e[m];
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
      s = (unsigned long long)v;
    }
    if (lane == 0 && s) lds_add(tot + m, s);
  }
  __syncthreads();
  if (tid < kFieldSums && tot[tid]) atomicAdd(a.out + (int64_t)tr * kFieldSums + tid, tot[tid]);
}

template <typename T, int VB>
hipError_t launch_v(hipStream_t stream, const FieldArgs& a, int n_trans) {
  const dim3 grid((a.w + kFieldCols - 1) / kFieldCols, (a.h2 + kFieldPairs - 1) / kFieldPairs, n_trans);
  hipLaunchKernelGGL((field_moments_kernel<T, VB>), grid, dim3(kBlock), 0, stream, a);
  return hipGetLastError();
}

}  // namespace

size_t field_out_bytes(int n_frames) {
  return (size_t)(n_frames > 1 ? n_frames - 1 : 0) * kFieldSums * sizeof(unsigned long long);
}

hipError_t launch_field_moments(hipStream_t stream, Elem elem, int bits, const void* ref, int64_t ref_row_pitch,
                                int64_t ref_frame_pitch, const void* dis, int64_t dis_row_pitch, int64_t dis_frame_pitch,
                                int n_frames, int w, int h, unsigned long long* out) {
  if (n_frames <= 1) return hipSuccess;
  FieldArgs a{};
  if (h < 2 || n_frames - 1 > 65535 ||
      !pair_planes(a, elem, bits, ref, ref_row_pitch, ref_frame_pitch, dis, dis_row_pitch, dis_frame_pitch, w, h))
    return hipErrorInvalidValue;
  const hipError_t e = hipMemsetAsync(out, 0, field_out_bytes(n_frames), stream);
  if (e != hipSuccess) return e;
  a.h2 = h / 2;
  a.top2 = ((1u << bits) - 1u) * 0x00010001u;
  a.out = out;
  // a lane starts a multiple of 16 bytes into its row
  return dispatch(elem, load_bytes(elem, a),
                  [&](auto t, auto vb) { return launch_v<decltype(t), decltype(vb)::value>(stream, a, n_frames - 1); });
}

}  // namespace pqa
