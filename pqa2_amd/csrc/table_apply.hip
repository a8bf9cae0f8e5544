// Transfer-curve alignment: planes through an integer table (pqa_table_apply / pqa_table_apply_device; restated in
// tests/curve_ref.py).  For one plane of w x h samples and a table of L = 2^bit_depth entries of the sample type:
//
//   dst[y][x] = table[min(src[y][x], L - 1)]
//
// Any table, monotone or not; the destination may be exactly the source.  Byte work bound by HBM, like format_convert.hip: one
// read and one write of the plane.  No scratch, no atomics, no floating point.
//
// Table.  Every workgroup copies the table from HBM (L2 after the first) into LDS with 16-byte moves: 256 B / 2 KiB / 8 KiB at
// 8 / 10 / 12 bit.  A lookup is one LDS read of a sample's width (ds_read_u8 / ds_read_u16) at a data-dependent address.  At
// 8 bit the table is 64 dwords: taking a byte read to be banked as a dword read is (32 banks over a group of 32 lanes; no
// counter run confirms it), a dword and the one 32 further on share a bank and lanes that read the same dword broadcast, so
// a group costs at most two LDS cycles on flat or smooth content and what the spread of its levels gives on noise.  Measured
// on noise through a permutation table: about one luma PSNR pass a plane.  The other form -- the 64
// dwords held one per lane of a wave and fetched with a cross-lane move -- was not built: it is the same LDS crossbar
// (ds_bpermute) plus a byte select per sample.
// Work.  An item is 16 bytes of a row (16 u8 / 8 u16 samples); a plane has ceil(w / S) items a row, numbered row by row, so a
// narrow plane fills its lanes as a wide one does.  A workgroup of 256 threads takes kTableItems * 256 consecutive items of
// one frame, thread t the items t, t + 256, ...: a wave reads 1 KiB of a row at a time.  A lane issues its kTableItems loads,
// then looks up and stores item by item, so the loads are in flight together.  One load is 16 bytes, 4 bytes or one sample,
// whichever the bases and pitches of BOTH planes allow (plane_scan.h, load_bytes); the store takes the same width.  The item
// that crosses the end of the row is read and written sample by sample: no source byte past a row's last sample is read and no
// destination byte past it is written.  In place: a lane reads and writes the same 16 bytes and nobody else's.
#include "plane_scan.h"

namespace pqa {
namespace {

constexpr int kTableItems = 4;   // items of 16 bytes a lane: 16 KiB a workgroup, 127 workgroups a 1080p 8-bit plane

struct TableArgs {
  const void* src;
  void* dst;
  const void* table;               // L entries of the sample type in HBM, 16-byte aligned
  int64_t src_rp, src_fp, dst_rp, dst_fp;   // elements
  int w, h, L;
  int segs;                        // items a row
  int step_rows, step_segs;        // kBlock items further on: kBlock / segs rows and kBlock % segs items
};

// the samples of four packed dwords through the table, packed again
template <typename T>
__device__ __forceinline__ PackedQuad lookup(const T* tab, const PackedQuad& q, unsigned top) {
  constexpr int PER = 4 / (int)sizeof(T), BITS = 8 * (int)sizeof(T);
  constexpr unsigned MASK = (1u << BITS) - 1u;
  PackedQuad o;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    unsigned v = 0u;
#pragma unroll
    for (int s = 0; s < PER; ++s) {
      unsigned i = (q.d[k] >> (BITS * s)) & MASK;
      if constexpr (sizeof(T) > 1) i = min(i, top);   // a u16 container can hold a sample above L - 1; a u8 one cannot
      v |= (unsigned)tab[i] << (BITS * s);
    }
    o.d[k] = v;
  }
  return o;
}

// VB: bytes of one load and of one store
template <typename T, int VB>
__global__ __launch_bounds__(kBlock) void table_apply_kernel(const TableArgs a) {
  extern __shared__ uint4 tab4[];
  constexpr int S = 16 / (int)sizeof(T), PER = 4 / (int)sizeof(T), BITS = 8 * (int)sizeof(T);
  const int tid = threadIdx.x;
  for (int i = tid; i < a.L * (int)sizeof(T) / 16; i += kBlock) tab4[i] = reinterpret_cast<const uint4*>(a.table)[i];
  __syncthreads();
  const T* tab = reinterpret_cast<const T*>(tab4);
  const unsigned top = (unsigned)a.L - 1u;

  const T* sf = (const T*)a.src + (int64_t)blockIdx.y * a.src_fp;
  T* df = (T*)a.dst + (int64_t)blockIdx.y * a.dst_fp;
  const int item = blockIdx.x * (kBlock * kTableItems) + tid;   // below 2^23 + 2^10: segs * h <= 8192 * 8192 / 8
  int y = item / a.segs, sg = item - y * a.segs;

  PackedQuad q[kTableItems];
  int ys[kTableItems], xs[kTableItems];
#pragma unroll
  for (int k = 0; k < kTableItems; ++k) {
    ys[k] = y; xs[k] = sg * S;
    if (y < a.h) q[k] = quad_load<T, VB, kTailZeros>(sf + (int64_t)y * a.src_rp, xs[k], a.w);
    y += a.step_rows; sg += a.step_segs;
    if (sg >= a.segs) { sg -= a.segs; ++y; }
  }
#pragma unroll
  for (int k = 0; k < kTableItems; ++k) {
    if (ys[k] >= a.h) continue;
    const PackedQuad o = lookup<T>(tab, q[k], top);
    T* row = df + (int64_t)ys[k] * a.dst_rp;
    const int x = xs[k];
    if (x + S <= a.w && VB == 16) {
      *reinterpret_cast<uint4*>(row + x) = make_uint4(o.d[0], o.d[1], o.d[2], o.d[3]);
    } else if (x + S <= a.w && VB == 4) {
#pragma unroll
      for (int j = 0; j < 4; ++j) *reinterpret_cast<unsigned*>(row + x + j * PER) = o.d[j];
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int s = 0; s < PER; ++s) {
          const int xx = x + j * PER + s;
          if (xx < a.w) row[xx] = (T)(o.d[j] >> (BITS * s));
        }
    }
  }
}

template <typename T, int VB>
hipError_t launch_v(hipStream_t stream, const TableArgs& a, int n_frames) {
  const int items = a.segs * a.h, per_block = kBlock * kTableItems;
  hipLaunchKernelGGL((table_apply_kernel<T, VB>), dim3((items + per_block - 1) / per_block, n_frames), dim3(kBlock),
                     (size_t)a.L * sizeof(T), stream, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_table_apply(hipStream_t stream, Elem elem, int bit_depth, const void* table, const void* src, int64_t src_row_pitch,
                              int64_t src_frame_pitch, void* dst, int64_t dst_row_pitch, int64_t dst_frame_pitch, int n_frames, int w,
                              int h) {
  if (n_frames <= 0) return hipSuccess;
  if (n_frames > 65535 || !table || !src || !dst || !scan_shape_ok(elem, bit_depth, w, h)) return hipErrorInvalidValue;
  const int es = elem == ELEM_U8 ? 1 : 2;
  // whole samples on both sides, rows that hold a row, a table the 16-byte moves can read
  if ((((uintptr_t)src | (uintptr_t)src_row_pitch | (uintptr_t)src_frame_pitch | (uintptr_t)dst | (uintptr_t)dst_row_pitch |
        (uintptr_t)dst_frame_pitch) & (uintptr_t)(es - 1)) ||
      ((uintptr_t)table & 15) || src_row_pitch < (int64_t)w * es || dst_row_pitch < (int64_t)w * es)
    return hipErrorInvalidValue;
  TableArgs a{};
  a.src = src; a.dst = dst; a.table = table;
  a.src_rp = src_row_pitch / es; a.src_fp = src_frame_pitch / es;
  a.dst_rp = dst_row_pitch / es; a.dst_fp = dst_frame_pitch / es;
  a.w = w; a.h = h; a.L = 1 << bit_depth;
  const int S = 16 / es;
  a.segs = (w + S - 1) / S;
  a.step_rows = kBlock / a.segs; a.step_segs = kBlock % a.segs;
  // an item starts a multiple of 16 bytes into its row
  const int vb = std::min(load_bytes(elem, src, a.src_rp, a.src_fp), load_bytes(elem, dst, a.dst_rp, a.dst_fp));
  return dispatch(elem, vb, [&](auto t, auto v) { return launch_v<decltype(t), decltype(v)::value>(stream, a, n_frames); });
}

}  // namespace pqa
