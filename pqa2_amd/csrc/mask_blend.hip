// Overlay masking: planes through a feathered mask, in exact integers (pqa_mask_blend / pqa_mask_blend_device; restated in
// tests/mask_ref.py).  The mask is a grid of nodes A[gy][gx] of 0 ... 256, Gx = 1 << sx and Gy = 1 << sy samples apart,
// gx = ((w + Gx - 1) >> sx) + 1 columns and gy rows likewise.  For sample (x, y), i = x >> sx, fx = x & (Gx - 1), j = y >> sy,
// fy = y & (Gy - 1):
//
//   E_i = A[j][i] (Gy - fy) + A[j+1][i] fy                                         0 ... 256 Gy, below 2^15
//   a   = (E_i (Gx - fx) + E_{i+1} fx + ((Gx Gy) >> 1)) >> (sx + sy)              0 ... 256, below 2^21 before the shift
//   dst = (src (256 - a) + fill a + 128) >> 8                                      below 2^21 at 12 bit
//
// fill: a constant, or the sample at (x, y) of a fill plane with a base and pitches of its own.  a = 0 gives src as it is,
// a = 256 gives fill.  u16: where a > 0 a source sample above top = 2^bit_depth - 1 is read as top, and so is every sample
// of the fill plane; where a = 0 the source sample is copied as it is, in and out of the launch's rectangle alike.
// Byte work bound by HBM, like table_apply.hip.  No scratch, no atomics, no floating point, plain vector stores.
//
// Work.  An item is 16 bytes of a row (16 u8 / 8 u16 samples).  A workgroup of 256 threads takes a tile of 64 items by
// 4 * rpw rows; wave v the rows v * rpw ... of it, lane l the item l of each, so a wave reads 1 KiB of a row at a time and a
// lane has its rpw source (and fill) loads in flight together.  A plane narrower than 64 items leaves lanes idle: masks are
// drawn on pictures, not on strips.
// LDS.  The workgroup first copies the node rows its rows touch, for the node columns its items touch, then forms E once per
// row and node column (u16 both).  An item reads the E of its columns once to sort itself: every E zero -> a is zero across it,
// the item is copied without arithmetic (in place: left alone, no load, no store); every E equal to 256 Gy -> a is 256 across
// it, the item is the fill and the source is not read; otherwise a runs across the item from E_i and E_{i+1} with one 24-bit
// multiply and one add a sample (v_mul_i32_i24 and a three-operand add is what the compiler makes of the mad; the blend takes
// the same pair again), stepping to the next node column where fx wraps.  rpw is 4, or 2 with sx = 0, where there is a node column
// a sample: 37 KiB of LDS at most.
// Rectangle.  The launch covers rows y0 ... y1 - 1 and the items from x0 (a multiple of an item) to x1.  In place (dst exactly
// src) that is the bounding rectangle of the samples with a > 0, which the host takes from the non-zero nodes: a logo on 2 % of
// the frame costs a pass over 2 % of it.  Not in place it is the whole plane, and what lies outside the mask is copied.
// One load is 16 bytes, 4 bytes or one sample, whichever the bases and pitches of ALL planes allow (plane_scan.h, load_bytes);
// the item that crosses the end of the row goes sample by sample: no source byte past a row's last sample is read and no
// destination byte past it is written.
#include "plane_scan.h"

#include <vector>

namespace pqa {
namespace {

constexpr int kMaskCols = 64;   // items a tile row: a wave
constexpr int kMaskWaves = kBlock / 64;

struct MaskArgs {
  const void* src;
  const void* fill;                // null: fill_const
  void* dst;
  const uint16_t* nodes;           // rows of gx; only the rows nj0 ... nj1 are there to be read, every other row is zero
  int64_t src_rp, src_fp, fill_rp, fill_fp, dst_rp, dst_fp;   // elements
  int w, h, gx, nj0, nj1, sx, sy;
  int x0, y0, x1, y1;              // the samples the launch covers; x0 a multiple of an item
  int rpw;                         // rows a wave
  int ncols, nrows;                // node columns and node rows a workgroup holds
  unsigned fill_const, top;
  int inplace;
};

enum ItemClass { kSkip, kCopy, kFill, kBlend };

template <typename T, int VB>
__device__ __forceinline__ void quad_store(T* row, int x, int x1, const PackedQuad& o) {
  constexpr int S = 16 / (int)sizeof(T), PER = 4 / (int)sizeof(T), BITS = 8 * (int)sizeof(T);
  if (x + S <= x1 && VB == 16) {
    *reinterpret_cast<uint4*>(row + x) = make_uint4(o.d[0], o.d[1], o.d[2], o.d[3]);
  } else if (x + S <= x1 && VB == 4) {
#pragma unroll
    for (int j = 0; j < 4; ++j) *reinterpret_cast<unsigned*>(row + x + j * PER) = o.d[j];
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int s = 0; s < PER; ++s) {
        const int xx = x + j * PER + s;
        if (xx < x1) row[xx] = (T)(o.d[j] >> (BITS * s));
      }
  }
}

// VB: bytes of one load and of one store.  PLANE: the fill is a plane.
template <typename T, int VB, bool PLANE>
__global__ __launch_bounds__(kBlock) void mask_blend_kernel(const MaskArgs a) {
  extern __shared__ uint4 lds4[];
  constexpr int S = 16 / (int)sizeof(T), PER = 4 / (int)sizeof(T), BITS = 8 * (int)sizeof(T);
  constexpr unsigned MASK = (1u << BITS) - 1u;
  uint16_t* const N = reinterpret_cast<uint16_t*>(lds4);   // nrows x ncols nodes
  uint16_t* const E = N + a.nrows * a.ncols;                // 4 rpw rows x ncols
  const int tid = threadIdx.x, rows = kMaskWaves * a.rpw;
  const int tx0 = a.x0 + (int)blockIdx.x * (kMaskCols * S), ty0 = a.y0 + (int)blockIdx.y * rows;
  const int ib = tx0 >> a.sx, j0 = ty0 >> a.sy;
  const int Gx = 1 << a.sx, Gy = 1 << a.sy;

  for (int idx = tid; idx < a.nrows * a.ncols; idx += kBlock) {
    const int jl = idx / a.ncols, il = idx - jl * a.ncols;
    const int jj = j0 + jl, ii = ib + il;
    N[idx] = jj >= a.nj0 && jj <= a.nj1 && ii < a.gx ? a.nodes[(int64_t)jj * a.gx + ii] : (uint16_t)0;
  }
  __syncthreads();
  for (int idx = tid; idx < rows * a.ncols; idx += kBlock) {
    const int r = idx / a.ncols, il = idx - r * a.ncols;
    const int y = ty0 + r, fy = y & (Gy - 1), jl = (y >> a.sy) - j0;
    unsigned e = 0u;
    if (y < a.y1) e = __umul24(N[jl * a.ncols + il], Gy - fy) + __umul24(N[(jl + 1) * a.ncols + il], fy);
    E[idx] = (uint16_t)e;
  }
  __syncthreads();

  const int wv = tid >> 6, lane = tid & 63;
  const int x = tx0 + lane * S;
  const unsigned full = 256u << a.sy;
  const int frame = blockIdx.z;
  const T* sf = (const T*)a.src + (int64_t)frame * a.src_fp;
  const T* ff = PLANE ? (const T*)a.fill + (int64_t)frame * a.fill_fp : nullptr;
  T* df = (T*)a.dst + (int64_t)frame * a.dst_fp;
  const int xe = min(x + S, a.w);              // the item's samples end before xe
  const int c0 = (x >> a.sx) - ib;             // its first node column in E
  const int c1 = ((xe - 1) >> a.sx) - ib + 1;  // its last

  PackedQuad qs[4], qf[4];
  int cls[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    cls[k] = kSkip;
    const int r = wv * a.rpw + k, y = ty0 + r;
    if (k >= a.rpw || y >= a.y1 || x >= a.x1) continue;
    const uint16_t* e = E + r * a.ncols;
    unsigned lo = e[c0], hi = lo;
    for (int c = c0 + 1; c <= c1; ++c) {
      const unsigned v = e[c];
      lo = min(lo, v); hi = max(hi, v);
    }
    int cl = hi == 0u ? kCopy : lo == full ? kFill : kBlend;
    if (cl == kCopy && a.inplace) cl = kSkip;
    if (cl == kCopy || cl == kBlend) qs[k] = quad_load<T, VB, kTailZeros>(sf + (int64_t)y * a.src_rp, x, a.w);
    if constexpr (PLANE)
      if (cl == kFill || cl == kBlend) qf[k] = quad_load<T, VB, kTailZeros>(ff + (int64_t)y * a.fill_rp, x, a.w);
    cls[k] = cl;
  }

  const int half = (Gx * Gy) >> 1, sh = a.sx + a.sy;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (cls[k] == kSkip) continue;
    const int r = wv * a.rpw + k, y = ty0 + r;
    PackedQuad o;
    if (cls[k] == kCopy) {
      o = qs[k];
    } else if (cls[k] == kFill) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        unsigned v = 0u;
#pragma unroll
        for (int s = 0; s < PER; ++s) {
          unsigned f = a.fill_const;
          if constexpr (PLANE) f = (qf[k].d[j] >> (BITS * s)) & MASK;
          if constexpr (PLANE && sizeof(T) > 1) f = min(f, a.top);
          v |= f << (BITS * s);
        }
        o.d[j] = v;
      }
    } else {
      const uint16_t* e = E + r * a.ncols;
      int c = c0, fx = x & (Gx - 1);
      int e0 = e[c], e1 = e[c + 1];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        unsigned v = 0u;
#pragma unroll
        for (int s = 0; s < PER; ++s) {
          const int al = (__mul24(e1 - e0, fx) + (e0 << a.sx) + half) >> sh;   // E_i (Gx - fx) + E_{i+1} fx = E_i Gx + (E_{i+1} - E_i) fx
          const unsigned raw = (qs[k].d[j] >> (BITS * s)) & MASK;
          int sv = (int)raw, f = (int)a.fill_const;
          if constexpr (PLANE) f = (int)((qf[k].d[j] >> (BITS * s)) & MASK);
          if constexpr (sizeof(T) > 1) {
            sv = min(sv, (int)a.top);
            if constexpr (PLANE) f = min(f, (int)a.top);
          }
          unsigned out = (unsigned)(__mul24(al, f - sv) + (sv << 8) + 128) >> 8;   // src (256 - a) + fill a + 128, never negative
          if constexpr (sizeof(T) > 1) out = al == 0 ? raw : out;
          v |= out << (BITS * s);
          if (j * PER + s < S - 1 && ++fx == Gx) {   // the next sample opens the next node column; c + 1 <= c1 while samples remain
            fx = 0; ++c;
            e0 = e1;
            if (c < c1) e1 = e[c + 1];
          }
        }
        o.d[j] = v;
      }
    }
    quad_store<T, VB>(df + (int64_t)y * a.dst_rp, x, a.w, o);
  }
}

template <typename T, int VB>
hipError_t launch_v(hipStream_t stream, const MaskArgs& a, int n_frames) {
  constexpr int S = 16 / (int)sizeof(T);
  const int rows = kMaskWaves * a.rpw, tile_w = kMaskCols * S;
  const dim3 grid((a.x1 - a.x0 + tile_w - 1) / tile_w, (a.y1 - a.y0 + rows - 1) / rows, n_frames);
  const size_t lds = (size_t)(a.nrows + rows) * a.ncols * sizeof(uint16_t);
  if (a.fill)
    hipLaunchKernelGGL((mask_blend_kernel<T, VB, true>), grid, dim3(kBlock), lds, stream, a);
  else
    hipLaunchKernelGGL((mask_blend_kernel<T, VB, false>), grid, dim3(kBlock), lds, stream, a);
  return hipGetLastError();
}

}  // namespace

bool mask_node_bounds(const uint16_t* nodes, int w, int h, int sx, int sy, MaskBounds* b) {
  const int gx = mask_grid(w, sx), gy = mask_grid(h, sy);
  // two loops the compiler turns into vector maxima: the call's host time is this scan and the grid's upload
  std::vector<uint16_t> colmax((size_t)gx, 0);
  uint16_t* cm = colmax.data();
  int j0 = gy, j1 = -1;
  unsigned all = 0u;
  for (int j = 0; j < gy; ++j) {
    const uint16_t* r = nodes + (size_t)j * gx;
    uint16_t m = 0;
    for (int i = 0; i < gx; ++i) m = std::max(m, r[i]);
    if (!m) continue;
    for (int i = 0; i < gx; ++i) cm[i] = std::max(cm[i], r[i]);
    all = std::max(all, (unsigned)m);
    j0 = std::min(j0, j);
    j1 = j;
  }
  if (all > 256u) return false;
  *b = MaskBounds{};
  if (j1 < 0) return true;
  int i0 = 0, i1 = gx - 1;
  while (!cm[i0]) ++i0;
  while (!cm[i1]) --i1;
  b->row0 = j0; b->rows = j1 - j0 + 1;
  // node i weighs on the samples strictly between nodes i - 1 and i + 1
  const auto lo = [](int n, int s) { return std::max(0, ((n - 1) << s) + 1); };
  const auto hi = [](int n, int s, int size) { return (int)std::min<int64_t>(size, (int64_t)(n + 1) << s); };
  const int rect[4] = {lo(i0, sx), lo(j0, sy), hi(i1, sx, w), hi(j1, sy, h)};
  if (rect[0] < rect[2] && rect[1] < rect[3])   // else: nodes past the last sample, which weigh on none
    for (int k = 0; k < 4; ++k) b->rect[k] = rect[k];
  return true;
}

hipError_t launch_mask_blend(hipStream_t stream, Elem elem, int bit_depth, const uint16_t* nodes, int sx, int sy, unsigned fill_const,
                             const MaskBounds& bounds, const void* src, int64_t src_row_pitch, int64_t src_frame_pitch, const void* fill,
                             int64_t fill_row_pitch, int64_t fill_frame_pitch, void* dst, int64_t dst_row_pitch, int64_t dst_frame_pitch,
                             int n_frames, int w, int h) {
  if (n_frames <= 0) return hipSuccess;
  const int* rect = bounds.rect;
  if (n_frames > 65535 || !nodes || !src || !dst || !scan_shape_ok(elem, bit_depth, w, h) || sx < 0 || sx > kMaskMaxStep ||
      sy < 0 || sy > kMaskMaxStep || fill_const >= (1u << bit_depth) || dst == fill)
    return hipErrorInvalidValue;
  const int es = elem == ELEM_U8 ? 1 : 2;
  uintptr_t bits = (uintptr_t)src | (uintptr_t)src_row_pitch | (uintptr_t)src_frame_pitch | (uintptr_t)dst | (uintptr_t)dst_row_pitch |
                   (uintptr_t)dst_frame_pitch;
  if (fill) bits |= (uintptr_t)fill | (uintptr_t)fill_row_pitch | (uintptr_t)fill_frame_pitch;
  const int64_t row = (int64_t)w * es;
  if ((bits & (uintptr_t)(es - 1)) || src_row_pitch < row || dst_row_pitch < row || (fill && fill_row_pitch < row))
    return hipErrorInvalidValue;
  if (rect[0] < 0 || rect[1] < 0 || rect[2] > w || rect[3] > h || bounds.row0 < 0 || bounds.rows < 0 ||
      bounds.row0 + bounds.rows > mask_grid(h, sy))
    return hipErrorInvalidValue;
  MaskArgs a{};
  a.src = src; a.fill = fill; a.dst = dst; a.nodes = nodes;
  a.src_rp = src_row_pitch / es; a.src_fp = src_frame_pitch / es;
  a.fill_rp = fill_row_pitch / es; a.fill_fp = fill_frame_pitch / es;
  a.dst_rp = dst_row_pitch / es; a.dst_fp = dst_frame_pitch / es;
  a.w = w; a.h = h; a.sx = sx; a.sy = sy;
  a.gx = mask_grid(w, sx);
  a.nj0 = bounds.row0; a.nj1 = bounds.row0 + bounds.rows - 1;
  a.fill_const = fill_const; a.top = (1u << bit_depth) - 1u;
  a.inplace = src == dst && src_row_pitch == dst_row_pitch && src_frame_pitch == dst_frame_pitch;
  const int S = 16 / es;
  if (a.inplace) {
    if (rect[0] >= rect[2] || rect[1] >= rect[3]) return hipSuccess;   // a is zero everywhere
    a.x0 = rect[0] / S * S; a.y0 = rect[1];
    a.x1 = std::min(w, (rect[2] + S - 1) / S * S); a.y1 = rect[3];
  } else {
    a.x0 = a.y0 = 0; a.x1 = w; a.y1 = h;
  }
  a.rpw = sx == 0 ? 2 : 4;
  const int rows = kMaskWaves * a.rpw, tile_w = kMaskCols * S;
  a.ncols = (tile_w >> sx) + 3;                       // a tile that starts inside a cell, and the node behind its last sample
  a.nrows = ((rows + (1 << sy) - 1) >> sy) + 2;       // likewise
  int vb = std::min(load_bytes(elem, src, a.src_rp, a.src_fp), load_bytes(elem, dst, a.dst_rp, a.dst_fp));
  if (fill) vb = std::min(vb, load_bytes(elem, fill, a.fill_rp, a.fill_fp));
  return dispatch(elem, vb, [&](auto t, auto v) { return launch_v<decltype(t), decltype(v)::value>(stream, a, n_frames); });
}

}  // namespace pqa
