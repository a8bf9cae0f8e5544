// Host side of the packed capture formats (pqa_submit_packed, pqa_unpack, pqa_rgb_convert; unpack.hip and rgb_convert.hip have
// the kernels), free of any device call: the row and file geometry of UYVY / YUYV / v210 and of the packed RGB formats, how one side of a chunk of frames -- planar planes or packed frames
// -- lies in a pinned buffer, the copy of a caller's frames into it and the copy of unpacked planes back out.  Packed bytes
// are copied as they are: nothing is de-interleaved on the host.  Header-only and plain C++17, as host_stage.h is, so that
// a CPU program drives it under AddressSanitizer + UBSan (tests/packed_harness.cpp).
#pragma once
#include <vector>

#include "host_pack.h"
#include "host_stage.h"

namespace pqa {
namespace host {

enum { FMT_PLANAR = 0, FMT_UYVY = 3, FMT_YUYV = 4, FMT_V210 = 5 };   // the PQA_SURFACE_* values (include/pqa_vmaf.h)

inline bool packed_format(uint32_t f) { return f == FMT_UYVY || f == FMT_YUYV || f == FMT_V210; }
inline int packed_bit_depth(uint32_t f) { return f == FMT_V210 ? 10 : 8; }
inline int packed_sample_bytes(uint32_t f) { return f == FMT_V210 ? 2 : 1; }
// the bytes of a row that hold samples: cw macropixels of 4 bytes; ceil(w / 6) groups of 16 bytes
inline int64_t packed_min_row_bytes(uint32_t f, int w) {
  return f == FMT_V210 ? 16 * (((int64_t)w + 5) / 6) : 4 * (((int64_t)w + 1) / 2);
}
// rows of a headerless file: v210 pads to 48 pixels (128 bytes), the 8-bit formats do not pad
inline int64_t packed_file_stride(uint32_t f, int w) {
  return f == FMT_V210 ? (((int64_t)w + 47) / 48) * 128 : packed_min_row_bytes(f, w);
}

// Packed RGB captures (pqa_rgb_convert; rgb_convert.hip has the kernel): a pixel is 4 bytes in every format.
enum { FMT_BGRA = 6, FMT_ARGB = 7, FMT_RGBA = 8, FMT_ABGR = 9, FMT_R210 = 10 };   // the PQA_SURFACE_* values
inline bool rgb_format(uint32_t f) { return f >= FMT_BGRA && f <= FMT_R210; }
inline int rgb_bit_depth(uint32_t f) { return f == FMT_R210 ? 10 : 8; }
inline int64_t rgb_min_row_bytes(int w) { return 4 * (int64_t)w; }
// rows of a headerless file: r210 pads to 64 pixels (256 bytes), the 8-bit formats do not pad
inline int64_t rgb_file_stride(uint32_t f, int w) { return f == FMT_R210 ? (((int64_t)w + 63) / 64) * 256 : rgb_min_row_bytes(w); }
// the byte of R, G, B in a pixel of the 8-bit formats (r210: unused, zeros)
inline void rgb_byte_order(uint32_t f, int at[3]) {
  static const int order[4][3] = {{2, 1, 0}, {1, 2, 3}, {0, 1, 2}, {3, 2, 1}};   // BGRA, ARGB, RGBA, ABGR
  for (int k = 0; k < 3; ++k) at[k] = f >= FMT_BGRA && f <= FMT_ABGR ? order[f - FMT_BGRA][k] : 0;
}
// The bound that makes int32 arithmetic legal in rgb_convert.hip: for every row c of the Q14 matrix m[3][4] (column 0 the
// offset), the extreme of |A_c| = |m[c][0] + m[c][1] R + m[c][2] G + m[c][3] B| over the cube [0, 2^src_bits - 1]^3, times the
// tap weights' sum S_x S_y (8 an axis of shift 1, else 1), plus the rounding half 2^(13 + log2(S_x S_y)), stays below 2^31.
inline bool rgb_matrix_fits(const int32_t m[12], int src_bits, int hshift, int vshift) {
  const int64_t top = ((int64_t)1 << src_bits) - 1, s = (int64_t)1 << (3 * (hshift + vshift));
  for (int c = 0; c < 3; ++c) {
    int64_t hi = m[4 * c], lo = m[4 * c];
    for (int k = 1; k < 4; ++k) (m[4 * c + k] > 0 ? hi : lo) += (int64_t)m[4 * c + k] * top;
    const int64_t ext = (hi < 0 ? -hi : hi) > (lo < 0 ? -lo : lo) ? (hi < 0 ? -hi : hi) : (lo < 0 ? -lo : lo);
    if (ext * s + (s << 13) >= ((int64_t)1 << 31)) return false;
  }
  return true;
}

// How a packed frame and the planes it turns into lie in a staging chunk (ClipLayout, host_stage.h).
inline ClipLayout packed_layout(uint32_t format, int w, int h) { return plane_clip((size_t)packed_min_row_bytes(format, w), h); }
// the planes a packed frame of w x h unpacks to: Y of w x h, U and V of ceil(w / 2) x h
inline ClipLayout unpacked_layout(uint32_t format, int w, int h, int n_planes) {
  const size_t es = (size_t)packed_sample_bytes(format);
  const size_t rb[3] = {(size_t)w * es, (size_t)((w + 1) / 2) * es, (size_t)((w + 1) / 2) * es};
  const int rows[3] = {h, h, h};
  return clip_layout(n_planes, rb, rows, 16, 16);
}

inline ClipLayout rgb_layout(int w, int h) { return plane_clip((size_t)rgb_min_row_bytes(w), h); }
// the planes an RGB frame of w x h converts to: Y of w x h, U and V of cw x ch, samples of es bytes
inline ClipLayout converted_layout(int w, int h, int cw, int ch, int es, int n_planes) {
  const size_t rb[3] = {(size_t)w * es, (size_t)cw * es, (size_t)cw * es};
  const int rows[3] = {h, ch, ch};
  return clip_layout(n_planes, rb, rows, 16, 16);
}

// pack_clip's copy as tasks of about task_bytes for the pack pool, appended to `tasks`: the builder of host_pack.h
// (pack_frame_tasks) over a caller's frame list; frame f0 + f of the clip is task.frame = f of the run.
inline void pack_clip_tasks(std::vector<PackTask>& tasks, uint8_t* pin, const ClipLayout& L, const void* const* frames,
                            const int64_t strides[3], int f0, int n, size_t task_bytes) {
  for (int f = 0; f < n; ++f) {
    PlaneSrc src[3] = {};
    for (int p = 0; p < L.n_planes; ++p) src[p] = PlaneSrc{(const uint8_t*)frames[(size_t)(f0 + f) * L.n_planes + p], strides[p], -1, 0};
    pack_frame_tasks(tasks, L, pin + (size_t)f * L.frame_bytes, src, 0, 0, f, task_bytes);
  }
}

}  // namespace host
}  // namespace pqa
