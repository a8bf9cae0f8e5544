// Host side of the packed capture formats (pqa_submit_packed, pqa_unpack; unpack.hip has the kernel), free of any device
// call: the row and file geometry of UYVY / YUYV / v210, how one side of a chunk of frames -- planar planes or packed frames
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

// One side of a chunk as it is staged: n_planes planes per frame (a packed frame is one "plane" of its minimum row bytes),
// plane p of frame f at f * frame_bytes + off[p].
struct ClipLayout {
  int n_planes = 0;
  PlaneLayout plane[3] = {};
  size_t off[3] = {0, 0, 0};
  size_t frame_bytes = 0;
};
// rows row_align bytes apart at least, planes plane_align
inline ClipLayout clip_layout(int n_planes, const size_t row_bytes[3], const int rows[3], int64_t row_align, int64_t plane_align) {
  ClipLayout L;
  L.n_planes = n_planes;
  size_t off = 0;
  for (int p = 0; p < n_planes; ++p) {
    const int64_t pitch = round_up((int64_t)row_bytes[p], row_align);
    L.plane[p] = PlaneLayout{row_bytes[p], rows[p], pitch, (size_t)pitch * rows[p]};
    L.off[p] = off;
    off += (size_t)round_up((int64_t)L.plane[p].frame_bytes, plane_align);
  }
  L.frame_bytes = off;
  return L;
}
inline ClipLayout packed_layout(uint32_t format, int w, int h) {
  const size_t rb[3] = {(size_t)packed_min_row_bytes(format, w), 0, 0};
  const int rows[3] = {h, 0, 0};
  return clip_layout(1, rb, rows, 16, 16);
}
// the planes a packed frame of w x h unpacks to: Y of w x h, U and V of ceil(w / 2) x h
inline ClipLayout unpacked_layout(uint32_t format, int w, int h, int n_planes) {
  const size_t es = (size_t)packed_sample_bytes(format);
  const size_t rb[3] = {(size_t)w * es, (size_t)((w + 1) / 2) * es, (size_t)((w + 1) / 2) * es};
  const int rows[3] = {h, h, h};
  return clip_layout(n_planes, rb, rows, 16, 16);
}

// frames f0 ... f0 + n - 1 of a caller's clip into slots 0 ... n - 1 of a pinned buffer.  `frames` holds L.n_planes
// pointers per frame, frame-major; rows strides[p] bytes apart.  Only the L.plane[p].row_bytes bytes of a row that hold
// samples are read: the caller's last row may end at the end of its allocation.
inline void pack_clip(uint8_t* pin, const ClipLayout& L, const void* const* frames, const int64_t strides[3], int f0, int n) {
  for (int f = 0; f < n; ++f)
    for (int p = 0; p < L.n_planes; ++p)
      copy_plane_rows(pin + (size_t)f * L.frame_bytes + L.off[p], L.plane[p].pitch,
                      (const uint8_t*)frames[(size_t)(f0 + f) * L.n_planes + p], strides[p], L.plane[p].row_bytes, L.plane[p].h);
}

// The same copy as tasks of about task_bytes for the pack pool (host_pack.h), appended to `tasks`: frame f0 + f of the clip is
// task.frame = f of the run.  Large frames only: one core's memcpy, not PCIe, would bound the path otherwise.
inline void pack_clip_tasks(std::vector<PackTask>& tasks, uint8_t* pin, const ClipLayout& L, const void* const* frames,
                            const int64_t strides[3], int f0, int n, size_t task_bytes) {
  for (int f = 0; f < n; ++f)
    for (int p = 0; p < L.n_planes; ++p) {
      const PlaneLayout& P = L.plane[p];
      int rows_per = (int)(task_bytes / (P.row_bytes ? P.row_bytes : 1));
      if (rows_per < 1) rows_per = 1;
      const uint8_t* src = (const uint8_t*)frames[(size_t)(f0 + f) * L.n_planes + p];
      for (int y = 0; y < P.h; y += rows_per) {
        PackTask t{pin + (size_t)f * L.frame_bytes + L.off[p] + (size_t)y * P.pitch, src + (int64_t)y * strides[p], P.pitch, strides[p],
                   P.row_bytes, P.h - y < rows_per ? P.h - y : rows_per};
        t.frame = f;
        tasks.push_back(t);
      }
    }
}

// The way back: slots 0 ... n - 1 of a pinned buffer into a caller's planes (3 pointers per frame, frame-major, of which
// the first L.n_planes are written), row by row: the bytes between a destination row's end and the next row stay as they are.
inline void unpack_clip_out(const uint8_t* pin, const ClipLayout& L, void* const* planes, const int64_t strides[3], int f0, int n) {
  for (int f = 0; f < n; ++f)
    for (int p = 0; p < L.n_planes; ++p)
      for (int y = 0; y < L.plane[p].h; ++y)
        memcpy((uint8_t*)planes[(size_t)(f0 + f) * 3 + p] + (int64_t)y * strides[p],
               pin + (size_t)f * L.frame_bytes + L.off[p] + (size_t)y * L.plane[p].pitch, L.plane[p].row_bytes);
}

}  // namespace host
}  // namespace pqa
