// Host side of the pair staging of the side analyses (pqa_side.hip), free of any device call: the packed layout of a plane of
// the call's own size, the packing of a chunk of planes into a pinned buffer, and the walk over the chunks of a clip pair.  The
// device is reached only through callables the caller passes in.  Header-only and plain C++17, as host_pack.h is, so that
// the CPU harness drives it under ThreadSanitizer / AddressSanitizer (tests/host_harness.cpp); pqa_ctx.h includes it as is.
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace pqa {

inline int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

// h rows of row_bytes; the last row ends at its last sample (the source need not hold a whole pitch behind it)
inline void copy_plane_rows(uint8_t* dst, int64_t dst_pitch, const uint8_t* src, int64_t src_pitch, size_t row_bytes, int h) {
  if (dst_pitch == src_pitch) {
    memcpy(dst, src, (size_t)dst_pitch * (h - 1) + row_bytes);
    return;
  }
  for (int y = 0; y < h; ++y) memcpy(dst + (int64_t)y * dst_pitch, src + (int64_t)y * src_pitch, row_bytes);
}

namespace host {

// A plane as it is staged: rows 16 bytes apart at least, so the kernels take their wide loads; planes one behind the other.
struct PlaneLayout {
  size_t row_bytes;
  int h;
  int64_t pitch;        // bytes from row to row
  size_t frame_bytes;   // bytes from plane to plane
};
inline PlaneLayout plane_layout(size_t row_bytes, int h) {
  const int64_t pitch = round_up((int64_t)row_bytes, 16);
  return PlaneLayout{row_bytes, h, pitch, (size_t)pitch * h};
}

// frames[0 .. n) (rows `stride` bytes apart) into slots 0 .. n - 1 of a pinned buffer
inline void pack_planes(uint8_t* pin, const PlaneLayout& L, const void* const* frames, int64_t stride, int n) {
  for (int f = 0; f < n; ++f) copy_plane_rows(pin + (size_t)f * L.frame_bytes, L.pitch, (const uint8_t*)frames[f], stride, L.row_bytes, L.h);
}

// n_frames planes of `ref` and of `dis` (null: the one-clip form, which leaves pin[1] alone) onto the device in chunks of at
// most `chunk`, each chunk launched before the next is packed.  For every chunk:
//   drain()                      not before the first chunk: the pinned buffers are packed again only after the device has
//                                read the chunk before (the staging is not pipelined)
//   pack                         the chunk's planes into slots 0 ... n - 1 of pin[0] (and pin[1])
//   seam(from_slot)              carry 1, not in the first chunk: device slot from_slot moves to device slot 0
//   upload(slot, n)              the n packed planes to device slots slot ... slot + n - 1
//   launch(slot, n, out_index)   n planes from device slot `slot` on; the results go `out_index` results into the output
// carry 0: a result per frame.  A chunk lands in slots 0 ... n - 1 and its launch writes results f0 ... f0 + n - 1.
// carry 1: a result per transition from a frame to the next.  The device buffers hold one slot more than a chunk: a chunk lands
// in slots 1 ... n, and before the next chunk overwrites them its last plane moves to slot 0 (only a full chunk has a
// successor, so that is slot `chunk`), where it is the predecessor of the next chunk's first.  So the first launch starts at
// slot 1 (n planes, n - 1 transitions from transition 0 on) and every later one at slot 0 (n + 1 planes, n transitions from
// f0 - 1 on).
// Stops at the first callable that returns something other than E{} (success) and returns that; stops before a chunk when
// `cancelled` is set and returns E{}.
template <class Drain, class Seam, class Upload, class Launch>
auto stage_walk(const PlaneLayout& L, uint8_t* const pin[2], const void* const* ref, int64_t ref_stride, const void* const* dis,
                int64_t dis_stride, int n_frames, int chunk, int carry, const std::atomic<int>& cancelled, Drain drain, Seam seam,
                Upload upload, Launch launch) -> decltype(drain()) {
  using E = decltype(drain());
  E e{};
  for (int f0 = 0; f0 < n_frames && e == E{} && !cancelled.load(); f0 += chunk) {
    const int n = n_frames - f0 < chunk ? n_frames - f0 : chunk;
    const int kept = carry && f0 > 0 ? 1 : 0;   // the predecessor from the chunk before
    if (f0 > 0) e = drain();
    if (e != E{}) break;
    pack_planes(pin[0], L, ref + f0, ref_stride, n);
    if (dis) pack_planes(pin[1], L, dis + f0, dis_stride, n);
    if (kept) e = seam(chunk);
    if (e == E{}) e = upload(carry, n);
    if (e == E{}) e = launch(carry - kept, n + kept, f0 - kept);
  }
  return e;
}

}  // namespace host
}  // namespace pqa
