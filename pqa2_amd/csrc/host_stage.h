// Host side of the staging of the side analyses and plane transforms (pqa_side.hip), free of any device call: how a chunk of
// frames of the call's own size lies in a pinned buffer, the copy of a caller's frames into it and of results back out, the
// walk over the chunks of a clip pair (stage_walk), the walk of a transform (transform_walk) and that of a transform with a
// window in time (window_walk).  The device is reached only through callables the caller passes in.  Header-only and plain
// C++17, as host_pack.h is, so that the CPU harnesses drive it under ThreadSanitizer / AddressSanitizer
// (tests/host_harness.cpp, tests/window_harness.cpp); pqa_ctx.h includes it as is.
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
// one plane a frame, as plane_layout stages it
inline ClipLayout plane_clip(size_t row_bytes, int h) {
  ClipLayout L;
  L.n_planes = 1;
  L.plane[0] = plane_layout(row_bytes, h);
  L.frame_bytes = L.plane[0].frame_bytes;
  return L;
}

// frames f0 ... f0 + n - 1 of a caller's clip into slots 0 ... n - 1 of a pinned buffer.  `frames` holds L.n_planes
// pointers per frame, frame-major; rows strides[p] bytes apart (negative: the rows lie bottom-up in the caller's memory).
// Only the L.plane[p].row_bytes bytes of a row that hold samples are read: the caller's last row may end at the end of its
// allocation.
inline void pack_clip(uint8_t* pin, const ClipLayout& L, const void* const* frames, const int64_t strides[3], int f0, int n) {
  for (int f = 0; f < n; ++f)
    for (int p = 0; p < L.n_planes; ++p)
      copy_plane_rows(pin + (size_t)f * L.frame_bytes + L.off[p], L.plane[p].pitch,
                      (const uint8_t*)frames[(size_t)(f0 + f) * L.n_planes + p], strides[p], L.plane[p].row_bytes, L.plane[p].h);
}

// The way back: slots 0 ... n - 1 of a pinned buffer into a caller's planes (`step` pointers per frame, frame-major, of which
// the first L.n_planes are written), row by row: the bytes between a destination row's end and the next row stay as they are.
inline void unpack_clip_out(const uint8_t* pin, const ClipLayout& L, void* const* planes, const int64_t strides[3], int step, int f0, int n) {
  for (int f = 0; f < n; ++f)
    for (int p = 0; p < L.n_planes; ++p)
      for (int y = 0; y < L.plane[p].h; ++y)
        memcpy((uint8_t*)planes[(size_t)(f0 + f) * step + p] + (int64_t)y * strides[p],
               pin + (size_t)f * L.frame_bytes + L.off[p] + (size_t)y * L.plane[p].pitch, L.plane[p].row_bytes);
}

// n_frames frames of `ref` and of `dis` (null: the one-clip form), L.n_planes pointers a frame, onto the device in chunks of
// at most `chunk`, each chunk launched before the next is packed.  Clip 0 is `ref` and clip 1 `dis`.  A pair packs clip k into
// pin[k]; the one-clip form packs chunk i into pin[i & 1], so that a chunk is packed under the upload of the chunk before.
// For every chunk:
//   drain(b)                     not before the first chunk, once per pinned buffer b the chunk packs: the buffer is packed
//                                again only after the upload that last read it has left it; the kernel of the chunk before
//                                may still run
//   seam(from_slot)              carry 1, not in the first chunk: device slot from_slot moves to device slot 0
//   pack, upload(b, k, slot, n)  per clip k: its n frames into slots 0 ... n - 1 of pin[b], then those to the clip's device
//                                slots slot ... slot + n - 1, in stream order behind the seam and the launch of the chunk
//                                before; the second clip is packed under the upload of the first
//   launch(slot, n, out_index)   n frames from device slot `slot` on; the results go `out_index` results into the output
// carry 0: a result per frame.  A chunk lands in slots 0 ... n - 1 and its launch writes results f0 ... f0 + n - 1.
// carry 1: a result per transition from a frame to the next.  The device buffers hold one slot more than a chunk: a chunk lands
// in slots 1 ... n, and before the next chunk overwrites them its last frame moves to slot 0 (only a full chunk has a
// successor, so that is slot `chunk`), where it is the predecessor of the next chunk's first.  So the first launch starts at
// slot 1 (n frames, n - 1 transitions from transition 0 on) and every later one at slot 0 (n + 1 frames, n transitions from
// f0 - 1 on).
// Stops at the first callable that returns something other than E{} (success) and returns that; stops before a chunk when
// `cancelled` is set and returns E{}.
template <class Drain, class Seam, class Upload, class Launch>
auto stage_walk(const ClipLayout& L, uint8_t* const pin[2], const void* const* ref, const int64_t ref_strides[3],
                const void* const* dis, const int64_t dis_strides[3], int n_frames, int chunk, int carry,
                const std::atomic<int>& cancelled, Drain drain, Seam seam, Upload upload, Launch launch) -> decltype(drain(0)) {
  using E = decltype(drain(0));
  E e{};
  for (int f0 = 0; f0 < n_frames && e == E{} && !cancelled.load(); f0 += chunk) {
    const int n = n_frames - f0 < chunk ? n_frames - f0 : chunk;
    const int kept = carry && f0 > 0 ? 1 : 0;   // the predecessor from the chunk before
    const int b = dis ? 0 : (f0 / chunk) & 1;
    if (f0 > 0) e = drain(b);
    if (e == E{} && f0 > 0 && dis) e = drain(1);
    if (e == E{} && kept) e = seam(chunk);
    if (e != E{}) break;
    pack_clip(pin[b], L, ref, ref_strides, f0, n);
    e = upload(b, 0, carry, n);
    if (e == E{} && dis) {
      pack_clip(pin[1], L, dis, dis_strides, f0, n);
      e = upload(1, 1, carry, n);
    }
    if (e == E{}) e = launch(carry - kept, n + kept, f0 - kept);
  }
  return e;
}

// A transform: n_frames frames of `src` (layout S) to as many of `dst` (layout D, dst_step pointers a frame), in chunks of at
// most `chunk`; `aux` (null: none) is a second input a frame, of the source's layout.  A chunk is through before the next is
// packed.  For every chunk of n frames from f0 on:
//   pack             the source frames into slots 0 ... n - 1 of pin[0], those of aux behind a whole chunk of them
//   upload(f0, n)    the packed frames to the device (f0 == 0: whatever else the launches read goes in front)
//   launch(n)        not after a failed upload
//   finish(e, n)     ALWAYS, with what upload and launch made of it: brings the n result frames to pin[1] and waits for the
//                    device, so that nothing still reads or writes the pinned buffers
//   copy out         the result frames from pin[1] into dst, sample bytes only
// Stops at the first finish() that returns something other than R{} (success), before the copy out, and returns that.
template <class Upload, class Launch, class Finish>
auto transform_walk(const ClipLayout& S, const ClipLayout& D, uint8_t* const pin[2], const void* const* src, const int64_t src_strides[3],
                    const void* const* aux, const int64_t aux_strides[3], void* const* dst, const int64_t dst_strides[3], int dst_step,
                    int n_frames, int chunk, Upload upload, Launch launch, Finish finish) -> decltype(finish(upload(0, 0), 0)) {
  using R = decltype(finish(upload(0, 0), 0));
  const size_t aux_at = S.frame_bytes * (size_t)(n_frames < chunk ? n_frames : chunk);
  for (int f0 = 0; f0 < n_frames; f0 += chunk) {
    const int n = n_frames - f0 < chunk ? n_frames - f0 : chunk;
    pack_clip(pin[0], S, src, src_strides, f0, n);
    if (aux) pack_clip(pin[0] + aux_at, S, aux, aux_strides, f0, n);
    auto e = upload(f0, n);
    if (e == decltype(e){}) e = launch(n);
    const R rc = finish(e, n);
    if (rc != R{}) return rc;
    unpack_clip_out(pin[1], D, dst, dst_strides, dst_step, f0, n);
  }
  return R{};
}

// A transform with a window in time: the outputs of source frame t read the frames t - 1, t and t + 1 (the first frame is its
// own predecessor and the last its own successor), `per` output frames a source frame, and every source frame is packed and
// uploaded ONCE.  The device buffer holds chunk + 2 slots (chunk >= 2): a chunk of n frames from f0 on lands in slots
// 2 ... n + 1, and before the next chunk overwrites them its last two frames move to slots 0 and 1 (only a full chunk has a
// successor, so those are slots chunk and chunk + 1), where they are the frames f0 - 2 and f0 - 1 of the next.  A chunk's
// launch emits the outputs of the source frames f0 - 1 ... f0 + n - 2 -- the first chunk's from frame 0 on --, and the clip's
// last chunk also those of the last frame.  For every chunk:
//   pack                            the source frames into slots 0 ... n - 1 of pin[0]
//   seam(from_slot)                 not in the first chunk: device slots from_slot, from_slot + 1 move to slots 0, 1
//   upload(slot, n)                 the packed frames to the device slots slot ... slot + n - 1
//   launch(slot, count, t0, m)      the frames the kernel may read are the `count` from device slot `slot` on (it clamps t - 1
//                                   and t + 1 to them itself); it emits the outputs of m of them from the t0-th on, m * per
//                                   frames, into the device's output slots 0 ...
//   finish(e, frames)               ALWAYS, with what the calls before made of it: brings `frames` result frames to pin[1] and
//                                   waits for the device, so that nothing still reads or writes the pinned buffers
//   copy out                        the result frames from pin[1] into dst, sample bytes only
// Stops at the first finish() that returns something other than R{} (success), before the copy out, and returns that.
template <class Seam, class Upload, class Launch, class Finish>
auto window_walk(const ClipLayout& S, const ClipLayout& D, uint8_t* const pin[2], const void* const* src, const int64_t src_strides[3],
                 void* const* dst, const int64_t dst_strides[3], int dst_step, int n_frames, int chunk, int per, Seam seam, Upload upload,
                 Launch launch, Finish finish) -> decltype(finish(upload(0, 0), 0)) {
  using R = decltype(finish(upload(0, 0), 0));
  for (int f0 = 0; f0 < n_frames; f0 += chunk) {
    const int n = n_frames - f0 < chunk ? n_frames - f0 : chunk;
    const int kept = f0 > 0 ? 2 : 0;                      // predecessors from the chunk before
    const int from = f0 > 0 ? f0 - 1 : 0;                 // the first source frame this launch emits
    const int m = f0 + n - 1 + (f0 + n == n_frames ? 1 : 0) - from;
    pack_clip(pin[0], S, src, src_strides, f0, n);
    auto e = kept ? seam(chunk) : decltype(upload(0, 0)){};
    if (e == decltype(e){}) e = upload(2, n);
    if (e == decltype(e){} && m > 0) e = launch(2 - kept, kept + n, from - (f0 - kept), m);
    const R rc = finish(e, m * per);
    if (rc != R{}) return rc;
    unpack_clip_out(pin[1], D, dst, dst_strides, dst_step, from * per, m * per);
  }
  return R{};
}

}  // namespace host
}  // namespace pqa
