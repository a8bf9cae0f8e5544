// CPU harness of pqa2_amd/csrc/host_packed.h under AddressSanitizer + UBSan (tests/test_packed_host.py builds and runs it):
// the row / file geometry of the packed formats, the copy of a caller's frames -- packed or planar -- into a staging buffer
// and the copy of unpacked planes back out.  Every caller buffer is a heap block of EXACTLY the bytes the contract lets the
// library touch (the last row ends at its last sample), so one byte read or written beyond it is a sanitizer report.
// No device: the staging buffers are plain heap memory here.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../pqa2_amd/csrc/host_packed.h"

using namespace pqa;
using namespace pqa::host;

#define CHECK(x)                                                        \
  do {                                                                  \
    if (!(x)) {                                                         \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #x); \
      exit(1);                                                          \
    }                                                                   \
  } while (0)

static uint8_t pattern(size_t i, int salt) { return (uint8_t)(1 + (i * 131 + (size_t)salt * 17) % 255); }

// a caller's plane / packed frame: h rows `stride` apart, the block ends with the last row's last sample
static std::unique_ptr<uint8_t[]> exact_block(int h, int64_t stride, size_t row_bytes, int salt, size_t* bytes) {
  *bytes = (size_t)stride * (h - 1) + row_bytes;
  std::unique_ptr<uint8_t[]> b(new uint8_t[*bytes]);
  for (size_t i = 0; i < *bytes; ++i) b[i] = pattern(i, salt);
  return b;
}

static void geometry() {
  const int ws[] = {16, 17, 19, 48, 50, 52, 96, 1280, 1920};
  const int64_t row8[] = {32, 36, 40, 96, 100, 104, 192, 2560, 3840};
  const int64_t row10[] = {48, 48, 64, 128, 144, 144, 256, 3424, 5120};
  const int64_t file10[] = {128, 128, 128, 128, 256, 256, 256, 3456, 5120};
  for (int i = 0; i < 9; ++i) {
    CHECK(packed_min_row_bytes(FMT_UYVY, ws[i]) == row8[i] && packed_min_row_bytes(FMT_YUYV, ws[i]) == row8[i]);
    CHECK(packed_file_stride(FMT_UYVY, ws[i]) == row8[i]);
    CHECK(packed_min_row_bytes(FMT_V210, ws[i]) == row10[i] && packed_file_stride(FMT_V210, ws[i]) == file10[i]);
  }
  CHECK(packed_format(3) && packed_format(4) && packed_format(5) && !packed_format(0) && !packed_format(1) && !packed_format(2) && !packed_format(6));
  CHECK(packed_bit_depth(FMT_V210) == 10 && packed_bit_depth(FMT_UYVY) == 8 && packed_sample_bytes(FMT_V210) == 2);
  const ClipLayout P = packed_layout(FMT_V210, 50, 16);
  CHECK(P.n_planes == 1 && P.plane[0].row_bytes == 144 && P.plane[0].pitch == 144 && P.frame_bytes == 144 * 16);
  const ClipLayout U = unpacked_layout(FMT_UYVY, 50, 16, 3);
  CHECK(U.plane[0].row_bytes == 50 && U.plane[0].pitch == 64 && U.plane[1].row_bytes == 25 && U.plane[1].pitch == 32);
  CHECK(U.off[1] == 64 * 16 && U.off[2] == 64 * 16 + 32 * 16 && U.frame_bytes == 64 * 16 + 2 * 32 * 16);
  CHECK(unpacked_layout(FMT_V210, 50, 16, 1).frame_bytes == 112 * 16);
}

// packed frames in: equal strides (one memcpy per frame) and padded ones (row by row), from exact blocks
static void pack_packed(uint32_t format, int w, int h, int64_t extra) {
  const ClipLayout L = packed_layout(format, w, h);
  const int n = 5, f0 = 1, m = 3;
  const int64_t strides[3] = {L.plane[0].pitch + extra, 0, 0};
  std::vector<std::unique_ptr<uint8_t[]>> keep;
  std::vector<const void*> frames;
  for (int f = 0; f < n; ++f) {
    size_t bytes;
    keep.push_back(exact_block(h, strides[0], L.plane[0].row_bytes, f, &bytes));
    frames.push_back(keep.back().get());
  }
  std::unique_ptr<uint8_t[]> pin(new uint8_t[L.frame_bytes * m]);   // exactly a chunk
  memset(pin.get(), 0, L.frame_bytes * m);
  pack_clip(pin.get(), L, frames.data(), strides, f0, m);
  for (int f = 0; f < m; ++f)
    for (int y = 0; y < h; ++y)
      CHECK(!memcmp(pin.get() + (size_t)f * L.frame_bytes + (size_t)y * L.plane[0].pitch,
                    (const uint8_t*)frames[f0 + f] + (int64_t)y * strides[0], L.plane[0].row_bytes));
  // the same copy cut into tasks for the pack pool (small tasks here, so that a plane is several): the bytes pack_clip wrote
  std::unique_ptr<uint8_t[]> pin2(new uint8_t[L.frame_bytes * m]);
  memset(pin2.get(), 0, L.frame_bytes * m);
  std::vector<PackTask> tasks;
  pack_clip_tasks(tasks, pin2.get(), L, frames.data(), strides, f0, m, 5 * L.plane[0].row_bytes + 1);
  CHECK((int)tasks.size() == m * ((h + 4) / 5) && tasks.front().frame == 0 && tasks.back().frame == m - 1);
  for (const PackTask& t : tasks) CHECK(run_pack_task(t));
  for (int f = 0; f < m; ++f)
    for (int y = 0; y < h; ++y)   // the samples: what lies between a row's end and the next row is nobody's
      CHECK(!memcmp(pin.get() + (size_t)f * L.frame_bytes + (size_t)y * L.plane[0].pitch,
                    pin2.get() + (size_t)f * L.frame_bytes + (size_t)y * L.plane[0].pitch, L.plane[0].row_bytes));
}

// planar frames in, with the slot alignment pqa_submit_packed uses, and planes back out into padded rows
static void planar_round_trip(int w, int h, int es, int n_planes) {
  const int cw = (w + 1) / 2;
  const size_t rb[3] = {(size_t)w * es, (size_t)cw * es, (size_t)cw * es};
  const int rows[3] = {h, h, h};
  const ClipLayout L = clip_layout(n_planes, rb, rows, 64, 256);
  for (int p = 0; p < n_planes; ++p) CHECK(L.plane[p].pitch % 64 == 0 && L.off[p] % 256 == 0 && L.plane[p].pitch >= (int64_t)rb[p]);
  const int n = 4, f0 = 2, m = 2;
  const int64_t strides[3] = {(int64_t)rb[0] + 3 * es, (int64_t)rb[1], (int64_t)rb[2] + es};
  std::vector<std::unique_ptr<uint8_t[]>> keep;
  std::vector<const void*> planes;
  for (int f = 0; f < n; ++f)
    for (int p = 0; p < n_planes; ++p) {
      size_t bytes;
      keep.push_back(exact_block(h, strides[p], rb[p], f * 3 + p, &bytes));
      planes.push_back(keep.back().get());
    }
  std::unique_ptr<uint8_t[]> pin(new uint8_t[L.frame_bytes * m]);
  memset(pin.get(), 0, L.frame_bytes * m);
  pack_clip(pin.get(), L, planes.data(), strides, f0, m);
  {
    std::unique_ptr<uint8_t[]> pin2(new uint8_t[L.frame_bytes * m]);
    memset(pin2.get(), 0, L.frame_bytes * m);
    std::vector<PackTask> tasks;
    pack_clip_tasks(tasks, pin2.get(), L, planes.data(), strides, f0, m, 1u << 20);
    for (const PackTask& t : tasks) CHECK(run_pack_task(t));
    for (int f = 0; f < m; ++f)
      for (int p = 0; p < n_planes; ++p)
        for (int y = 0; y < h; ++y) {
          const size_t at = (size_t)f * L.frame_bytes + L.off[p] + (size_t)y * L.plane[p].pitch;
          CHECK(!memcmp(pin.get() + at, pin2.get() + at, rb[p]));
        }
  }
  // ... and out again: 3 pointers per frame, rows padded, the padding must keep its sentinel
  const int64_t out_strides[3] = {(int64_t)rb[0] + 5, (int64_t)rb[1] + 1, (int64_t)rb[2]};
  std::vector<std::unique_ptr<uint8_t[]>> out_keep;
  std::vector<void*> out(3 * (f0 + m), nullptr);
  std::vector<size_t> out_bytes(3 * (f0 + m), 0);
  for (int f = f0; f < f0 + m; ++f)
    for (int p = 0; p < n_planes; ++p) {
      out_bytes[3 * f + p] = (size_t)out_strides[p] * (h - 1) + rb[p];
      out_keep.emplace_back(new uint8_t[out_bytes[3 * f + p]]);
      memset(out_keep.back().get(), 0xEE, out_bytes[3 * f + p]);
      out[3 * f + p] = out_keep.back().get();
    }
  unpack_clip_out(pin.get(), L, out.data(), out_strides, 3, f0, m);
  for (int f = f0; f < f0 + m; ++f)
    for (int p = 0; p < n_planes; ++p)
      for (int y = 0; y < h; ++y) {
        const uint8_t* o = (const uint8_t*)out[3 * f + p] + (int64_t)y * out_strides[p];
        CHECK(!memcmp(o, (const uint8_t*)planes[(size_t)f * n_planes + p] + (int64_t)y * strides[p], rb[p]));
        if (y + 1 < h)
          for (int64_t i = (int64_t)rb[p]; i < out_strides[p]; ++i) CHECK(o[i] == 0xEE);
      }
}

int main(int argc, char** argv) {
  if (argc >= 3 && !strcmp(argv[1], "--selftest") && !strcmp(argv[2], "overflow")) {
    // the sanitizer must be alive: a staging buffer one byte short of a chunk
    const ClipLayout L = packed_layout(FMT_UYVY, 48, 16);   // rows without padding: the copy fills the chunk to its last byte
    size_t bytes;
    auto src = exact_block(16, L.plane[0].pitch, L.plane[0].row_bytes, 0, &bytes);
    const void* frames[1] = {src.get()};
    const int64_t strides[3] = {L.plane[0].pitch, 0, 0};
    std::unique_ptr<uint8_t[]> pin(new uint8_t[L.frame_bytes - 1]);
    pack_clip(pin.get(), L, frames, strides, 0, 1);
    printf("%d\n", pin[0]);
    return 0;
  }
  geometry();
  const int sizes[][2] = {{16, 16}, {17, 16}, {19, 17}, {48, 16}, {50, 16}, {52, 20}, {96, 18}, {642, 362}};
  for (const auto& s : sizes) {
    for (uint32_t fmt : {(uint32_t)FMT_UYVY, (uint32_t)FMT_YUYV, (uint32_t)FMT_V210}) {
      pack_packed(fmt, s[0], s[1], 0);
      pack_packed(fmt, s[0], s[1], fmt == FMT_V210 ? 4 : 3);
      pack_packed(fmt, s[0], s[1], packed_file_stride(fmt, s[0]) - packed_min_row_bytes(fmt, s[0]));
    }
    for (int es = 1; es <= 2; ++es) {
      planar_round_trip(s[0], s[1], es, 3);
      planar_round_trip(s[0], s[1], es, 1);
    }
  }
  printf("packed harness ok\n");
  return 0;
}
