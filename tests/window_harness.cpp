// CPU harness for host::window_walk (pqa2_amd/csrc/host_stage.h), the staging walk of a transform with a window in time
// (pqa_deinterlace): the device is a byte vector behind the four callables, the "kernel" a function of the frames t - 1, t and
// t + 1 that clamps them to the frames it was given, as deinterlace.hip does.  Checked for the frame counts around the chunk:
// every source frame is uploaded once and in order, every output is emitted once and in order and is the one of the whole clip,
// a failing callable stops the walk, and caller rows that end at the end of their allocation are neither over-read nor
// over-written (AddressSanitizer).  Built by tests/test_host_window.py under -fsanitize=address,undefined and -fsanitize=thread
// and run directly; nothing here is loaded into Python.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../pqa2_amd/csrc/host_stage.h"

using namespace pqa;

namespace {

constexpr int kRow = 5, kRows = 3;               // a plane of 5 bytes by 3 rows
constexpr int64_t kSrcStride = 7, kDstStride = 9;

int fails = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      ++fails;                                            \
      fprintf(stderr, "%s:%d: ", __FILE__, __LINE__);     \
      fprintf(stderr, __VA_ARGS__);                       \
      fprintf(stderr, "\n");                              \
    }                                                     \
  } while (0)

uint8_t src_byte(int t, int y, int x) { return (uint8_t)(t * 17 + y * 5 + x + 1); }
uint8_t out_byte(int n, int t, int k, int y, int x) {
  const int p = t > 0 ? t - 1 : 0, nx = t + 1 < n ? t + 1 : n - 1;
  return (uint8_t)(src_byte(p, y, x) + 3 * src_byte(t, y, x) + 5 * src_byte(nx, y, x) + 7 * k);
}

// a caller's plane: the last row ends at the end of the allocation
std::vector<uint8_t> caller_plane(int64_t stride) { return std::vector<uint8_t>((size_t)stride * (kRows - 1) + kRow, 0xEE); }

enum Fail { kNone, kSeam, kUpload, kLaunch, kFinish };

// walks a clip of n frames in chunks of `chunk`, `per` outputs a frame; fail_at: the chunk in which callable `fail` fails
void run(int n, int chunk, int per, Fail fail = kNone, int fail_at = 0) {
  const host::ClipLayout L = host::plane_clip(kRow, kRows);
  const size_t fb = L.frame_bytes;
  std::vector<std::vector<uint8_t>> src, dst;
  std::vector<const void*> sp;
  std::vector<void*> dp;
  for (int t = 0; t < n; ++t) {
    src.push_back(caller_plane(kSrcStride));
    for (int y = 0; y < kRows; ++y)
      for (int x = 0; x < kRow; ++x) src[t][(size_t)y * kSrcStride + x] = src_byte(t, y, x);
  }
  for (int k = 0; k < n * per; ++k) dst.push_back(caller_plane(kDstStride));
  for (auto& f : src) sp.push_back(f.data());
  for (auto& f : dst) dp.push_back(f.data());
  const int slots = n < chunk ? n : chunk;
  std::vector<uint8_t> pin0(fb * slots, 0x11), pin1(fb * (slots + 1) * per, 0x22);
  std::vector<uint8_t> dev(fb * (slots + 2), 0x33), dev_out(fb * (slots + 1) * per, 0x44);   // stale bytes everywhere
  uint8_t* const pin[2] = {pin0.data(), pin1.data()};

  int chunk_no = -1, uploaded = 0, emitted = 0, calls_after_failure = 0;
  bool failed = false, seamed = false;   // seamed: this chunk began with its seam
  const auto fails_here = [&](Fail f) {
    if (failed) ++calls_after_failure;
    if (fail == f && chunk_no == fail_at) {
      failed = true;
      return 7;
    }
    return 0;
  };
  const int64_t strides_s[3] = {kSrcStride, 0, 0}, strides_d[3] = {kDstStride, 0, 0};
  const int rc = host::window_walk(
      L, L, pin, sp.data(), strides_s, dp.data(), strides_d, 1, n, chunk, per,
      [&](int from_slot) {
        ++chunk_no;
        seamed = true;
        CHECK(chunk_no >= 1 && from_slot == chunk, "seam from slot %d in chunk %d", from_slot, chunk_no);
        if (const int e = fails_here(kSeam)) return e;
        memmove(dev.data(), dev.data() + fb * from_slot, 2 * fb);
        return 0;
      },
      [&](int slot, int m) {
        if (!seamed) ++chunk_no;   // only the first chunk begins with its upload
        seamed = false;
        CHECK(slot == 2 && m >= 1 && m <= slots, "upload of %d frames to slot %d", m, slot);
        if (const int e = fails_here(kUpload)) return e;
        for (int f = 0; f < m; ++f)   // every frame once and in order: the packed frame is the next one of the clip
          CHECK(pin0[fb * f] == src_byte(uploaded + f, 0, 0) && pin0[fb * f + L.plane[0].pitch * (kRows - 1) + kRow - 1] == src_byte(uploaded + f, kRows - 1, kRow - 1),
                "chunk %d packs frame %d at place %d wrongly", chunk_no, uploaded + f, f);
        memcpy(dev.data() + fb * slot, pin0.data(), fb * m);
        uploaded += m;
        return 0;
      },
      [&](int slot, int count, int t0, int m) {
        if (const int e = fails_here(kLaunch)) return e;
        CHECK(slot >= 0 && slot + count <= slots + 2 && t0 >= 0 && t0 + m <= count && m <= slots + 1, "launch %d %d %d %d", slot, count, t0, m);
        for (int i = 0; i < m; ++i)
          for (int k = 0; k < per; ++k) {
            const int t = t0 + i, p = t > 0 ? t - 1 : 0, nx = t + 1 < count ? t + 1 : count - 1;
            const uint8_t *P = dev.data() + fb * (slot + p), *Cc = dev.data() + fb * (slot + t), *Nn = dev.data() + fb * (slot + nx);
            uint8_t* O = dev_out.data() + fb * (i * per + k);
            for (int y = 0; y < kRows; ++y)
              for (int x = 0; x < kRow; ++x) {
                const size_t at = (size_t)y * L.plane[0].pitch + x;
                O[at] = (uint8_t)(P[at] + 3 * Cc[at] + 5 * Nn[at] + 7 * k);
              }
          }
        return 0;
      },
      [&](int e, int frames) {
        if (e == 0) e = fails_here(kFinish);
        if (e == 0) {
          CHECK((size_t)frames * fb <= pin1.size(), "finish brings back %d frames", frames);
          memcpy(pin1.data(), dev_out.data(), fb * frames);
          emitted += frames;
        }
        return e;
      });
  if (fail == kNone) {
    CHECK(rc == 0, "n %d: rc %d", n, rc);
    CHECK(uploaded == n && emitted == n * per, "n %d: %d frames uploaded, %d emitted", n, uploaded, emitted);
    for (int t = 0; t < n; ++t)
      for (int k = 0; k < per; ++k)
        for (int y = 0; y < kRows; ++y) {
          const uint8_t* row = dst[(size_t)t * per + k].data() + (size_t)y * kDstStride;
          for (int x = 0; x < kRow; ++x)
            CHECK(row[x] == out_byte(n, t, k, y, x), "n %d chunk %d per %d: output %d of frame %d at (%d, %d)", n, chunk, per, k, t, y, x);
          if (y + 1 < kRows) CHECK(row[kRow] == 0xEE && row[kDstStride - 1] == 0xEE, "n %d: the gap behind row %d of frame %d was written", n, y, t);
        }
  } else {
    CHECK(rc == 7, "n %d fail %d at %d: rc %d", n, (int)fail, fail_at, rc);
    // finish is called with the failure and passes it on; nothing else is called
    CHECK(calls_after_failure == 0, "n %d fail %d: %d calls after the failure", n, (int)fail, calls_after_failure);
    // the outputs of the chunks before the failing one are there, none of a later one
    const int done = fail_at == 0 ? 0 : fail_at * chunk - 1;
    for (int t = 0; t < n; ++t) {
      const uint8_t v = dst[(size_t)t * per][0];
      if (t < done) CHECK(v == out_byte(n, t, 0, 0, 0), "n %d fail %d: frame %d is missing", n, (int)fail, t);
      else CHECK(v == 0xEE, "n %d fail %d: frame %d was written after the failure", n, (int)fail, t);
    }
  }
}

}  // namespace

int main() {
  for (int per = 1; per <= 2; ++per) {
    for (int n : {1, 2, 8, 9, 10, 16, 17}) run(n, 8, per);
    for (int n : {1, 2, 3, 4, 5, 7}) run(n, 2, per);   // the smallest chunk the walk allows
  }
  for (Fail f : {kUpload, kLaunch, kFinish})
    for (int at : {0, 1, 2}) run(17, 8, 2, f, at);
  for (int at : {1, 2}) run(17, 8, 1, kSeam, at);
  if (fails) {
    fprintf(stderr, "%d checks failed\n", fails);
    return 1;
  }
  printf("window harness ok\n");
  return 0;
}
