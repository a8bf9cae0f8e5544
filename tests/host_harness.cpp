// CPU harness for the library's device-free host code (pqa2_amd/csrc/host_pack.h, host_ring.h, host_stage.h, host_chain.h): built with
// -fsanitize=thread and with -fsanitize=address,undefined by tests/test_host_sanitizers.py and driven through the call
// sequences the GPU tests put the real library through (tests/test_gpu_configs.py PQA_ESTATE cases, the truncated-file cases
// of tests/test_gpu_engine.py, a cancel flag raised from another thread; the pair staging of the side analyses against fake
// device buffers of exactly the reserved sizes, as tests/test_gpu_pair_entries.py and the chunk tests of the six analyses put
// it; the frame histories of motion, xpsnr, siti and the integrity SAD through the shard, reset and split-call sequences of
// tests/test_gpu_xpsnr.py, test_gpu_siti.py and test_gpu_integrity.py, and a random walk beside the four state machines the
// one type replaced).  Memory / race safety, for the pair staging which frames a launch sees, for the histories which frame a
// batch reads as its predecessor: no parity claim.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fcntl.h>
#include <memory>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "../pqa2_amd/csrc/host_chain.h"
#include "../pqa2_amd/csrc/host_pack.h"
#include "../pqa2_amd/csrc/host_ring.h"
#include "../pqa2_amd/csrc/host_stage.h"

using namespace pqa::host;

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "CHECK failed at %s:%d: %s\n", __FILE__, __LINE__, #x); exit(1); } } while (0)

struct Geometry { int w, h, n_planes; };

// The task list of m frame pairs as submit_run (pqa_api.hip) cuts it: the library's builder per frame and side, the frames
// frame_step bytes apart behind src, into slots of two sides each.
static std::vector<PackTask> run_tasks(const ClipLayout& L, int m, uint8_t* slots, const PlaneSrc (&src)[2][3], int64_t frame_step,
                                       unsigned task_bytes) {
  std::vector<PackTask> t;
  for (int k = 0; k < m; ++k)
    for (int side = 0; side < 2; ++side)
      pack_frame_tasks(t, L, slots + (size_t)(2 * k + side) * L.frame_bytes, src[side], frame_step, k, k, task_bytes);
  return t;
}

static void pack_scenarios(const char* dir) {
  const Geometry g{322, 182, 3};   // odd width: staging rows are padded, so every plane is packed row by row
  const int n = 11, HB = 4;
  const int cw = (g.w + 1) / 2, ch = (g.h + 1) / 2;
  const int64_t frame_bytes = (int64_t)g.w * g.h + 2ll * cw * ch;
  const int64_t file_plane_off[3] = {0, (int64_t)g.w * g.h, (int64_t)g.w * g.h + (int64_t)cw * ch};
  const size_t row_bytes[3] = {(size_t)g.w, (size_t)cw, (size_t)cw};
  const int rows[3] = {g.h, ch, ch};
  const ClipLayout L = clip_layout(g.n_planes, row_bytes, rows, 64, 256);   // one side of the context's slot
  const int64_t slot_pitch[3] = {L.plane[0].pitch, L.plane[1].pitch, L.plane[2].pitch};
  size_t plane_off[2][3];
  for (int side = 0; side < 2; ++side)
    for (int p = 0; p < 3; ++p) plane_off[side][p] = side * L.frame_bytes + L.off[p];
  const size_t slot_bytes = 2 * L.frame_bytes;
  // both clips from memory (frame `first` in front) or from the files, plane p of the files' first frame at off[p]
  struct Sources { PlaneSrc s[2][3]; };
  const auto sources = [&](const uint8_t* const mem[2], const int fds[2], const int64_t off[3]) {
    Sources r;
    for (int side = 0; side < 2; ++side)
      for (int p = 0; p < 3; ++p)
        r.s[side][p] = mem[side] ? PlaneSrc{mem[side] + off[p], (int64_t)row_bytes[p], -1, 0} : PlaneSrc{nullptr, (int64_t)row_bytes[p], fds[side], off[p]};
    return r;
  };
  std::mt19937 rng(7);
  std::vector<uint8_t> clip[2];
  char path[2][512];
  int fds[2];
  for (int side = 0; side < 2; ++side) {
    clip[side].resize((size_t)frame_bytes * n);
    for (auto& b : clip[side]) b = (uint8_t)rng();
    snprintf(path[side], sizeof path[side], "%s/harness_%d.yuv", dir, side);
    FILE* f = fopen(path[side], "wb");
    CHECK(f && fwrite(clip[side].data(), 1, clip[side].size(), f) == clip[side].size());
    fclose(f);
    fds[side] = open(path[side], O_RDONLY);
    CHECK(fds[side] >= 0);
  }
  std::vector<uint8_t> slots(slot_bytes * HB);
  const auto verify = [&](int first, int m) {
    for (int k = 0; k < m; ++k)
      for (int side = 0; side < 2; ++side)
        for (int p = 0; p < 3; ++p) {
          const int pw = p ? cw : g.w, ph = p ? ch : g.h;
          for (int y = 0; y < ph; ++y)
            CHECK(!memcmp(slots.data() + (size_t)k * slot_bytes + plane_off[side][p] + (size_t)y * slot_pitch[p],
                          clip[side].data() + (size_t)(first + k) * frame_bytes + file_plane_off[p] + (size_t)y * pw, (size_t)pw));
        }
  };
  std::atomic<int> cancelled{0};
  for (int helpers : {1, 3, 7}) {
    PackPool pool(helpers);
    // (1) memory sources, frame by frame (pqa_submit), plain run()
    for (int i = 0; i < n; ++i) {
      const uint8_t* mem[2] = {clip[0].data() + (size_t)i * frame_bytes, clip[1].data() + (size_t)i * frame_bytes};
      auto t = run_tasks(L, 1, slots.data(), sources(mem, fds, file_plane_off).s, 0, 16 << 10);
      CHECK(pool.run(t.data(), (int)t.size()));
      verify(i, 1);
    }
    // (2) file sources in runs (pqa_submit_fd_run): frames are handed over in order, on the caller's thread
    const uint8_t* nomem[2] = {nullptr, nullptr};
    const auto caller = std::this_thread::get_id();
    for (int first = 0; first < n; first += HB) {
      const int m = n - first < HB ? n - first : HB;
      std::fill(slots.begin(), slots.end(), 0);
      const int64_t base[3] = {file_plane_off[0] + first * frame_bytes, file_plane_off[1] + first * frame_bytes, file_plane_off[2] + first * frame_bytes};
      auto t = run_tasks(L, m, slots.data(), sources(nomem, fds, base).s, frame_bytes, 24 << 10);
      int next = 0;
      const bool ok = pool.run_frames(t.data(), (int)t.size(), m, [&](int k) {
        CHECK(k == next && std::this_thread::get_id() == caller);
        verify(first + k, 0);   // (the slot of frame k is complete here: checked below for all of them)
        ++next;
        return true;
      });
      CHECK(ok && next == m);
      verify(first, m);
    }
    // (3) a file that ends inside frame 2 of a run of 4: false, and no frame from the incomplete one on is handed over
    {
      char sp[512];
      snprintf(sp, sizeof sp, "%s/harness_short.yuv", dir);
      FILE* f = fopen(sp, "wb");
      CHECK(f && fwrite(clip[0].data(), 1, (size_t)(2 * frame_bytes + 1000), f) == (size_t)(2 * frame_bytes + 1000));
      fclose(f);
      int sfd[2] = {open(sp, O_RDONLY), fds[1]};
      CHECK(sfd[0] >= 0);
      auto t = run_tasks(L, 4, slots.data(), sources(nomem, sfd, file_plane_off).s, frame_bytes, 24 << 10);
      std::vector<int> seen;
      CHECK(!pool.run_frames(t.data(), (int)t.size(), 4, [&](int k) { seen.push_back(k); return true; }));
      for (size_t i = 0; i < seen.size(); ++i) CHECK(seen[i] == (int)i && seen[i] < 2);
      // a callback that fails (the upload could not be queued) ends the hand-over too
      auto t2 = run_tasks(L, 3, slots.data(), sources(nomem, fds, file_plane_off).s, frame_bytes, 24 << 10);
      int calls = 0;
      CHECK(!pool.run_frames(t2.data(), (int)t2.size(), 3, [&](int) { ++calls; return false; }) && calls == 1);
      close(sfd[0]);
      remove(sp);
    }
    // (4) pqa_cancel from another thread while a submit loop runs: the loop polls the flag between runs, as submit_run does
    {
      cancelled.store(0);
      std::thread other([&] { std::this_thread::sleep_for(std::chrono::milliseconds(2)); cancelled.store(1); });
      int submitted = 0;
      for (int rep = 0; rep < 400 && !cancelled.load(); ++rep) {
        auto t = run_tasks(L, HB, slots.data(), sources(nomem, fds, file_plane_off).s, frame_bytes, 24 << 10);
        CHECK(pool.run_frames(t.data(), (int)t.size(), HB, [&](int) { return true; }));
        submitted += HB;
      }
      other.join();
      CHECK(submitted > 0);
    }
  }   // the pool is destroyed while idle here, three times
  for (int side = 0; side < 2; ++side) { close(fds[side]); remove(path[side]); }
}

// A packed clip as pqa_submit_packed stages it: one plane of minimum row bytes a frame, the caller's rows unpadded (one copy a
// task) and padded (row by row), every caller frame a heap block that ends with its last sample; tasks of a few rows.
static void packed_clip_scenarios() {
  const int h = 18, n = 5, f0 = 1, m = 3;
  for (size_t row : {(size_t)192, (size_t)100, (size_t)144}) {   // UYVY at 96 and 50 wide, v210 at 52
    const ClipLayout L = plane_clip(row, h);
    for (int64_t stride : {(int64_t)row, (int64_t)row + 12}) {
      std::vector<std::unique_ptr<uint8_t[]>> frames;
      for (int f = 0; f < n; ++f) {
        const size_t bytes = (size_t)stride * (h - 1) + row;
        frames.emplace_back(new uint8_t[bytes]);
        for (size_t i = 0; i < bytes; ++i) frames.back()[i] = (uint8_t)(1 + (i * 131 + f * 17) % 255);
      }
      std::unique_ptr<uint8_t[]> pin(new uint8_t[L.frame_bytes * m]);   // exactly a chunk
      memset(pin.get(), 0, L.frame_bytes * m);
      std::vector<PackTask> t;
      for (int f = 0; f < m; ++f) {
        const PlaneSrc src[3] = {{frames[f0 + f].get(), stride, -1, 0}, {}, {}};
        pack_frame_tasks(t, L, pin.get() + (size_t)f * L.frame_bytes, src, 0, 0, f, 5 * row + 1);
      }
      CHECK((int)t.size() == m * ((h + 4) / 5) && t.front().frame == 0 && t.back().frame == m - 1);
      PackPool pool(2);
      CHECK(pool.run(t.data(), (int)t.size()));
      for (int f = 0; f < m; ++f)
        for (int y = 0; y < h; ++y)
          CHECK(!memcmp(pin.get() + (size_t)f * L.frame_bytes + (size_t)y * L.plane[0].pitch, frames[f0 + f].get() + (int64_t)y * stride, row));
    }
  }
}

// host::launch_size: equal launches of at most B frames, as few as launches of B would be
static void launch_size_properties() {
  CHECK(launch_size(300, 32) == 30);
  for (int B = 1; B <= 40; ++B) {
    CHECK(launch_size(0, B) == 0);
    for (int n = 1; n <= 700; ++n) {
      const int per = launch_size(n, B);
      CHECK(per >= 1 && per <= B && (n + per - 1) / per == (n + B - 1) / B);
    }
  }
  CHECK(launch_size(16384, 256) == 256 && launch_size(16385, 256) <= 256);
}

static void ring_scenarios() {
  RecordRing r;
  r.init(4);
  int64_t f = -1, holder = -1, bad = -1;
  bool never = false;
  uint64_t need = 0;
  CHECK(!r.collectable(0, 1, &need, &bad, &never, &holder) && never && bad == 0);       // nothing was ever submitted
  CHECK(r.can_submit(0, 4, &f, &holder));
  r.claim(0, 2, 1);
  r.claim(2, 2, 2);
  CHECK(!r.can_submit(4, 1, &f, &holder) && f == 4 && holder == 0);                      // would overwrite frame 0's record
  CHECK(r.can_submit(0, 4, &f, &holder));                                                // a re-run of the same frames may
  CHECK(r.collectable(0, 4, &need, &bad, &never, &holder) && need == 2);
  CHECK(r.collectable(0, 2, &need, &bad, &never, &holder) && need == 1);                 // ... waits for ITS batch only
  r.mark_collected(0, 1);
  CHECK(r.can_submit(4, 1, &f, &holder));
  CHECK(!r.can_submit(4, 2, &f, &holder) && f == 5 && holder == 1);
  r.claim(4, 1, 3);                                                                      // wraps onto slot 0
  CHECK(!r.collectable(0, 1, &need, &bad, &never, &holder) && !never && bad == 0 && holder == 4);   // overwritten
  CHECK(r.collectable(4, 1, &need, &bad, &never, &holder) && need == 3);
  CHECK(r.collectable(1, 3, &need, &bad, &never, &holder) && need == 2);
  r.mark_collected(1, 3);
  r.mark_collected(4, 1);
  CHECK(r.can_submit(5, 4, &f, &holder));
  r.claim(5, 4, 4);                                                                      // frames 5..8 on slots 1, 2, 3, 0
  CHECK(r.collectable(5, 4, &need, &bad, &never, &holder) && need == 4);
  CHECK(!r.can_submit(9, 1, &f, &holder) && holder == 5);
  r.reset();
  CHECK(r.can_submit(9, 4, &f, &holder));
  CHECK(!r.collectable(5, 1, &need, &bad, &never, &holder) && never);
  // a long walk: submit in batches of 3, collect two batches late; never a false conflict, never a lost record
  r.init(16);
  uint64_t seq = 0;
  for (int64_t first = 0; first < 3000; first += 3) {
    CHECK(r.can_submit(first, 3, &f, &holder));
    r.claim(first, 3, ++seq);
    if (first >= 6) {
      CHECK(r.collectable(first - 6, 3, &need, &bad, &never, &holder) && need == seq - 2);
      r.mark_collected(first - 6, 3);
    }
  }
}

// ---- the pair staging (host_stage.h) ---------------------------------------------------------------------------------------
// The device is two heap buffers of exactly the bytes pqa_side.hip reserves; the callables copy as the HIP calls there do and
// log themselves.  A launch notes which source frames lie in the slots it was given.  For each pinned buffer the model notes
// whether an upload out of it is in flight: upload sets the flag, drain clears it, and a buffer that was just packed must not
// carry it.
static uint8_t sample_of(int clip, int frame, int y, size_t x) { return (uint8_t)(clip * 131 + frame * 7 + y * 31 + (int)x * 3 + 1); }

struct StageCase {
  size_t row_bytes;
  int h;
  int64_t stride_extra;   // 0: the source rows lie a packed pitch apart (copy_plane_rows takes its single memcpy)
  int n_frames, carry, clips;
  char fail_in = 0;       // 'D', 'S', 'U' or 'L': that callable returns 7 in the second chunk
  bool cancel = false;    // the first launch raises the cancel flag
  int planes = 1;         // per frame; 3: as pqa_colour_moments stages them (plane p is 5 * p bytes a row wider, planes 256 bytes apart)
};

struct Launched { int out_index; std::vector<int> seen[2]; };

static void stage_case(const StageCase& k) {
  const int chunk = 8, slots = k.n_frames < chunk ? k.n_frames : chunk;
  const PlaneLayout L = plane_layout(k.row_bytes, k.h);
  CHECK(L.pitch % 16 == 0 && L.pitch >= (int64_t)k.row_bytes && L.pitch < (int64_t)k.row_bytes + 16 && L.frame_bytes == (size_t)L.pitch * k.h);
  const int np = k.planes;
  const size_t rb[3] = {k.row_bytes, k.row_bytes + 5, k.row_bytes + 10};
  const int rows[3] = {k.h, k.h, k.h};
  const ClipLayout C = np == 1 ? plane_clip(k.row_bytes, k.h) : clip_layout(np, rb, rows, 16, 256);
  CHECK(C.n_planes == np && C.plane[0].pitch == L.pitch && (np == 3 || C.frame_bytes == L.frame_bytes));
  int64_t strides[3];
  for (int p = 0; p < np; ++p) {
    strides[p] = C.plane[p].pitch + k.stride_extra;
    CHECK(C.off[p] % (np == 1 ? 16 : 256) == 0 && C.off[p] + C.plane[p].frame_bytes <= (p + 1 < np ? C.off[p + 1] : C.frame_bytes));
  }
  // every source plane is an allocation of its own that ends with the last sample of its last row
  std::vector<std::unique_ptr<uint8_t[]>> src[2];
  std::vector<const void*> list[2];
  std::unique_ptr<uint8_t[]> pin[2], dev[2];
  for (int c = 0; c < k.clips; ++c) {
    for (int f = 0; f < k.n_frames; ++f)
      for (int p = 0; p < np; ++p) {
        const int64_t stride = strides[p];
        src[c].emplace_back(new uint8_t[(size_t)stride * (k.h - 1) + rb[p]]);
        for (int y = 0; y < k.h; ++y)
          for (size_t x = 0; x < (size_t)(y < k.h - 1 ? stride : (int64_t)rb[p]); ++x)
            src[c].back()[(size_t)y * stride + x] = x < rb[p] ? sample_of(c, f, y, x + 5 * p) : 0xee;
        list[c].push_back(src[c].back().get());
      }
    dev[c].reset(new uint8_t[C.frame_bytes * (slots + k.carry)]);
  }
  for (auto& b : pin) b.reset(new uint8_t[C.frame_bytes * slots]);   // one clip: its chunks alternate between the two
  uint8_t* const pins[2] = {pin[0].get(), pin[1].get()};
  const size_t fb = C.frame_bytes;
  std::string log;
  std::vector<Launched> launches;
  std::atomic<int> cancelled{0};
  int chunk_no = 0;   // of the chunk a callable belongs to: upload() opens a chunk's device work, drain() the chunk's host work
  bool in_flight[2] = {false, false};
  const auto fails = [&](char who) { log += who; return k.fail_in == who && chunk_no == 1 ? 7 : 0; };
  const int rc = stage_walk(
      C, pins, list[0].data(), strides, k.clips == 2 ? list[1].data() : nullptr, strides, k.n_frames, chunk, k.carry, cancelled,
      [&](int b) {   // once per pinned buffer the chunk packs: a pair 0 then 1, one clip the chunk's parity
        if (k.clips == 1 || b == 0) ++chunk_no;
        CHECK(k.clips == 2 ? (b == 0 || b == 1) : b == (chunk_no & 1));
        in_flight[b] = false;
        return fails('D');
      },
      [&](int from) {
        CHECK(from >= 1 && from < slots + k.carry);
        for (int c = 0; c < k.clips; ++c) memcpy(dev[c].get(), dev[c].get() + (size_t)from * fb, fb);
        return fails('S');
      },
      [&](int b, int c, int slot, int n) {
        CHECK(c < k.clips && b == (k.clips == 2 ? c : chunk_no & 1) && slot == k.carry && n >= 1 && n <= slots);
        CHECK(!in_flight[b]);   // the pack in front of this upload wrote the buffer
        memcpy(dev[c].get() + (size_t)slot * fb, pins[b], fb * n);
        in_flight[b] = true;
        return fails('U');
      },
      [&](int slot, int n, int out_index) {
        CHECK(slot >= 0 && n >= 1 && slot + n <= slots + k.carry);
        Launched l{out_index, {}};
        for (int c = 0; c < k.clips; ++c)
          for (int i = 0; i < n; ++i) {   // the frame whose samples lie in slot + i
            const uint8_t* plane = dev[c].get() + (size_t)(slot + i) * fb;
            const int f = (uint8_t)(plane[0] - sample_of(c, 0, 0, 0)) / 7;   // 24 frames at most: 7 f stays below 256
            CHECK(f >= 0 && f < k.n_frames);
            for (int p = 0; p < np; ++p)
              for (int y = 0; y < k.h; ++y)
                CHECK(!memcmp(plane + C.off[p] + (size_t)y * C.plane[p].pitch, src[c][(size_t)f * np + p].get() + (size_t)y * strides[p], rb[p]));
            l.seen[c].push_back(f);
          }
        launches.push_back(l);
        if (k.cancel) cancelled.store(1);
        return fails('L');
      });
  // the calls, restated: per chunk drain (not the first), seam (carry 1, not the first), upload, launch; drain and upload
  // once per pinned buffer, so twice for a pair
  std::string want;
  bool failed = false;
  const int n_chunks = (k.n_frames + chunk - 1) / chunk;
  for (int i = 0; i < n_chunks; ++i) {
    for (char who : {'D', 'S', 'U', 'L'}) {
      if ((who == 'D' && i == 0) || (who == 'S' && (i == 0 || !k.carry))) continue;
      for (int c = 0; c < (who == 'D' || who == 'U' ? k.clips : 1); ++c) {
        want += who;
        if (i == 1 && who == k.fail_in) { failed = true; goto done; }
      }
    }
    if (k.cancel) break;
  }
done:
  CHECK(log == want);
  CHECK(rc == (failed ? 7 : 0));
  if (k.fail_in || k.cancel) return;
  // the results, restated: result r is written once, in order, by a launch that saw frames r ... r + carry of both clips where
  // the kernel reads them -- at plane r - out_index (and the next) of the launch
  int next = 0;
  for (const Launched& l : launches) {
    CHECK(l.out_index == next);
    for (int c = 0; c < k.clips; ++c)
      for (size_t i = 0; i < l.seen[c].size(); ++i) CHECK(l.seen[c][i] == l.out_index + (int)i);
    next += (int)l.seen[0].size() - k.carry;
  }
  CHECK(next == (k.n_frames > k.carry ? k.n_frames - k.carry : 0));
}

static void stage_scenarios() {
  for (size_t row_bytes : {1, 15, 16, 17, 33})
    for (int h : {1, 3})
      for (int64_t extra : {0, 7})
        for (int n : {0, 1, 2, 8, 9, 16, 17, 24})
          for (int carry : {0, 1})
            for (int clips : {2, 1}) stage_case(StageCase{row_bytes, h, extra, n, carry, clips});
  // three planes a frame (pqa_colour_moments, pqa_delta_itp: two clips, a result per frame)
  for (size_t row_bytes : {1, 15, 16, 17, 33})
    for (int h : {1, 3})
      for (int64_t extra : {0, 7})
        for (int n : {0, 1, 8, 9, 17}) stage_case(StageCase{row_bytes, h, extra, n, 0, 2, 0, false, 3});
  for (char who : {'D', 'U', 'L'}) stage_case(StageCase{17, 3, 7, 17, 0, 2, who, false, 3});
  stage_case(StageCase{17, 3, 7, 17, 0, 2, 0, true, 3});
  for (int carry : {0, 1})
    for (int clips : {2, 1}) {
      for (char who : {'D', 'S', 'U', 'L'}) stage_case(StageCase{17, 3, 7, 17, carry, clips, who});
      stage_case(StageCase{17, 3, 7, 17, carry, clips, 0, true});
    }
}

// ---- the transform staging (host_stage.h: transform_walk) ------------------------------------------------------------------------
// The device is the two heap buffers pqa_side.hip reserves for a transform (source chunk / result chunk; in place: source
// chunk / second input), the pinned chunks two more.  The "kernel" copies: destination plane p is source plane p % src_planes
// (so one packed plane fans out to three, as pqa_unpack's does); in place it leaves the source where it lies and checks that
// the second input beside it belongs to the same frame.
struct TransformCase {
  int n_frames, src_planes, dst_planes, dst_step;
  size_t row_bytes;
  int h;
  int64_t stride_extra;
  bool aux;            // a second input a frame; the result stays where the source was uploaded
  char fail_in = 0;    // 'U', 'L' or 'F': that callable returns 7 in the second chunk
};

static void transform_case(const TransformCase& k) {
  const int chunk = 8, slots = k.n_frames < chunk ? k.n_frames : chunk, sp = k.src_planes, dp = k.dst_planes;
  const size_t srb[3] = {k.row_bytes, k.row_bytes + 5, k.row_bytes + 10};
  const size_t drb[3] = {srb[0], srb[1 % sp], srb[2 % sp]};
  const int rows[3] = {k.h, k.h, k.h};
  const ClipLayout S = sp == 1 ? plane_clip(srb[0], k.h) : clip_layout(sp, srb, rows, 16, 256);
  const ClipLayout D = k.aux ? S : dp == 1 ? plane_clip(drb[0], k.h) : clip_layout(dp, drb, rows, 16, 16);   // in place: one layout
  int64_t ss[3] = {0, 0, 0}, ds[3] = {0, 0, 0};
  for (int p = 0; p < sp; ++p) ss[p] = S.plane[p].pitch + k.stride_extra;
  for (int p = 0; p < dp; ++p) ds[p] = (int64_t)drb[p] + k.stride_extra;
  // sources (clip 1: the second input) end at their last sample; destinations carry sentinels between the rows and behind the last
  std::vector<std::unique_ptr<uint8_t[]>> src[2], dst;
  std::vector<const void*> list[2];
  std::vector<void*> out((size_t)k.n_frames * k.dst_step, nullptr);
  const auto dst_bytes = [&](int p) { return (size_t)ds[p] * k.h + 8; };
  for (int f = 0; f < k.n_frames; ++f) {
    for (int c = 0; c < (k.aux ? 2 : 1); ++c)
      for (int p = 0; p < sp; ++p) {
        src[c].emplace_back(new uint8_t[(size_t)ss[p] * (k.h - 1) + srb[p]]);
        for (int y = 0; y < k.h; ++y)
          for (size_t x = 0; x < (size_t)(y < k.h - 1 ? ss[p] : (int64_t)srb[p]); ++x)
            src[c].back()[(size_t)y * ss[p] + x] = x < srb[p] ? sample_of(c, f, y, x + 5 * p) : 0xee;
        list[c].push_back(src[c].back().get());
      }
    for (int p = 0; p < dp; ++p) {
      dst.emplace_back(new uint8_t[dst_bytes(p)]);
      memset(dst.back().get(), 0xEE, dst_bytes(p));
      out[(size_t)f * k.dst_step + p] = dst.back().get();
    }
  }
  const size_t sb = S.frame_bytes * slots, db = D.frame_bytes * slots;
  std::unique_ptr<uint8_t[]> pin0(new uint8_t[sb * (k.aux ? 2 : 1)]), pin1(new uint8_t[db]), a(new uint8_t[sb]), b(new uint8_t[k.aux ? sb : db]);
  uint8_t* const pins[2] = {pin0.get(), pin1.get()};
  std::string log;
  int chunk_no = -1, uploaded = 0;
  const auto fails = [&](char who) { log += who; return k.fail_in == who && chunk_no == 1 ? 7 : 0; };
  const int rc = transform_walk(
      S, D, pins, list[0].data(), ss, k.aux ? list[1].data() : nullptr, ss, out.data(), ds, k.dst_step, k.n_frames, chunk,
      [&](int f0, int n) {
        ++chunk_no;
        CHECK(f0 == chunk_no * chunk && n >= 1 && n <= slots && f0 + n <= k.n_frames);
        memcpy(a.get(), pins[0], S.frame_bytes * n);
        if (k.aux) memcpy(b.get(), pins[0] + sb, S.frame_bytes * n);
        uploaded = n;
        return fails('U');
      },
      [&](int n) {
        CHECK(n == uploaded);
        for (int f = 0; f < n; ++f)
          for (int p = 0; p < dp; ++p)
            for (int y = 0; y < k.h; ++y) {
              const uint8_t* from = a.get() + (size_t)f * S.frame_bytes + S.off[p % sp] + (size_t)y * S.plane[p % sp].pitch;
              if (k.aux)   // the second input of the same frame lies beside the source
                CHECK(!memcmp(b.get() + (from - a.get()), src[1][(size_t)(chunk_no * chunk + f) * sp + p].get() + (size_t)y * ss[p], srb[p]));
              else
                memcpy(b.get() + (size_t)f * D.frame_bytes + D.off[p] + (size_t)y * D.plane[p].pitch, from, drb[p]);
            }
        return fails('L');
      },
      [&](int e, int n) {
        CHECK(n == uploaded);
        memcpy(pins[1], k.aux ? a.get() : b.get(), D.frame_bytes * n);
        const int own = fails('F');
        return e ? e : own;
      });
  // the calls, restated: per chunk upload, launch (not after a failed upload), finish (always)
  std::string want;
  const int n_chunks = (k.n_frames + chunk - 1) / chunk;
  int done = k.n_frames;   // frames of the chunks that came through
  for (int i = 0; i < n_chunks; ++i) {
    const bool hit = i == 1 && k.fail_in;
    want += hit && k.fail_in == 'U' ? "UF" : "ULF";
    if (hit) { done = chunk; break; }
  }
  CHECK(log == want);
  CHECK(rc == (k.fail_in ? 7 : 0));
  // every destination frame of a chunk that came through holds its own source frame, the others nothing; every sentinel survives
  for (int f = 0; f < k.n_frames; ++f)
    for (int p = 0; p < dp; ++p) {
      const uint8_t* o = (const uint8_t*)out[(size_t)f * k.dst_step + p];
      for (size_t i = 0; i < dst_bytes(p); ++i) {
        const int y = (int)(i / (size_t)ds[p]);
        const size_t x = i % (size_t)ds[p];
        const bool sample = f < done && y < k.h && x < drb[p];
        CHECK(o[i] == (sample ? sample_of(0, f, y, x + 5 * (p % sp)) : 0xEE));
      }
    }
}

static void transform_scenarios() {
  const int shapes[][3] = {{1, 1, 1}, {1, 1, 3}, {1, 3, 3}, {3, 3, 3}};   // source planes, destination planes, destination pointer step
  for (const auto& sh : shapes)
    for (size_t row_bytes : {1, 15, 16, 17, 33})
      for (int h : {1, 3})
        for (int64_t extra : {0, 7})
          for (int n : {0, 1, 8, 9, 17})
            for (bool aux : {false, true})
              if (!aux || sh[0] == sh[1]) transform_case(TransformCase{n, sh[0], sh[1], sh[2], row_bytes, h, extra, aux});
  for (const auto& sh : shapes)
    for (char who : {'U', 'L', 'F'}) {
      transform_case(TransformCase{17, sh[0], sh[1], sh[2], 17, 3, 7, false, who});
      if (sh[0] == sh[1]) transform_case(TransformCase{17, sh[0], sh[1], sh[2], 17, 3, 7, true, who});
    }
}

// ---- the frame histories (host_chain.h) ------------------------------------------------------------------------------------
// A history plane is modelled by the frame number last copied into it.  Planes the caller arms hold a token until the next
// batch says which frames they are.
constexpr int64_t kNoFrame = -1000, kArmToken = -100;   // nothing read / never written; armed plane j holds kArmToken - j

// A chain as pqa_api.hip drives it: begin and the lookups of a step, end and its keep copies.
struct ChainSim {
  FrameChain ch;
  bool takes_prev;
  int64_t plane[2] = {kNoFrame, kNoFrame};
  int64_t read[2] = {kNoFrame, kNoFrame};   // what the last batch read as frames first-1, first-2
  FrameChain::Copy cp[FrameChain::kMaxDepth];
  int n_cp = 0;
  ChainSim(int depth, bool prev) : ch(depth), takes_prev(prev) {}
  void arm(int n) {
    for (int j = 0; j < n; ++j) plane[j] = kArmToken - j;
    ch.arm(n);
  }
  void batch(int64_t first, int n, bool prev) {
    ch.begin(first);
    for (int j = 0; j < 2; ++j) {
      const int slot = ch.find(first - 1 - j);
      read[j] = j == 0 && prev && takes_prev ? first - 1 : slot >= 0 ? plane[slot] : kNoFrame;
    }
    n_cp = ch.end(first, n, prev && takes_prev, cp);
    for (int i = 0; i < n_cp; ++i) {
      CHECK(cp[i].slot >= 0 && cp[i].slot < 2 && (cp[i].src == FrameChain::kFromPrev ? prev : cp[i].src >= 0 && cp[i].src < n));
      plane[cp[i].slot] = cp[i].src == FrameChain::kFromPrev ? first - 1 : first + cp[i].src;
    }
  }
  bool copies(std::initializer_list<std::pair<int, int>> want) const {
    int i = 0;
    for (const auto& w : want)
      if (i >= n_cp || cp[i].slot != w.first || cp[i++].src != w.second) return false;
    return i == n_cp;
  }
};

// The four state machines as pqa_api.hip spelled them before FrameChain, variable by variable: motion, xpsnr, siti (z = 0 the
// distorted clip, which takes no caller's plane; z = 1 the reference), integrity.
struct OldChains {
  int64_t last_luma = kNoFrame, last_index = -1;
  bool have_last = false, halo_armed = false;
  int64_t xp_hist[2] = {kNoFrame, kNoFrame}, xp_hist_idx[2] = {-1, -1}, xp_last = -1;
  int xp_armed = -1;
  int64_t st_hist[2] = {kNoFrame, kNoFrame}, st_hist_idx[2] = {-1, -1};
  bool st_armed[2] = {false, false};
  int64_t ig_hist = kNoFrame, ig_hist_idx = -1;
  bool ig_armed = false;
  int64_t read[5][2];   // per feature (motion, xpsnr, siti z = 0, siti z = 1, integrity): frames first-1, first-2 as read

  void restart() {   // pqa_reset; the n_prev == 0 / NULL branches of the setters clear the same variables, feature by feature
    have_last = halo_armed = false; last_index = -1;
    xp_armed = -1; xp_last = -1; xp_hist_idx[0] = xp_hist_idx[1] = -1;
    st_armed[0] = st_armed[1] = false; st_hist_idx[0] = st_hist_idx[1] = -1;
    ig_armed = false; ig_hist_idx = -1;
  }
  void arm(int n_prev) {   // set_history, pqa_set_dis_history and pqa_set_dis_history_planes in one
    last_luma = kArmToken; halo_armed = true;
    for (int j = 0; j < n_prev; ++j) xp_hist[j] = kArmToken - j;
    xp_armed = n_prev;
    for (int z = 0; z < 2; ++z) { st_hist[z] = kArmToken; st_armed[z] = true; }
    ig_hist = kArmToken; ig_armed = true;
  }
  void batch(int64_t first, int n, bool prev) {
    for (auto& r : read) r[0] = r[1] = kNoFrame;
    // motion
    if (prev) read[0][0] = first - 1;
    else if (halo_armed || (have_last && last_index == first - 1)) read[0][0] = last_luma;
    // xpsnr
    if (xp_armed >= 0) {
      xp_hist_idx[0] = xp_armed >= 1 ? first - 1 : -1;
      xp_hist_idx[1] = xp_armed >= 2 ? first - 2 : -1;
      xp_armed = -1;
    } else if (xp_last != first - 1) {
      xp_hist_idx[0] = xp_hist_idx[1] = -1;
    }
    const auto held = [&](int64_t idx) { return idx < 0 ? -1 : xp_hist_idx[0] == idx ? 0 : xp_hist_idx[1] == idx ? 1 : -1; };
    const int xp_h1 = held(first - 1), j2 = held(first - 2);
    if (prev) read[1][0] = first - 1;
    else if (xp_h1 >= 0) read[1][0] = xp_hist[xp_h1];
    if (j2 >= 0) read[1][1] = xp_hist[j2];
    // siti
    for (int z = 0; z < 2; ++z) {
      if (st_armed[z]) { st_hist_idx[z] = first - 1; st_armed[z] = false; }
      if (st_hist_idx[z] >= 0 && st_hist_idx[z] == first - 1) read[2 + z][0] = st_hist[z];
    }
    if (prev) read[3][0] = first - 1;
    // integrity
    if (ig_armed) { ig_hist_idx = first - 1; ig_armed = false; }
    if (ig_hist_idx >= 0 && ig_hist_idx == first - 1) read[4][0] = ig_hist;
    // the keep copies at the end of the batch
    last_luma = first + n - 1; have_last = true; halo_armed = false; last_index = first + n - 1;
    const auto keep = [&](int slot, int64_t frame) { xp_hist_idx[slot] = frame; xp_hist[slot] = frame; };
    if (n >= 2) {
      keep(0, first + n - 2);
      keep(1, first + n - 1);
    } else if (n == 1) {
      int older = xp_h1;
      if (older < 0 && prev) { older = 0; keep(0, first - 1); }
      const int slot = older == 0 ? 1 : 0;
      if (older < 0) xp_hist_idx[1] = -1;
      keep(slot, first);
    }
    xp_last = first + n - 1;
    for (int z = 0; z < 2; ++z) st_hist[z] = st_hist_idx[z] = first + n - 1;
    ig_hist = ig_hist_idx = first + n - 1;
  }
};

static void chain_scenarios() {
  {   // a shard that starts at frame 5 with two armed planes, in batches of two (tests/test_gpu_xpsnr.py); then with one
    ChainSim x(2, true);
    x.arm(2);
    x.batch(5, 2, false);
    CHECK(x.read[0] == kArmToken && x.read[1] == kArmToken - 1 && x.copies({{0, 0}, {1, 1}}));
    x.batch(7, 2, false);
    CHECK(x.read[0] == 6 && x.read[1] == 5);
    x.ch.restart();
    x.arm(1);
    x.batch(5, 2, false);
    CHECK(x.read[0] == kArmToken && x.read[1] == kNoFrame);
  }
  for (int depth : {1, 2}) {   // arm, then restart (NULL / n_prev = 0): a chain start; a reset in the middle of a chain likewise
    ChainSim x(depth, false);
    x.arm(1);
    x.ch.restart();
    x.batch(5, 1, false);
    CHECK(x.read[0] == kNoFrame && x.read[1] == kNoFrame);
    x.batch(6, 3, false);
    CHECK(x.read[0] == 5 && x.read[1] == kNoFrame);
    x.ch.restart();
    x.batch(9, 2, false);
    CHECK(x.read[0] == kNoFrame && x.read[1] == kNoFrame);
  }
  {   // one-frame batches, the first with a caller's plane: it goes to slot 0, the frame to slot 1, then the slots alternate
    ChainSim x(2, true);
    x.batch(3, 1, true);
    CHECK(x.read[0] == 2 && x.read[1] == kNoFrame && x.copies({{0, FrameChain::kFromPrev}, {1, 0}}));
    x.batch(4, 1, false);
    CHECK(x.read[0] == 3 && x.read[1] == 2 && x.copies({{0, 0}}));
    x.batch(5, 1, true);   // the kept frame 4 stays where it is although the caller gave it again
    CHECK(x.read[0] == 4 && x.read[1] == 3 && x.copies({{1, 0}}));
    // without one: the older slot is left empty
    ChainSim y(2, true);
    y.batch(3, 1, false);
    CHECK(y.read[0] == kNoFrame && y.read[1] == kNoFrame && y.copies({{0, 0}}) && y.ch.find(3) == 0 && y.ch.find(2) == -1);
    y.batch(4, 1, false);
    CHECK(y.read[0] == 3 && y.read[1] == kNoFrame && y.copies({{1, 0}}));
    // a chain that takes no caller's plane (siti's distorted clip, integrity) does not see it
    ChainSim z(1, false);
    z.batch(3, 1, true);
    CHECK(z.read[0] == kNoFrame && z.copies({{0, 0}}));
  }
  for (int depth : {1, 2}) {   // frames 0..2, then 7..8 with no reset and nothing armed: a chain start; 9 continues it
    ChainSim x(depth, true);
    x.batch(0, 2, false);
    CHECK(x.read[0] == kNoFrame && x.read[1] == kNoFrame && x.ch.find(-1) == -1);
    x.batch(2, 1, false);
    CHECK(x.read[0] == 1 && x.read[1] == (depth == 2 ? 0 : kNoFrame));
    x.batch(7, 2, false);
    CHECK(x.read[0] == kNoFrame && x.read[1] == kNoFrame);
    x.batch(9, 1, false);
    CHECK(x.read[0] == 8 && x.read[1] == (depth == 2 ? 7 : kNoFrame));
  }
  // a random walk over arm / restart / batch: the five chains of a context beside the parent's variables.  After every batch
  // both read the same planes as frames first-1 and first-2, and those are the right frames or none.  (A plane armed in front
  // of frame 0 would be frame -1, which no chain holds; the walk does not arm there.)
  for (unsigned seed : {1u, 2u, 3u}) {
    std::mt19937 rng(seed);
    ChainSim sims[5] = {{1, true}, {2, true}, {1, false}, {1, true}, {1, false}};
    OldChains old;
    int armed = -1;              // planes armed since the last batch or restart (-1: none)
    int64_t last = -1;           // last frame of the previous batch (-1: a chain start)
    bool have2[5] = {};          // frame last-1 is there for the next batch (depth 2)
    for (int step = 0; step < 4000; ++step) {
      const unsigned what = rng() % 8;
      if (what == 0) {
        const int n = 1 + (int)(rng() % 2);
        for (auto& s : sims) s.arm(n);
        old.arm(n);
        armed = n;
      } else if (what == 1) {
        for (auto& s : sims) s.ch.restart();
        old.restart();
        armed = -1; last = -1;
      } else {
        const bool jump = last < 0 || rng() % 4 == 0;
        int64_t first = jump ? (int64_t)(rng() % 40) : last + 1;
        if (armed >= 0 && first < 2) first = 2;
        const int n = 1 + (int)(rng() % 4);
        const bool prev = first >= 1 && rng() % 3 == 0;
        const bool continues = armed < 0 && last >= 0 && last == first - 1;
        // the armed planes are frames first-1, first-2 of this batch
        const auto label = [&](int64_t& p) { if (armed >= 0 && p <= kArmToken && p > kArmToken - armed) p = first - 1 - (kArmToken - p); };
        for (auto& s : sims) { label(s.plane[0]); label(s.plane[1]); }
        label(old.last_luma); label(old.xp_hist[0]); label(old.xp_hist[1]); label(old.st_hist[0]); label(old.st_hist[1]); label(old.ig_hist);
        old.batch(first, n, prev);
        for (int i = 0; i < 5; ++i) {
          ChainSim& s = sims[i];
          s.batch(first, n, prev);
          const bool two = i == 1;
          const int64_t want1 = (prev && s.takes_prev) || armed >= 1 || continues ? first - 1 : kNoFrame;
          const int64_t want2 = two && (armed >= 2 || (continues && have2[i])) ? first - 2 : kNoFrame;
          CHECK(s.read[0] == want1 && s.read[1] == want2);
          CHECK(old.read[i][0] == want1 && old.read[i][1] == want2);
          have2[i] = n >= 2 || want1 != kNoFrame;
        }
        armed = -1;
        last = first + n - 1;
      }
    }
  }
}

// proof that the sanitizer under which this binary was built is alive: a real data race / a real heap overflow, on request
static int g_plain = 0;
static void selftest(const char* what) {
  if (!strcmp(what, "race")) {
    std::thread a([] { for (int i = 0; i < 100000; ++i) g_plain = g_plain + 1; });
    std::thread b([] { for (int i = 0; i < 100000; ++i) g_plain = g_plain + 1; });
    a.join(); b.join();
  } else {
    std::vector<uint8_t> v(16);
    volatile uint8_t* p = v.data();
    p[16 + (g_plain & 1)] = 1;
  }
  printf("selftest %s done (%d)\n", what, g_plain);
}

int main(int argc, char** argv) {
  if (argc > 2 && !strcmp(argv[1], "--selftest")) { selftest(argv[2]); return 0; }
  const char* dir = argc > 1 ? argv[1] : "/tmp";
  ring_scenarios();
  chain_scenarios();
  stage_scenarios();
  transform_scenarios();
  pack_scenarios(dir);
  packed_clip_scenarios();
  launch_size_properties();
  printf("host harness ok\n");
  return 0;
}
