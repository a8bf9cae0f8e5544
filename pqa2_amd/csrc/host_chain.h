// Host-side bookkeeping of the frames a feature keeps in front of the next batch, free of any device call (see host_pack.h for
// why it is a header of its own).  Motion, XPSNR, SI / TI and the integrity SAD all read frame first-1 (XPSNR: first-2 too) of
// a batch, and all follow one policy: planes the caller armed are frames first-1, first-2 of whichever batch comes next; a
// plane kept from the last batch counts only if this batch continues the chain; where the feature takes it, a caller's `prev`
// plane wins over both (that choice, the planes and their pitches stay with the context: pqa_ctx.h).
#pragma once
#include <cstdint>

namespace pqa {
namespace host {

class FrameChain {
 public:
  static constexpr int kMaxDepth = 2;
  static constexpr int kFromPrev = -1;   // Copy::src: the caller's `prev` plane, not a frame of the batch
  struct Copy { int slot, src; };        // a keep copy to enqueue: frame `src` of the batch (0 .. n-1) into plane `slot`

  explicit FrameChain(int depth = 1) : depth_(depth) {}

  // Everything empty, nothing armed: a chain start.
  void restart() {
    idx_[0] = idx_[1] = last_ = -1;
    armed_ = -1;
  }
  // The caller's planes were copied into slots 0 .. n-1: frames first-1 .. first-n of the next batch, whatever was kept.
  void arm(int n) { armed_ = n < depth_ ? n : depth_; }
  // Before a batch reads its predecessors: bind what was armed; else a batch that does not continue the chain starts one.
  void begin(int64_t first) {
    if (armed_ >= 0) {
      for (int j = 0; j < kMaxDepth; ++j) idx_[j] = j < armed_ ? first - 1 - j : -1;
      armed_ = -1;
    } else if (last_ != first - 1) {
      idx_[0] = idx_[1] = -1;
    }
  }
  // The slot that holds `frame`, or -1 (-1 marks an empty slot: frames before 0 are never held).
  int find(int64_t frame) const {
    if (frame < 0) return -1;
    for (int j = 0; j < depth_; ++j)
      if (idx_[j] == frame) return j;
    return -1;
  }
  // After the batch of frames first .. first+n-1 (n >= 1): the copies that leave the last `depth` frames available in the
  // slots, at most `depth` of them; returns their number.  A one-frame batch of a chain of depth 2 keeps frame first-1 in the
  // slot it is in, or takes it from the caller's plane into slot 0, and puts the new frame into the other slot; an older
  // frame that is missing leaves its slot empty.
  int end(int64_t first, int n, bool caller_gave_prev, Copy out[kMaxDepth]) {
    int m = 0;
    if (n >= depth_) {
      for (int j = 0; j < depth_; ++j) {
        out[m++] = Copy{j, n - depth_ + j};
        idx_[j] = first + n - depth_ + j;
      }
    } else {
      int older = find(first - 1);
      if (older < 0 && caller_gave_prev) {
        older = 0;
        out[m++] = Copy{0, kFromPrev};
        idx_[0] = first - 1;
      }
      const int slot = older == 0 ? 1 : 0;
      if (older < 0) idx_[1] = -1;
      out[m++] = Copy{slot, 0};
      idx_[slot] = first;
    }
    last_ = first + n - 1;
    return m;
  }

 private:
  int depth_;
  int64_t idx_[kMaxDepth] = {-1, -1};   // the frame each slot holds (-1: empty)
  int64_t last_ = -1;                   // last frame of the previous batch: the chain continues at last_ + 1
  int armed_ = -1;                      // slots the caller armed for the next batch (-1: none)
};

}  // namespace host
}  // namespace pqa
