// Which coefficients of the ADM pyramid anything downstream can consume: the dependency cone of libvmaf's 10 % windows.
//
// libvmaf accumulates every ADM scale over its own window [left, right) x [top, bottom) (adm_window in
// oracle/vmaf_oracle.c: 10 % cropped on each side, per scale).  Outside it a march kernel owes only the approximation band
// -- and only where the NEXT scale reads it, which is cropped by the same rule.  By induction from the last scale (which
// owes no band) the coefficient positions at which anything must be computed are, per scale s and per axis:
//   scale 3     : the window dilated by the 3 x 3 masking box                               [top - 1, bottom + 1)
//   scale s < 3 : the hull of that and of what the needed range [a, b) of scale s + 1 reads through the DWT: coefficient
//                 j reads positions 2j - 1 .. 2j + 2 of the band above (adm_pyramid.hip "Scale-1 row j needs scale-0 rows
//                 2j - 1 .. 2j + 2"; adm_march.hip "rows 2i - 1, 2i (carried) and 2i + 1, 2i + 2 (new)")  [2a - 1, 2b + 1)
// clamped to the band.  The clamp is the mirror: position -1 folds to 1 and positions n, n + 1 fold to n - 1, n - 2, all
// inside a hull that reaches the edge they fold at.  The input samples needed are what scale 0's range reads.  For small
// frames (about 256 and below per axis) the cone is the whole band.
// Plain C++, no device code: the launchers, pqa_debug_adm_need and stand-alone host programs include it.
#pragma once

namespace pqa {

struct AdmSpan {
  int lo, hi;   // half-open
};
struct AdmNeed {
  AdmSpan rows[4], cols[4];     // per ADM scale: coefficient positions at which anything must be computed
  AdmSpan in_rows, in_cols;     // input samples read for them
};

// One axis of a pyramid of n_scales (1 .. 4) scales over n input samples, the last of which owes no band: need[0 ..
// n_scales).  cone = false: every position of every band (the whole-band partner of the cone).
inline void adm_need_axis(int n, int n_scales, bool cone, AdmSpan* need, AdmSpan* input) {
  int len[4];
  for (int s = 0, m = n; s < n_scales; ++s) { m = (m + 1) / 2; len[s] = m; }
  AdmSpan above{0, 0};   // needed range of scale s + 1
  for (int s = n_scales - 1; s >= 0; --s) {
    const int lo_win = (int)(len[s] * 0.1 - 0.5);              // ADM_BORDER_FACTOR window
    AdmSpan r{lo_win - 1, len[s] - lo_win + 1};                // dilated by the masking box
    if (s < n_scales - 1) {
      const int a = 2 * above.lo - 1, b = 2 * above.hi + 1;    // read through the four-tap DWT
      r.lo = a < r.lo ? a : r.lo;
      r.hi = b > r.hi ? b : r.hi;
    }
    if (!cone) r = AdmSpan{0, len[s]};
    r.lo = r.lo < 0 ? 0 : r.lo;
    r.hi = r.hi > len[s] ? len[s] : r.hi;
    need[s] = above = r;
  }
  AdmSpan in{2 * above.lo - 1, 2 * above.hi + 1};
  in.lo = in.lo < 0 ? 0 : in.lo;
  in.hi = in.hi > n ? n : in.hi;
  *input = in;
}

inline AdmNeed adm_need(int w, int h, bool cone = true) {
  AdmNeed o{};
  adm_need_axis(h, 4, cone, o.rows, &o.in_rows);
  adm_need_axis(w, 4, cone, o.cols, &o.in_cols);
  return o;
}

// The same for one launch of ADM scale `scale` (0 .. 3) on its own input of w x h samples (the frame at scale 0, the band
// of scale - 1 otherwise): the pyramid below it is all that decides its range.
inline void adm_need_scale(int scale, int w, int h, bool cone, AdmSpan* rows, AdmSpan* cols) {
  AdmSpan need[4], in;
  adm_need_axis(h, 4 - scale, cone, need, &in);
  *rows = need[0];
  adm_need_axis(w, 4 - scale, cone, need, &in);
  *cols = need[0];
}

}  // namespace pqa
