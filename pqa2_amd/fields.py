"""Field alignment on the host: from the field-against-field squared errors of a clip pair (FeatureEngine.field_moments,
pqa_field_moments) to the field structure of the capture and the plan that undoes it.

    X[k-1][0..13], k = 1 ... n - 1, E(A, p, B, q) = sum over the row pairs of (A[2 i + p] - B[2 i + q])^2:
      2 p + q      E(D_k, p, R_k, q)          4 + 2 p + q   E(D_k, p, R_{k-1}, q)       8 + 2 p + q   E(D_{k-1}, p, R_k, q)
      12           E(D_k, 0, D_k, 1)          13            E(R_k, 0, R_k, 1)

A progressive programme carried over an interlaced link comes back with the rows of one parity taken from the neighbouring frame
(field shift), with both fields in the wrong line positions (field swap) or with one field dropped and the other line-doubled
(single field).  A STATE (q0, j0, q1, j1) says that the captured rows of parity p show the reference rows of parity q_p of
frame t + j_p; the first two faults are states with q0 != q1 and are exactly reversible by moving rows (weave_plan).

Everything that decides is Python-int / Fraction arithmetic on exact integers, so a result does not depend on the machine, the
rank or the run; floats appear in the report only."""
from __future__ import annotations

from fractions import Fraction

import numpy as np

from .align import default_penalty

OFFSETS = (-1, 0, 1)
IDENTITY = (0, 0, 1, 0)


def _states():
    every = [(q0, j0, q1, j1) for q0 in (0, 1) for j0 in OFFSETS for q1 in (0, 1) for j1 in OFFSETS]
    own = sorted((s for s in every if (s[0], s[2]) == (0, 1) and s != IDENTITY), key=lambda s: (abs(s[1]) + abs(s[3]), s))
    rest = sorted((s for s in every if (s[0], s[2]) != (0, 1)), key=lambda s: (abs(s[1]) + abs(s[3]), s))
    return (IDENTITY,) + tuple(own) + tuple(rest)


# the 36 states: the identity, then the own-parity states by |j0| + |j1|, then the rest by |j0| + |j1|, ties lexicographic; every
# tie in the solver goes to the earlier one
STATES = _states()


def kind_of(state) -> str:
    """the name of a state, but for single_field / vertical_shift, which the combs tell apart (summary)"""
    q0, j0, q1, j1 = state
    if (q0, q1) == (0, 1):
        return "progressive" if (j0, j1) == (0, 0) else "field_shift" if j0 != j1 else "frame_offset"
    return "field_swap" if (q0, q1) == (1, 0) else "vertical_shift"


def _ints(X):
    X = np.asarray(X)
    if X.ndim != 2 or X.shape[1] != 14:
        raise ValueError("X must be [n - 1, 14]")
    return [[int(v) for v in row] for row in X]


def frame_costs(X):
    """C[t - 1][p][q][j + 1] for the captured frames t = 1 ... n - 2 that have all six candidates: the squared error of the
    captured rows of parity p of frame t against the reference rows of parity q of frame t + j (Python ints).  j = 0 is in
    record t - 1, word 2 p + q; j = -1 in record t - 1, word 4 + 2 p + q; j = +1 in record t, word 8 + 2 p + q."""
    X = _ints(X)
    return [[[[X[t - 1][4 + 2 * p + q], X[t - 1][2 * p + q], X[t][8 + 2 * p + q]] for q in (0, 1)] for p in (0, 1)]
            for t in range(1, len(X))]


def _state_cost(c, s) -> int:
    return c[0][s[0]][s[1] + 1] + c[1][s[2]][s[3] + 1]


def segments(X, n_pixels: int, bit_depth: int = 8, penalty_mse: float | None = None, min_improvement: float = 2.0):
    """[(first, last, state)]: the runs of captured frames first ... last - 1 that share a state, over the frames 1 ... n - 2.

    The cheapest path through STATES: a state costs the sum of its two candidates at every frame (frame_costs), a change of
    state costs P = align.default_penalty(n_pixels, bit_depth, penalty_mse); O(frames * states) through the running minimum
    over the previous frame.  A run whose state is not the identity is then kept only if the identity's cost over the run is
    at least `min_improvement` times its own AND exceeds it by at least 0.5 * 4^(bit_depth - 8) per pixel and frame;
    otherwise it becomes identity and merges with its neighbours.  Fewer than three frames: no run."""
    C = frame_costs(X)
    if not C:
        return []
    P = default_penalty(n_pixels, bit_depth, penalty_mse)
    S = len(STATES)
    V = [_state_cost(C[0], s) for s in STATES]
    back = []
    for c in C[1:]:
        m = min(range(S), key=lambda i: (V[i], i))     # the cheapest state to leave, the earlier of equals
        row, brow = [0] * S, [0] * S
        for i, s in enumerate(STATES):
            stay, move = V[i], V[m] + P
            brow[i] = i if (stay, i) <= (move, m) else m
            row[i] = min(stay, move) + _state_cost(c, s)
        V = row
        back.append(brow)
    i = min(range(S), key=lambda k: (V[k], k))
    path = [i]
    for brow in reversed(back):
        i = brow[i]
        path.append(i)
    path.reverse()

    bar = Fraction(1, 2) * 4 ** (int(bit_depth) - 8) * int(n_pixels)
    runs = []     # [first index into C, last, state index]
    for k, i in enumerate(path):
        if runs and runs[-1][2] == i:
            runs[-1][1] = k + 1
        else:
            runs.append([k, k + 1, i])
    for r in runs:
        if r[2] != 0:
            own = sum(_state_cost(C[k], STATES[r[2]]) for k in range(r[0], r[1]))
            idn = sum(_state_cost(C[k], IDENTITY) for k in range(r[0], r[1]))
            if not (idn >= Fraction(min_improvement) * own and idn - own >= bar * (r[1] - r[0])):
                r[2] = 0
    out = []
    for a, b, i in runs:
        if out and out[-1][2] == STATES[i]:
            out[-1] = (out[-1][0], b + 1, STATES[i])
        else:
            out.append((a + 1, b + 1, STATES[i]))
    return out


def _ratio(num: int, den: int):
    return float("inf") if den == 0 and num > 0 else None if den == 0 else num / den


def summary(X, width: int, height: int, bit_depth: int = 8, penalty_mse: float | None = None, min_improvement: float = 2.0) -> dict:
    """The report of a clip pair's field structure from X[n - 1][14] of planes of width x height.

    segments: [{first, last, state, kind}] of segments(); kind: progressive (the identity), field_shift (own parities,
    j0 != j1), frame_offset (own parities, j0 = j1 != 0), field_swap (q = (1, 0)), single_field (q0 = q1 and 8 * sum of word
    12 <= sum of word 13 over the segment: the captured frame has no comb where the reference has one) or vertical_shift
    (q0 = q1 otherwise: a picture one line off; spatial alignment is the tool).  kind / state: those of the segments that
    cover most frames (of equals, the kind met first; its longest segment's state).  flips = segments - 1.  top / bottom:
    {parity, offset, confidence} of that state per captured parity, confidence = the smallest clip total of the other five
    candidates over the chosen one's.  mse_before / mse_after: the identity's and the chosen path's cost per counted pixel and
    frame.  comb_ratio = sum of word 12 / sum of word 13.  static: for both captured parities and either reference parity the clip
    totals of the three offsets lie within `min_improvement` of each other -- nothing moves, the neighbouring frames hold the
    same picture, and "progressive" then says nothing.  (The two reference parities of one frame differ by the picture's
    vertical detail whether it moves or not, so they are not held against each other.)  weavable: every segment has
    q0 != q1."""
    rows = _ints(X)
    C = frame_costs(X)
    n_pixels = int(width) * int(height)
    counted = 2 * (int(height) // 2) * int(width)
    segs = segments(X, n_pixels, bit_depth, penalty_mse, min_improvement)
    listed, span = [], {}
    for a, b, s in segs:
        kind = kind_of(s)
        if s[0] == s[2]:
            comb_d, comb_r = (sum(rows[t - 1][w] for t in range(a, b)) for w in (12, 13))
            kind = "single_field" if 8 * comb_d <= comb_r else "vertical_shift"
        listed.append({"first": a, "last": b, "state": list(s), "kind": kind})
        span[kind] = span.get(kind, 0) + b - a
    kind = max(span, key=lambda k: span[k]) if span else "progressive"     # max keeps the first of equals
    of_kind = [g for g in listed if g["kind"] == kind]
    state = tuple(max(of_kind, key=lambda g: g["last"] - g["first"])["state"]) if of_kind else IDENTITY
    total = [[[sum(c[p][q][j] for c in C) for j in range(3)] for q in (0, 1)] for p in (0, 1)]
    chosen = {}
    for p, name in enumerate(("top", "bottom")):
        q, j = state[2 * p], state[2 * p + 1]
        best = total[p][q][j + 1]
        others = [total[p][qq][jj] for qq in (0, 1) for jj in range(3) if (qq, jj) != (q, j + 1)]
        chosen[name] = {"parity": q, "offset": j, "confidence": _ratio(min(others), best)}
    by_frame = [total[p][q] for p in (0, 1) for q in (0, 1)]     # the candidates that differ in the frame alone
    before = sum(_state_cost(c, IDENTITY) for c in C)
    after = sum(_state_cost(C[t - 1], s) for a, b, s in segs for t in range(a, b))
    comb_d, comb_r = (sum(r[w] for r in rows) for w in (12, 13))
    den = float(len(C) * counted)
    return {"kind": kind, "state": list(state), "segments": listed, "flips": max(len(listed) - 1, 0), **chosen,
            "mse_before": before / den if den else None, "mse_after": after / den if den else None,
            "comb_ratio": _ratio(comb_d, comb_r),
            "static": bool(C) and all(max(f) <= Fraction(min_improvement) * min(f) for f in by_frame),
            "weavable": all(g["state"][0] != g["state"][2] for g in listed)}


def weave_plan(segs, n: int) -> dict:
    """Where every field of the re-woven clip comes from: {u_lo, u_hi, sources, unfilled}.

    The state of the segment that holds captured frame t says that its rows of parity p show the reference rows of parity q_p
    of frame t + j_p; the first segment also holds the frames before it and the last one the frames behind it.  For the output
    frames u = u_lo ... u_hi - 1, sources[u - u_lo][r] = (t, p): rows r, r + 2, ... of output frame u are rows p, p + 2, ... of
    captured frame t, where t + j_p = u and q_p = r; of two providers the earlier frame wins.  A field with no provider (the
    field lost at a flip) is left as captured frame u has it, (u, r), and listed in `unfilled`.  [u_lo, u_hi) is the range for
    which the unflipped ends have sources: u_lo = max(0, j0, j1) of the first state, u_hi = n + min(0, j0, j1) of the last."""
    n = int(n)
    segs = [(int(a), int(b), tuple(s)) for a, b, s in segs] or [(0, n, IDENTITY)]
    state_at = []
    for t in range(n):
        held = [s for a, b, s in segs if a <= t < b]
        state_at.append(held[0] if held else segs[0][2] if t < segs[0][0] else segs[-1][2])
    first, last = segs[0][2], segs[-1][2]
    u_lo, u_hi = max(0, first[1], first[3]), n + min(0, last[1], last[3])
    sources, unfilled = [], []
    for u in range(u_lo, max(u_hi, u_lo)):
        pair = []
        for r in (0, 1):
            src = None
            for t in (u - 1, u, u + 1):     # t + j = u, the earlier frame first
                if 0 <= t < n and src is None:
                    s = state_at[t]
                    for p in (0, 1):
                        if src is None and s[2 * p] == r and t + s[2 * p + 1] == u:
                            src = (t, p)
            if src is None:
                src = (u, r)
                unfilled.append((u, r))
            pair.append(src)
        sources.append(tuple(pair))
    return {"u_lo": u_lo, "u_hi": max(u_hi, u_lo), "sources": sources, "unfilled": unfilled}
