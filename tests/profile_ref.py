"""Numpy restatement of the line profiles (pqa_line_profiles, csrc/line_profiles.hip): per row and per column of a plane the
sum of its samples and the sum of their squares, uint64; a sample above 2^bit_depth - 1 is read as that."""
import numpy as np


def line_profiles(frames, bit_depth: int = 8):
    """(rows [n, H, 2], cols [n, W, 2]) uint64 of a list of 2-D planes of one size"""
    top = (1 << bit_depth) - 1
    rows, cols = [], []
    for f in frames:
        v = np.minimum(np.asarray(f).astype(np.uint64), np.uint64(top))
        sq = v * v
        rows.append(np.stack([v.sum(axis=1, dtype=np.uint64), sq.sum(axis=1, dtype=np.uint64)], axis=1))
        cols.append(np.stack([v.sum(axis=0, dtype=np.uint64), sq.sum(axis=0, dtype=np.uint64)], axis=1))
    if not frames:
        return np.zeros((0, 0, 2), np.uint64), np.zeros((0, 0, 2), np.uint64)
    return np.stack(rows), np.stack(cols)


def random_frames(seed: int, n: int, w: int, h: int, bpc: int = 8):
    """n planes of w x h uniform noise over the whole code range"""
    rng = np.random.default_rng(seed)
    dt = np.uint8 if bpc == 8 else np.uint16
    return [rng.integers(0, 1 << bpc, (h, w)).astype(dt) for _ in range(n)]


def cols_of(frames, bit_depth: int = 8):
    """the callable align.active_picture asks for the columns of the active rows with: a second pass over row-sliced views"""
    h = frames[0].shape[0]
    return lambda top, bottom: line_profiles([f[top:h - bottom] for f in frames], bit_depth)[1]
