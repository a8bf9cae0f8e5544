"""Numpy restatement of the overlay mask (pqa_mask_blend, csrc/mask_blend.hip) and of the two grid builders
(distortion.overlay_mask, overlay_mask_from_boxes), written from the formulas in include/pqa_vmaf.h and the builders' contract,
not from the library's code.  Everything is int64; nothing here is fast."""
import numpy as np


def grid_shape(width: int, height: int, sx: int, sy: int):
    """(rows, columns) of the node grid of a width x height plane"""
    return ((height + (1 << sy) - 1) >> sy) + 1, ((width + (1 << sx) - 1) >> sx) + 1


def alpha(nodes, width: int, height: int, sx: int, sy: int) -> np.ndarray:
    """int64 [height, width]: the four-node formula, term by term"""
    A = np.asarray(nodes, np.int64)
    assert A.shape == grid_shape(width, height, sx, sy)
    Gx, Gy = 1 << sx, 1 << sy
    y, x = np.mgrid[0:height, 0:width].astype(np.int64)
    i, fx, j, fy = x >> sx, x & (Gx - 1), y >> sy, y & (Gy - 1)
    num = (A[j, i] * (Gx - fx) * (Gy - fy) + A[j, i + 1] * fx * (Gy - fy) + A[j + 1, i] * (Gx - fx) * fy + A[j + 1, i + 1] * fx * fy
           + ((Gx * Gy) >> 1))
    assert num.max(initial=0) < 1 << 21
    return num >> (sx + sy)


def blend(src, nodes, sx: int, sy: int, fill, bit_depth: int) -> np.ndarray:
    """the blended plane, of src's dtype.  fill: an integer, or a plane of src's shape.  u16: where alpha > 0 a source sample
    above top is read as top, and so is every fill sample; where alpha = 0 the source sample is copied as it is."""
    src = np.asarray(src)
    top = (1 << bit_depth) - 1
    h, w = src.shape
    a = alpha(nodes, w, h, sx, sy)
    s = np.minimum(src.astype(np.int64), top)
    f = np.minimum(np.asarray(fill).astype(np.int64), top) + np.zeros_like(s)
    out = (s * (256 - a) + f * a + 128) >> 8
    return np.where(a == 0, src.astype(np.int64), out).astype(src.dtype)


def bounds(nodes, width: int, height: int, sx: int, sy: int):
    """[x0, y0, x1, y1]: the smallest rectangle that holds every sample with alpha > 0 -- or, where a node's weight rounds to
    zero, a little more: every sample strictly between the neighbours of a non-zero node.  None: no such sample."""
    A = np.asarray(nodes)
    js, is_ = np.nonzero(A)
    if not len(js):
        return None
    x0, x1 = max(0, (int(is_.min()) - 1) * (1 << sx) + 1), min(width, (int(is_.max()) + 1) * (1 << sx))
    y0, y1 = max(0, (int(js.min()) - 1) * (1 << sy) + 1), min(height, (int(js.max()) + 1) * (1 << sy))
    return [x0, y0, x1, y1] if x0 < x1 and y0 < y1 else None


def _grown(tiles, grow: int) -> np.ndarray:
    t = np.asarray(tiles, bool)
    out = t.copy()
    for _ in range(grow):
        nxt = out.copy()
        for j, i in zip(*np.nonzero(out)):
            nxt[max(j - 1, 0):j + 2, max(i - 1, 0):i + 2] = True
        out = nxt
    return out


def _feathered(inside: np.ndarray, feather: int, node: int) -> np.ndarray:
    """nodes from the inside set: the Chebyshev distance of every node to it, by brute force"""
    K = feather // node
    gy, gx = inside.shape
    out = np.zeros((gy, gx), np.int64)
    pts = np.argwhere(inside)
    for j in range(gy):
        for i in range(gx):
            if inside[j, i]:
                out[j, i] = 256
            elif len(pts):
                s = int(np.maximum(np.abs(pts[:, 0] - j), np.abs(pts[:, 1] - i)).min())
                if 1 <= s < K:
                    out[j, i] = 256 - (256 * s) // K
    return out


def overlay_nodes(tiles, width: int, height: int, tile: int, grow: int = 1, feather: int = 16, node: int = 8) -> np.ndarray:
    """the grid of distortion.overlay_mask: a node is inside when its position lies in the closed square of a (grown) tile"""
    t = _grown(tiles, grow)
    step = node.bit_length() - 1
    gy, gx = grid_shape(width, height, step, step)
    inside = np.zeros((gy, gx), bool)
    for j in range(gy):
        for i in range(gx):
            px, py = i * node, j * node
            for tj, ti in zip(*np.nonzero(t)):
                if ti * tile <= px <= (ti + 1) * tile and tj * tile <= py <= (tj + 1) * tile:
                    inside[j, i] = True
                    break
    return _feathered(inside, feather, node)


def box_nodes(boxes, width: int, height: int, feather: int = 16, node: int = 8):
    """(grid, snapped boxes) of distortion.overlay_mask_from_boxes"""
    step = node.bit_length() - 1
    gy, gx = grid_shape(width, height, step, step)
    inside = np.zeros((gy, gx), bool)
    snapped = []
    for x0, y0, x1, y1 in boxes:
        x0, y0 = x0 - x0 % node, y0 - y0 % node
        x1, y1 = x1 + (-x1) % node, y1 + (-y1) % node
        snapped.append([x0, y0, min(x1, width), min(y1, height)])
        for j in range(gy):
            for i in range(gx):
                if x0 <= i * node <= x1 and y0 <= j * node <= y1:
                    inside[j, i] = True
    return _feathered(inside, feather, node), snapped


def random_grid(rng, width: int, height: int, sx: int, sy: int) -> np.ndarray:
    """uint16 nodes 0 ... 256 with forced runs of 0 and of 256, so that the copied, the filled and the blended items all occur"""
    gy, gx = grid_shape(width, height, sx, sy)
    A = rng.integers(0, 257, (gy, gx)).astype(np.uint16)
    for v in (0, 256):
        for _ in range(2):
            j, i = int(rng.integers(0, gy)), int(rng.integers(0, gx))
            A[j:j + max(2, gy // 3), i:i + max(3, gx // 3)] = v
    return A


LOGO_BOX = (219, 123, 283, 155)      # a 64 x 32 overlay on a 320 x 180 picture, on no tile or node boundary


def checker_logo(plane, box=LOGO_BOX, cell: int = 4, bit_depth: int = 8) -> np.ndarray:
    """a copy of a luma plane with a checkerboard of near-black and near-white cells burnt into box = (x0, y0, x1, y1)"""
    x0, y0, x1, y1 = box
    out = np.array(plane, copy=True)
    y, x = np.mgrid[y0:y1, x0:x1]
    scale = 1 << (bit_depth - 8)
    out[y0:y1, x0:x1] = np.where((((x - x0) // cell) + ((y - y0) // cell)) % 2 == 0, 235 * scale, 16 * scale).astype(out.dtype)
    return out


def tile_moments(refs, diss, tile: int) -> np.ndarray:
    """uint64 [n, ty, tx, 6]: the sums of r, d, r^2, d^2, r d and |d - r| of every tile (FeatureEngine.tile_moments)"""
    n, (h, w) = len(refs), np.shape(refs[0])
    ty, tx = -(-h // tile), -(-w // tile)
    out = np.zeros((n, ty, tx, 6), np.uint64)
    for f in range(n):
        r, d = np.asarray(refs[f], np.int64), np.asarray(diss[f], np.int64)
        for k, v in enumerate((r, d, r * r, d * d, r * d, np.abs(d - r))):
            p = np.zeros((ty * tile, tx * tile), np.int64)
            p[:h, :w] = v
            out[f, :, :, k] = p.reshape(ty, tile, tx, tile).sum(axis=(1, 3)).astype(np.uint64)
    return out
