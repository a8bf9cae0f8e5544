"""numpy restatement of the pixel-format conversion (include/pqa_vmaf.h, pqa_format_convert; kernel: csrc/format_convert.hip).
Integer arithmetic only.  A layout is (hshift, vshift, hsite, vsite, bits), as FeatureEngine.format_convert takes it.

Per axis, positions in HALF luma samples, F = 1 << shift: sample k sits at P(k) = 2 F k + (centre ? F - 1 : 0);
W = max(F_src, F_dst); destination sample i takes source sample j with w = 2 W - |P_src(j) - P_dst(i)| where positive,
j folded onto clamp(j, 0, n_src - 1).  The weights sum to S = 2 W^2 / F_src.  One rounding for both axes and the depth."""
import numpy as np

COSITED, CENTRE = 0, 1


def plane_size(luma: int, shift: int) -> int:
    return -(-luma >> shift)


def position(k: int, shift: int, site: int) -> int:
    f = 1 << shift
    return 2 * f * k + (f - 1 if site == CENTRE else 0)


def weight_sum(src_shift: int, dst_shift: int) -> int:
    w = max(1 << src_shift, 1 << dst_shift)
    return 2 * w * w >> src_shift


def taps(luma: int, src_shift: int, dst_shift: int, src_site: int, dst_site: int):
    """one axis: per destination sample the list of (source index BEFORE the clamp, weight), by trying every
    candidate of a generous range around the triangle -- no closed form for the first tap, so that the kernel's is tested
    against something else"""
    n_src, n_dst = plane_size(luma, src_shift), plane_size(luma, dst_shift)
    w = max(1 << src_shift, 1 << dst_shift)
    out = []
    for i in range(n_dst):
        pd = position(i, dst_shift, dst_site)
        row = []
        lo = (pd - 2 * w) // (2 << src_shift) - 2   # generous: two candidates before the triangle's foot, four behind it
        for j in range(lo, lo + (2 * w >> src_shift) + 6):
            wt = 2 * w - abs(position(j, src_shift, src_site) - pd)
            if wt > 0:
                row.append((j, wt))
        out.append(row)
    return out


def axis_matrix(luma: int, src_shift: int, dst_shift: int, src_site: int, dst_site: int) -> np.ndarray:
    """[n_dst, n_src] int64: the taps with the edge replication folded in"""
    n_src, n_dst = plane_size(luma, src_shift), plane_size(luma, dst_shift)
    m = np.zeros((n_dst, n_src), np.int64)
    for i, row in enumerate(taps(luma, src_shift, dst_shift, src_site, dst_site)):
        for j, wt in row:
            m[i, min(max(j, 0), n_src - 1)] += wt
    return m


def convert(plane: np.ndarray, luma_shape, src, dst) -> np.ndarray:
    """`plane` (2-D, of the layout src in a frame of luma_shape = (height, width)) in the layout dst"""
    shs, svs, shsite, svsite, sbits = (int(v) for v in src)
    dhs, dvs, dhsite, dvsite, dbits = (int(v) for v in dst)
    lh, lw = int(luma_shape[0]), int(luma_shape[1])
    assert plane.shape == (plane_size(lh, svs), plane_size(lw, shs)), plane.shape
    s = np.minimum(plane.astype(np.int64), (1 << sbits) - 1)
    mx, my = axis_matrix(lw, shs, dhs, shsite, dhsite), axis_matrix(lh, svs, dvs, svsite, dvsite)
    acc = my @ s @ mx.T
    t = (weight_sum(shs, dhs) * weight_sum(svs, dvs)).bit_length() - 1
    d = dbits - sbits
    if t > d:
        out = np.minimum((acc + (1 << (t - d - 1))) >> (t - d), (1 << dbits) - 1)
    else:
        out = acc << (d - t)
    return out.astype(np.uint8 if dbits <= 8 else np.uint16)


def convert_frame(planes, info_src_layout, info_dst_layout, luma_shape):
    """[Y, U, V] of a frame: the luma with the depth change only, the chroma planes with the layouts given"""
    luma_src = (0, 0, 0, 0, info_src_layout[4])
    luma_dst = (0, 0, 0, 0, info_dst_layout[4])
    return [convert(planes[0], luma_shape, luma_src, luma_dst)] + [convert(p, luma_shape, info_src_layout, info_dst_layout)
                                                                   for p in planes[1:3]]
