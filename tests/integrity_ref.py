"""numpy restatement of the capture-integrity feature (PQA_FEAT_INTEGRITY), written from the definitions of FFmpeg's
freezedetect, blackdetect and scdet as the project states them, not from the HIP kernel.

Device quantities (exact integers): sad_prev[p] = sum |dis_i[p] - dis_{i-1}[p]| over plane p, black_count = number of luma
samples <= the black threshold.  Host quantities: scdet's mafd / score, blackdetect's ratio and runs, freezedetect's
anchored mafd and runs -- here computed brute force from the FRAMES (every frame against its anchor frame), so that the
product's state machines, which see only rows and a callback, have an independent partner."""
import numpy as np

EXT5_DOUBLES = 8


def sad(a, b) -> int:
    return int(np.abs(np.asarray(a, np.int64) - np.asarray(b, np.int64)).sum())


def black_count(luma, threshold: int) -> int:
    return int((np.asarray(luma, np.int64) <= int(threshold)).sum())


def black_threshold(bit_depth: int, full_range: bool = False, pixel_black_th: float = 0.10) -> int:
    f = 2 ** (bit_depth - 8)
    if full_range:
        return int(np.trunc(pixel_black_th * (2 ** bit_depth - 1)))
    return int(np.trunc(16 * f + pixel_black_th * 219 * f))


def rows(frames, threshold: int, prev=None, n_planes=None) -> np.ndarray:
    """[n, 8] fifth-extension rows of a run of frames (each a list of planes): SADs in 0..2 (NaN at a chain start and for
    planes the clip does not have), the black count in 3, NaN in 4..7.  prev: the frame in front of the run, or None."""
    out = np.full((len(frames), EXT5_DOUBLES), np.nan)
    for i, fr in enumerate(frames):
        npl = n_planes or len(fr)
        before = frames[i - 1] if i > 0 else prev
        if before is not None:
            for p in range(npl):
                out[i, p] = float(sad(fr[p], before[p]))
        out[i, 3] = float(black_count(fr[0], threshold))
    return out


def frame_sad(anchor, frames, n_planes=None) -> np.ndarray:
    """[n, 3] uint64 SAD of every plane of each frame against the anchor frame (0 for planes the clip does not have)."""
    out = np.zeros((len(frames), 3), np.uint64)
    for i, fr in enumerate(frames):
        for p in range(n_planes or len(fr)):
            out[i, p] = sad(fr[p], anchor[p])
    return out


def pts(i, fps_num, fps_den):
    return i * fps_den / fps_num


def scdet(frames, bit_depth, threshold=10.0, fps=(25, 1)):
    """(mafd, score, [(frame, score)]) of the luma planes."""
    n = len(frames)
    h, w = np.shape(frames[0][0])
    mafd = np.zeros(n)
    score = np.zeros(n)
    for i in range(1, n):
        mafd[i] = 100.0 * sad(frames[i][0], frames[i - 1][0]) / (w * h) / 2 ** bit_depth
        score[i] = min(max(min(mafd[i], abs(mafd[i] - mafd[i - 1])), 0.0), 100.0)
    return mafd, score, [(i, score[i]) for i in range(n) if score[i] >= threshold]


def freezedetect(frames, bit_depth, noise=0.001, duration=2.0, fps=(25, 1)):
    """(mafd against the anchor [n], anchor index [n], [(first_frame, end_frame or None)]) brute force from the frames."""
    n = len(frames)
    total = sum(int(np.size(p)) for p in frames[0])
    mafd, anchor, events = np.zeros(n), np.zeros(n, np.int64), []
    A, open_at = 0, None
    for i in range(1, n):
        s = sum(sad(frames[i][p], frames[A][p]) for p in range(len(frames[i])))
        mafd[i], anchor[i] = s / total / 2 ** bit_depth, A
        if mafd[i] <= noise:
            if open_at is None and (i - A) * fps[1] >= duration * fps[0]:
                open_at = A
        else:
            if open_at is not None:
                events.append((open_at, i))
                open_at = None
            A = i
    if open_at is not None:
        events.append((open_at, None))
    return mafd, anchor, events


def blackdetect(frames, threshold, ratio_th=0.98, min_duration=2.0, fps=(25, 1)):
    """(ratio [n], [(first_frame, end_frame)]): end_frame is the first non-black frame, or the last frame of the clip."""
    n = len(frames)
    ratio = np.array([black_count(f[0], threshold) / np.size(f[0]) for f in frames])
    events, start = [], None
    for i in range(n + 1):
        black = i < n and ratio[i] >= ratio_th
        if black and start is None:
            start = i
        elif not black and start is not None:
            end = i if i < n else n - 1
            if (end - start) * fps[1] >= min_duration * fps[0]:
                events.append((start, end))
            start = None
    return ratio, events


def fault_clip(n_black, n_a, n_freeze, n_resume, n_b, w=64, h=48):
    """(refs, diss): 8-bit 4:2:0 frames [Y, U, V] with hand-computable integrity figures.  Content: Y = base + (x + 2 j) % 64
    at frame j (a ramp moving 2 columns per frame: mean |difference| 3.875 between neighbours), U = V = 128.  The
    distorted clip: n_black frames of Y = 16, n_a frames of base 60, n_freeze repeats of the frame that follows, n_resume
    more frames of base 60, then a hard cut to base 150 for n_b frames.  The reference is base 60 throughout."""
    assert w % 64 == 0
    x = np.arange(w)[None, :] + np.zeros((h, 1), np.int64)
    c = np.full(((h + 1) // 2, (w + 1) // 2), 128, np.uint8)

    def frame(base, j):
        return [(base + (x + 2 * j) % 64).astype(np.uint8), c.copy(), c.copy()]
    n = n_black + n_a + n_freeze + n_resume + n_b
    f0 = n_black + n_a
    refs = [frame(60, j) for j in range(n)]
    diss = []
    for j in range(n):
        if j < n_black:
            diss.append([np.full((h, w), 16, np.uint8), c.copy(), c.copy()])
        elif j < f0:
            diss.append(frame(60, j))
        elif j < f0 + n_freeze:
            diss.append(frame(60, f0))
        elif j < f0 + n_freeze + n_resume:
            diss.append(frame(60, j))
        else:
            diss.append(frame(150, j))
    return refs, diss
