"""The numpy model of yrt_render_adaptive's contrast rule (include/yrt.h, step 2) and of its
output (not a test module).

flags(B, threshold): pixel P of the (H, W, >= 3) float32 frame B is flagged iff a pixel Q of the
frame with max(|Px-Qx|, |Py-Qy|) == 1 and a channel c of r, g, b exist with
abs(B[P].c - B[Q].c) > threshold, in float32, an IEEE comparison (false on NaN). It is written as
an OR of comparisons over the eight offsets, never as a maximum: a NaN difference must drop out
of the one comparison it is in and nothing else.
"""
import numpy as np

OFFSETS = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0)]


def flags(base, threshold) -> np.ndarray:
    """(H, W) bool"""
    b = np.asarray(base, np.float32)[..., :3]
    h, w = b.shape[:2]
    t = np.float32(threshold)
    out = np.zeros((h, w), bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for dy, dx in OFFSETS:
            # P over the pixels that have a neighbour at this offset inside the frame, Q that neighbour
            py = slice(max(0, -dy), h - max(0, dy))
            px = slice(max(0, -dx), w - max(0, dx))
            qy = slice(max(0, dy), h - max(0, -dy))
            qx = slice(max(0, dx), w - max(0, -dx))
            d = np.abs((b[py, px] - b[qy, qx]).astype(np.float32))
            out[py, px] |= (d > t).any(axis=-1)
    return out


def flags_brute(base, threshold) -> np.ndarray:
    """the same rule as a double loop over P and its neighbours, one scalar comparison at a time"""
    b = np.asarray(base, np.float32)
    h, w = b.shape[:2]
    t = np.float32(threshold)
    out = np.zeros((h, w), bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for y in range(h):
            for x in range(w):
                for dy, dx in OFFSETS:
                    qy, qx = y + dy, x + dx
                    if not (0 <= qy < h and 0 <= qx < w):
                        continue
                    for c in range(3):
                        if np.abs(np.float32(b[y, x, c] - b[qy, qx, c])) > t:
                            out[y, x] = True
    return out


def compose(flag, full, base) -> np.ndarray:
    """the adaptive frame: the full render's pixel where flagged, the base frame's elsewhere"""
    return np.where(np.asarray(flag, bool)[..., None], full, base).astype(np.float32)
