"""Restatement of the quick-look arithmetic for the tests, in the terms include/oip_c.h states it: numpy integer block sums
for the decimation, np.bincount for the histogram, np.sort for the percentile limits and the integer stretch formula."""
import math

import numpy as np


def decimate(img, F):
    """(rows, w) -> (ceil(rows / F), ceil(w / F)) uint16, or (rows, w, spp) -> (spp, ...) planes: q = (S + n // 2) // n"""
    img = np.asarray(img)
    if img.ndim == 3:
        return np.stack([decimate(img[:, :, c], F) for c in range(img.shape[2])])
    rows, w = img.shape
    if rows > 64 * F:                                    # blocks of lines: the int64 copies of a large raster stay small
        return np.concatenate([decimate(img[r:r + 64 * F], F) for r in range(0, rows, 64 * F)])
    ys, xs = np.arange(0, rows, F), np.arange(0, w, F)
    S = np.add.reduceat(np.add.reduceat(img.astype(np.int64), ys, axis=0), xs, axis=1)
    n = np.outer(np.minimum(F, rows - ys), np.minimum(F, w - xs))
    return ((S + n // 2) // n).astype(np.uint16)


def histogram(img):
    return np.bincount(np.asarray(img).ravel(), minlength=65536).astype(np.uint64)


def stretch_limits(samples, valid_min=1, valid_max=65535, p_lo=2.0, p_hi=98.0):
    """(lo, hi, N) from the samples themselves: the values at sorted index r among the valid ones"""
    v = np.asarray(samples).ravel()
    v = np.sort(v[(v >= valid_min) & (v <= valid_max)])
    N = int(v.size)
    if N == 0:
        return 0, 0, 0
    rank = lambda p: min(N - 1, int(math.floor(float(N) * p / 100.0)))  # noqa: E731
    return int(v[rank(p_lo)]), int(v[rank(p_hi)]), N


def stretch_lut(lo, hi):
    v = np.arange(65536, dtype=np.int64)
    span = hi - lo
    if span == 0:
        return np.where(v < lo, 0, 255).astype(np.uint8)
    return (((np.clip(v, lo, hi) - lo) * 510 + span) // (2 * span)).astype(np.uint8)


def quicklook(planes, **kw):
    """decimated planes (one per output channel, in output order) -> ((rows, w[, 3]) uint8, [(lo, hi, N) per channel])"""
    lim = [stretch_limits(p, **kw) for p in planes]
    out = [stretch_lut(lo, hi)[p] for p, (lo, hi, _) in zip(planes, lim)]
    return (out[0] if len(out) == 1 else np.stack(out, -1)), lim
