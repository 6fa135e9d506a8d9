"""numpy restatement of `oip rescale` (include/oip_c.h: oip_rescale_taps, oip_rescale_size, oip_rescale_src_range,
oip_rescale_u16), written from the definition and not from the C++: the Q14 tap tables of an axis, the two passes with the
clamped 16-bit intermediate, the replicate border and the no-data rule.  Rasters are (lines, pixels * spp) uint16."""
import math

import numpy as np

KERNELS = {"lanczos": 3, "cubic": 2, "linear": 1}
PAIRS = ((64, 64), (203, 152), (203, 51), (203, 162), (61, 37), (50, 200), (37, 61), (64, 17), (517, 130), (517, 1034), (33, 528))


def h(kind, x):
    x = abs(x)
    if kind == "lanczos":
        if x >= 3.0:
            return 0.0
        if x == 0.0:
            return 1.0
        px = math.pi * x
        return (math.sin(px) / px) * (math.sin(px / 3.0) / (px / 3.0))
    if kind == "cubic":
        if x <= 1.0:
            return 1.5 * x ** 3 - 2.5 * x ** 2 + 1.0
        if x < 2.0:
            return -0.5 * x ** 3 + 2.5 * x ** 2 - 4.0 * x + 2.0
        return 0.0
    return max(0.0, 1.0 - x)


def taps_k(kind, n_in, n_out):
    a, mx = KERNELS[kind], max(n_in, n_out)
    return 2 * -(-a * mx // n_out)


def taps(kind, n_in, n_out, margins=None):
    """(first (n_out,) int32, taps (n_out, K) int16).  margins: a list that receives, per tap, the distance of its pre-rounding
    value from the nearest half-integer"""
    if n_in < 1 or n_out < 1 or n_in > 4 * n_out or n_out > 16 * n_in:
        raise ValueError("rescale: axis %d -> %d refused" % (n_in, n_out))
    K, mx = taps_k(kind, n_in, n_out), max(n_in, n_out)
    first = np.zeros(n_out, np.int32)
    out = np.zeros((n_out, K), np.int16)
    for o in range(n_out):
        num, den = (2 * o + 1) * n_in - n_out, 2 * n_out
        f = num // den - K // 2 + 1
        w = [h(kind, (2 * n_out * (f + k) - num) / (2 * mx)) for k in range(K)]
        s = 0.0
        for v in w:
            s += v
        pre = [v / s * 16384 for v in w]
        if margins is not None:
            margins.extend(abs(p - math.floor(p) - 0.5) for p in pre)
        t = [math.floor(p + 0.5) for p in pre]
        t[t.index(max(t))] += 16384 - sum(t)
        assert sum(abs(v) for v in t) <= 32767
        first[o] = f
        out[o] = t
    return first, out


def size(n_in, p, q):
    return (2 * n_in * p + q) // (2 * q)


def src_range(n_in, n_out, K, out0, outs):
    """(src0, srcs): the clamped index range that outputs [out0, out0 + outs) read"""
    if outs == 0:
        return 0, 0
    def first(o):
        return ((2 * o + 1) * n_in - n_out) // (2 * n_out) - K // 2 + 1
    lo = min(max(first(out0), 0), n_in - 1)
    hi = min(max(first(out0 + outs - 1) + K - 1, 0), n_in - 1)
    return lo, hi - lo + 1


def nearest(n_in, n_out):
    o = np.arange(n_out, dtype=np.int64)
    return (2 * o + 1) * n_in // (2 * n_out)


def rescale(src, spp, Wo, Lo, fx, tx, fy, ty, valid_min=0, rows=None):
    """the W x L x spp raster `src` on the Wo x Lo grid with the tables (fx, tx) across and (fy, ty) along; rows = (y0, n): only
    those output lines"""
    L, Ws = src.shape
    W = Ws // spp
    y0, n = (0, Lo) if rows is None else rows
    fy, ty = np.asarray(fy, np.int64)[y0:y0 + n], np.asarray(ty, np.int64)[y0:y0 + n]
    fx, tx = np.asarray(fx, np.int64), np.asarray(tx, np.int64)
    Ky, Kx = ty.shape[1], tx.shape[1]
    p = src.reshape(L, W, spp)
    s = p.astype(np.int64) - 32768
    v = np.zeros((n, W, spp), np.int64)
    bad = np.zeros((n, W, spp), bool)
    for k in range(Ky):
        idx = np.clip(fy + k, 0, L - 1)
        v += ty[:, k, None, None] * s[idx]
        bad |= p[idx] < valid_min
    v = np.clip((v + 8192) >> 14, -32768, 32767)
    out = np.zeros((n, Wo, spp), np.int64)
    flag = np.zeros((n, Wo, spp), bool)
    for k in range(Kx):
        idx = np.clip(fx + k, 0, W - 1)
        out += tx[None, :, k, None] * v[:, idx]
        flag |= bad[:, idx]
    out = np.clip(((out + 8192) >> 14) + 32768, 0, 65535)
    if valid_min > 0:
        near = p[nearest(L, Lo)[y0:y0 + n]][:, nearest(W, Wo)]
        out = np.where(flag, near, out)
    return out.astype(np.uint16).reshape(n, Wo * spp)


def rescale_kind(src, spp, Wo, Lo, kind="lanczos", valid_min=0):
    L, W = src.shape[0], src.shape[1] // spp
    fx, tx = taps(kind, W, Wo)
    fy, ty = taps(kind, L, Lo)
    return rescale(src, spp, Wo, Lo, fx, tx, fy, ty, valid_min)


def rescale_float(src, Wo, Lo, kind="lanczos"):
    """the same filter in floating point (single channel), for the distance of the Q14 form from it"""
    L, W = src.shape
    def matrix(n_in, n_out):
        K, mx = taps_k(kind, n_in, n_out), max(n_in, n_out)
        m = np.zeros((n_out, n_in))
        for o in range(n_out):
            num, den = (2 * o + 1) * n_in - n_out, 2 * n_out
            f = num // den - K // 2 + 1
            w = np.array([h(kind, (2 * n_out * (f + k) - num) / (2 * mx)) for k in range(K)])
            w /= w.sum()
            for k in range(K):
                m[o, min(max(f + k, 0), n_in - 1)] += w[k]
        return m
    return matrix(L, Lo) @ src.astype(np.float64) @ matrix(W, Wo).T
