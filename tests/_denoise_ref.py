"""numpy restatement of oip_sigma_filter_u16 and oip_denoise_thresholds, written from the text of include/oip_c.h (the sigma
filter section), not from the kernel; plus the test image and the test table of the denoise tests.

    c < valid_min:  out = c
    T0 = thr[ch][c >> 8];  lo0 = max(c - T0, valid_min), hi0 = min(c + T0, 65535)
    stage 1 over 3 x 3:           S1, m1 = sum, count of the n with lo0 <= n <= hi0;  c1 = (2 S1 + m1) // (2 m1)
    T1 = thr[ch][c1 >> 8]; lo = max(c1 - T1, valid_min), hi = min(c1 + T1, 65535)
    stage 2 over (2r+1) x (2r+1): S, m = sum, count of the n with lo <= n <= hi
    m < min_members: out = c;  else out = (2 S + m) // (2 m)
Neighbours are samples of the same channel; the border is replicated (pixel and line index clamped)."""
import math

import numpy as np


def _window(a, lo, hi, r):
    """(S, m) over the (2r+1)^2 replicated-border neighbourhood of every sample of a (L, W, spp) int64 array"""
    L, W, _ = a.shape
    p = np.pad(a, ((r, r), (r, r), (0, 0)), mode="edge")
    S = np.zeros_like(a)
    m = np.zeros_like(a)
    for j in range(2 * r + 1):
        for i in range(2 * r + 1):
            n = p[j:j + L, i:i + W]
            k = (n >= lo) & (n <= hi)
            S += np.where(k, n, 0)
            m += k
    return S, m


def sigma_filter_parts(img, thr, radius, min_members=None, valid_min=1, spp=1):
    """dict of out (uint16, the shape of img), c1, T0, T1, m, filt (each (L, W * spp)) and stats (the four counters) for a
    (L, W * spp) uint16 image and a (spp, 256) table"""
    img = np.asarray(img)
    L, Ws = img.shape
    W = Ws // spp
    assert img.dtype == np.uint16 and W * spp == Ws and radius in (1, 2, 3)
    min_members = 2 * radius + 1 if min_members is None else min_members
    assert 1 <= min_members <= (2 * radius + 1) ** 2 and 0 <= valid_min <= 65535
    t = np.asarray(thr).reshape(spp, 256).astype(np.int64)
    ch = np.arange(spp)[None, None, :]
    c = img.reshape(L, W, spp).astype(np.int64)
    alive = c >= valid_min
    T0 = t[ch, c >> 8]
    S1, m1 = _window(c, np.maximum(c - T0, valid_min), np.minimum(c + T0, 65535), 1)
    assert (m1[alive] >= 1).all()
    c1 = np.where(alive, (2 * S1 + m1) // np.maximum(2 * m1, 1), c)
    T1 = t[ch, c1 >> 8]
    S, m = _window(c, np.maximum(c1 - T1, valid_min), np.minimum(c1 + T1, 65535), radius)
    filt = alive & (m >= min_members)
    out = np.where(filt, (2 * S + m) // np.maximum(2 * m, 1), c)
    assert out.min() >= 0 and out.max() <= 65535
    stats = [int(alive.sum()), int((alive & ~filt).sum()), int(m[filt].sum()), int((out != c).sum())]
    flat = lambda x: x.reshape(L, Ws)
    return dict(out=flat(out).astype(np.uint16), c1=flat(c1), T0=flat(T0), T1=flat(T1), m=flat(np.where(alive, m, 0)), filt=flat(filt),
                alive=flat(alive), stats=stats)


def sigma_filter(img, thr, radius, min_members=None, valid_min=1, spp=1):
    return sigma_filter_parts(img, thr, radius, min_members, valid_min, spp)["out"]


def thresholds(a, b, k):
    """oip_denoise_thresholds: thr[l] = min(65535, ceil(k * sqrt(a + b * (256 l + 128)))), fp64; None for the model without noise"""
    if a == 0.0 and b == 0.0:
        return None
    out = np.zeros(256, np.uint16)
    for l in range(256):
        s = math.sqrt(a + b * float(256 * l + 128))
        out[l] = 65535 if math.isinf(s) else min(65535, math.ceil(k * s))
    return out


# The residual standard deviation of a flat noisy field over the input's (a = 9, b = 0.02, K = 2, M = 2r + 1), measured with this
# restatement on 256 x 256, seeds 1..3 at levels 500 and 30000 (six values per radius, min .. max):
#   r = 1: 0.422 .. 0.448      r = 2: 0.283 .. 0.312      r = 3: 0.230 .. 0.258          (box-filter floors: 1/3, 1/5, 1/7)
# The bar is 1.15 x the largest, the margin for the seed-to-seed scatter of such a field.
FLAT_BARS = {1: 1.15 * 0.448, 2: 1.15 * 0.312, 3: 1.15 * 0.258}


def table(spp):
    """the test table: thr[ch][l] = 20 + l * (2 + ch)"""
    return np.array([[20 + l * (2 + ch) for l in range(256)] for ch in range(spp)], np.uint16)


def image(W, L, spp, seed):
    """a ramp 200 .. 65200 across the line (every table level, both range clamps), Gaussian noise whose amplitude goes through
    3 / 30 / 300 / 3000 every 4 lines, clipped to u16, 3 % zeros"""
    rng = np.random.default_rng(seed)
    ramp = np.linspace(200.0, 65200.0, W) if W > 1 else np.array([200.0])
    amp = np.array([3.0, 30.0, 300.0, 3000.0])[(np.arange(L) // 4) % 4]
    v = ramp[None, :, None] + rng.normal(0.0, 1.0, (L, W, spp)) * amp[:, None, None]
    img = np.clip(np.rint(v), 0, 65535).astype(np.uint16)
    img[rng.random(img.shape) < 0.03] = 0
    return img.reshape(L, W * spp)
