"""The numpy restatement of the Wallis filter as include/oip_c.h states it: block moments (oip_block_moments_u16), the fit
(oip_wallis_fit) and the transform (oip_wallis_apply_u16).  Rasters are (rows, w * spp) uint16, pixel-interleaved; moments are
(3, spp, gh, gw) uint64; node tables are (gh, gw, spp).  The device side is integers, the fit one correctly rounded fp64
operation per step in the stated order -- Python floats and ints do exactly that."""
import math

import numpy as np

BLOCKS = (32, 64, 128, 256)
IDENTITY = (65536, 0)


def grid(w, h, B):
    return -(-w // B), -(-h // B)


def moments(img, spp, B, vmin=1, vmax=65535):
    """(3, spp, gh, gw) uint64: n, S1, S2 over the samples vmin <= v <= vmax of every block and channel"""
    rows, ws = img.shape
    w = ws // spp
    gw, gh = grid(w, rows, B)
    out = np.zeros((3, spp, gh, gw), np.uint64)
    v = img.reshape(rows, w, spp).astype(np.uint64)
    ok = (v >= vmin) & (v <= vmax)
    for c in range(spp):
        pad = np.zeros((3, gh * B, gw * B), np.uint64)
        pad[0, :rows, :w] = ok[:, :, c]
        pad[1, :rows, :w] = v[:, :, c] * ok[:, :, c]
        pad[2, :rows, :w] = v[:, :, c] * v[:, :, c] * ok[:, :, c]
        out[:, c] = pad.reshape(3, gh, B, gw, B).sum((2, 4), dtype=np.uint64)
    return out


def _fit_one(n, S1, S2, c, b, gmin, gmax, mt, st, need):
    D = n * S2 - S1 * S1
    if n < need or D <= 0:
        return None
    m = float(S1) / float(n)
    s = math.sqrt(float(D)) / float(n)
    den = c * s + (1.0 - c) * st
    g = (c * st) / den
    g = min(max(g, gmin), gmax)
    o = (b * mt + (1.0 - b) * m) - g * m
    return int(np.rint(g * 65536.0)), int(np.rint(o * 256.0))


def fit(acc, c=0.8, b=0.6, gmin=0.25, gmax=4.0, min_count=0, mean=None, std=None):
    """(gain_q16, offset_q8, substituted) as (gh, gw, spp) int32 and the (spp, 9) report; ValueError / RuntimeError as the
    C entry point's INVALID / RUNTIME"""
    acc = np.asarray(acc)
    _, spp, gh, gw = acc.shape
    if not (0.0 < c <= 1.0 and 0.0 <= b <= 1.0 and 0.0 < gmin <= 1.0 <= gmax <= 16.0) or spp not in (1, 4):
        raise ValueError("bad argument")
    need = max(int(min_count), 2)
    G, O, sub = (np.zeros((gh, gw, spp), np.int32) for _ in range(3))
    report = np.zeros((spp, 9))
    for ch in range(spp):
        given_m = None if mean is None or math.isnan(mean[ch]) else float(mean[ch])
        given_s = None if std is None or math.isnan(std[ch]) else float(std[ch])
        if (given_m is not None and not 0.0 <= given_m <= 65535.0) or (given_s is not None and not given_s <= 65535.0):
            raise ValueError("bad argument")
    for ch in range(spp):
        n, S1, S2 = ([[int(v) for v in row] for row in acc[k, ch]] for k in range(3))
        N, A, Q = (sum(sum(row) for row in p) for p in (n, S1, S2))
        if N < need:
            raise RuntimeError("channel %d: too few samples" % ch)
        D0 = N * Q - A * A
        m0 = float(A) / float(N)
        s0 = math.sqrt(float(D0)) / float(N)
        mt = m0 if mean is None or math.isnan(mean[ch]) else float(mean[ch])
        st = s0 if std is None or math.isnan(std[ch]) else float(std[ch])
        if not st > 0.0:
            raise RuntimeError("channel %d: target std not positive" % ch)
        args = (c, b, gmin, gmax, mt, st, need)
        g0 = _fit_one(N, A, Q, *args) if D0 != 0 else IDENTITY
        for j in range(gh):
            for i in range(gw):
                r = _fit_one(n[j][i], S1[j][i], S2[j][i], *args)
                sub[j, i, ch] = r is None
                G[j, i, ch], O[j, i, ch] = g0 if r is None else r
        report[ch] = (N, m0, s0, mt, st, gh * gw, int(sub[:, :, ch].sum()), int(G[:, :, ch].min()), int(G[:, :, ch].max()))
    return G, O, sub, report


def interp(V, n, B, pos):
    """the nodes V (n, ...) along axis 0 at the integer positions pos -> (len(pos), ...) int64"""
    h = B // 2
    u = np.asarray(pos, np.int64) - h
    k = np.clip(np.floor_divide(u, B), 0, max(n - 2, 0))
    t = np.clip(u - k * B, 0, B)
    k2 = np.minimum(k + 1, n - 1)
    t = t.reshape((len(u),) + (1,) * (V.ndim - 1))
    V = V.astype(np.int64)
    return np.floor_divide(V[k] * (B - t) + V[k2] * t + h, B)


def tables(G, O, B, W, L, row0=0, rows=None):
    """G(y, x, c), O(y, x, c) of the lines [row0, row0 + rows) as (rows, W, spp) int64"""
    gh, gw, _ = G.shape
    assert (gw, gh) == grid(W, L, B)
    rows = L - row0 if rows is None else rows
    out = []
    for V in (G, O):
        Vy = interp(V, gh, B, np.arange(row0, row0 + rows))                           # (rows, gw, spp)
        out.append(interp(Vy.transpose(1, 0, 2), gw, B, np.arange(W)).transpose(1, 0, 2))
    return out


def apply(img, spp, G, O, B, vmin=1, vmax=65535, cmax=65535, row0=0, L=None):
    """the lines img of a raster of L lines (img holds [row0, row0 + len(img))) -> (out uint16, the three counters uint64)"""
    rows, ws = img.shape
    W = ws // spp
    L = rows if L is None else L
    Gx, Ox = tables(G, O, B, W, L, row0, rows)
    v = img.reshape(rows, W, spp).astype(np.int64)
    q = (Gx * v + 256 * Ox + 32768) >> 16
    valid = (v >= vmin) & (v <= vmax)
    out = np.where(valid, np.clip(q, vmin, cmax), v).astype(np.uint16).reshape(rows, ws)
    counts = np.array([valid.sum(), (valid & (q < vmin)).sum(), (valid & (q > cmax)).sum()], np.uint64)
    return out, counts


def plain(img, g, o, vmin=1, vmax=65535, cmax=65535):
    """the per-sample transform with one (G, O)"""
    v = img.astype(np.int64)
    q = (g * v + 256 * o + 32768) >> 16
    return np.where((v >= vmin) & (v <= vmax), np.clip(q, vmin, cmax), v).astype(np.uint16)


def random_raster(rows, ws, seed, lo=0, hi=4096, specials=(0, 65535), rate=0.02):
    """uniform samples in [lo, hi) with a share of zeros and of 65535"""
    rng = np.random.default_rng(seed)
    img = rng.integers(lo, hi, (rows, ws)).astype(np.uint16)
    for s in specials:
        img[rng.random((rows, ws)) < rate] = s
    return img


def random_nodes(gh, gw, spp, seed):
    """node tables over the whole allowed range: G in [16384, 2^20], O in +-2^28, the extremes among them"""
    rng = np.random.default_rng(seed)
    G = rng.integers(16384, (1 << 20) + 1, (gh, gw, spp)).astype(np.int32)
    O = rng.integers(-(1 << 28), (1 << 28) + 1, (gh, gw, spp)).astype(np.int32)
    flat_g, flat_o = G.reshape(-1), O.reshape(-1)
    flat_g[0], flat_o[0] = 1 << 20, -(1 << 28)
    flat_g[-1], flat_o[-1] = 16384, 1 << 28
    return G, O


def mild_nodes(gh, gw, spp, seed):
    """node tables as a fit produces them on 12-bit data: gains 0.25 .. 4, offsets within +-2000 DN"""
    rng = np.random.default_rng(seed)
    G = rng.integers(16384, (1 << 18) + 1, (gh, gw, spp)).astype(np.int32)
    O = rng.integers(-2000 * 256, 2000 * 256 + 1, (gh, gw, spp)).astype(np.int32)
    return G, O


def scene(H=700, W=900, seed=0):
    """a mean of 1500 with Gaussian texture of sigma 300, times a radial falloff to 0.5 at the corners, clipped to 1..4095"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    tex = 1500 + 300 * rng.standard_normal((H, W))
    vig = 1.0 - 0.5 * (((xx - W / 2) / (W / 2)) ** 2 + ((yy - H / 2) / (H / 2)) ** 2) / 2
    return np.clip(tex * vig, 1, 4095).astype(np.uint16)


def block_means(acc):
    """(gh, gw) float64 means of channel 0 from its moments"""
    return acc[1, 0].astype(np.float64) / np.maximum(acc[0, 0], 1).astype(np.float64)
