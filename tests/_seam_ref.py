"""Restatement of the seam arithmetic for the tests (the reference has no such step, so this file is the yardstick): numpy
integer sums for the overlap totals, Python integers and math.sqrt for the fit in the operation order include/oip_c.h states
for oip_seam_fit, int64 arithmetic for the per-sample formula of oip_stitch_balanced_u16.  Images are (L, W * spp) uint16,
pixel-interleaved; `fold` and `h` are in pixels."""
import math

import numpy as np


def build_pair(W, L, fold, g, o, seed, spp=1):
    """the construction the issue's checks use: one scene of 2 W - 2 fold columns uniform in 300..3800 (nothing clamps),
    left = its first W columns, right = its last W columns seen through b = (scene - o) / g, rounded.  g, o: scalars or one
    value per channel."""
    rng = np.random.default_rng(seed)
    scene = rng.integers(300, 3801, (L, 2 * W - 2 * fold, spp)).astype(np.float64)
    g = np.broadcast_to(np.asarray(g, np.float64), (spp,))
    o = np.broadcast_to(np.asarray(o, np.float64), (spp,))
    left = scene[:, :W].astype(np.uint16)
    right = np.clip(np.rint((scene[:, W - 2 * fold:] - o) / g), 0, 65535).astype(np.uint16)
    return left.reshape(L, W * spp), right.reshape(L, W * spp)


def overlap(left, right, fold, spp):
    """(a, b): the overlap pairs as (L, 2 fold, spp) arrays"""
    L, Ws = left.shape
    fs = fold * spp
    return left[:, Ws - 2 * fs:].reshape(L, 2 * fold, spp), right[:, :2 * fs].reshape(L, 2 * fold, spp)


def moments(left, right, fold, spp, valid_min=0, valid_max=65535):
    """(6, spp) uint64: n, Sa, Sb, Saa, Sbb, Sab over the pairs whose two samples lie in [valid_min, valid_max]"""
    a, b = overlap(left, right, fold, spp)
    a, b = a.astype(np.uint64), b.astype(np.uint64)
    ok = (a >= valid_min) & (a <= valid_max) & (b >= valid_min) & (b <= valid_max)
    a, b = np.where(ok, a, np.uint64(0)), np.where(ok, b, np.uint64(0))
    planes = [ok.astype(np.uint64), a, b, a * a, b * b, a * b]
    return np.stack([p.sum((0, 1), dtype=np.uint64) for p in planes])


def fit(acc, mode, min_count=0):
    """-> gain_q16, offset_q16, identity (lists of int), report (spp, 6).  Python floats are IEEE doubles; float(int),
    int / int via floats, math.sqrt and the four operations round correctly, as the C code's do; round() is rint."""
    spp = acc.shape[1]
    need = max(int(min_count), 2)
    G, O, ident, report = [], [], [], np.zeros((spp, 6))
    for c in range(spp):
        n, Sa, Sb, Saa, Sbb, Sab = (int(acc[k, c]) for k in range(6))
        Da, Db, Dab = max(n * Saa - Sa * Sa, 0), max(n * Sbb - Sb * Sb, 0), n * Sab - Sa * Sb
        mean_a = mean_b = sigma_a = sigma_b = r = 0.0
        if n > 0:
            nd = float(n)
            mean_a, mean_b = float(Sa) / nd, float(Sb) / nd
            ra, rb = math.sqrt(float(Da)), math.sqrt(float(Db))
            sigma_a, sigma_b = ra / nd, rb / nd
            if Da and Db:
                r = float(Dab) / (ra * rb)
        report[c] = (float(n), mean_a, mean_b, sigma_a, sigma_b, r)
        G.append(65536), O.append(0), ident.append(1)
        if n < need:
            continue
        g = 1.0
        if mode == "moments":
            if Da == 0 or Db == 0:
                continue
            g = math.sqrt(float(Da) / float(Db))
        elif mode == "gain":
            if Sb == 0:
                continue
            g = float(Sa) / float(Sb)
        Gc = round(g * 65536.0)
        if not 16384 <= Gc <= 262144:
            raise ValueError("channel %d: gain_q16 %d" % (c, Gc))
        Oc = 0
        if mode != "gain":
            gq = float(Gc) / 65536.0
            Oc = round((mean_a - gq * mean_b) * 65536.0)
            if not -2 ** 31 <= Oc < 2 ** 31:
                raise ValueError("channel %d: offset_q16 %d" % (c, Oc))
        G[c], O[c], ident[c] = Gc, Oc, 0
    return G, O, ident, report


def balance(b, G, O):
    """b' = clamp((G b + O + 32768) >> 16, 0, 65535); b: (..., spp), G, O: one per channel"""
    G, O = np.asarray(G, np.int64), np.asarray(O, np.int64)
    return np.clip((G * b.astype(np.int64) + O + 32768) >> 16, 0, 65535)


def stitch(left, right, fold, spp, G, O, h, valid_min):
    """the (L, 2 (W - fold) spp) uint16 product of oip_stitch_balanced_u16"""
    L, Ws = left.shape
    W = Ws // spp
    s = W - fold
    a = left.reshape(L, W, spp).astype(np.int64)
    bb = right.reshape(L, W, spp).astype(np.int64)
    out = np.empty((L, 2 * s, spp), np.int64)
    out[:, :s - h] = a[:, :s - h]
    out[:, s + h:] = balance(bb[:, fold + h:], G, O)               # p - (W - 2 fold) for p >= s + h
    if h:
        za = a[:, s - h:s + h]
        zb = bb[:, fold - h:fold + h]
        zbb = balance(zb, G, O)
        t = np.arange(2 * h, dtype=np.int64)[None, :, None]
        wr = 2 * t + 1
        wl = 4 * h - wr
        z = (wl * za + wr * zbb + 2 * h) // (4 * h)
        z = np.where(zb < valid_min, za, z)
        z = np.where(za < valid_min, zbb, z)
        out[:, s - h:s + h] = z
    return out.astype(np.uint16).reshape(L, 2 * s * spp)
