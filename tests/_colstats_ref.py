"""Restatement of the RRC calibration arithmetic for the tests: numpy integer sums for the column statistics, Python
integers and math.sqrt for the fit, in the operation order include/oip_c.h states for oip_rrc_fit_columns."""
import math

import numpy as np


def totals(img, valid_min=0, valid_max=65535):
    """(3, w) uint64 planes n, S1, S2 of a (rows, w) uint16 raster; only valid_min <= v <= valid_max count"""
    img = np.asarray(img)
    out = np.zeros((3, img.shape[1]), np.uint64)
    for r in range(0, img.shape[0], 1024):                # blocks of lines: the uint64 copies of a large raster stay small
        v = img[r:r + 1024].astype(np.uint64)
        ok = (v >= valid_min) & (v <= valid_max)
        v = np.where(ok, v, np.uint64(0))
        out += np.stack([ok.sum(0, dtype=np.uint64), v.sum(0, dtype=np.uint64), (v * v).sum(0, dtype=np.uint64)])
    return out


def fit_columns(acc, groups, mode, min_count):
    """-> kb (w, 2) float64, dead columns per group, (mu_ref, sigma_ref) per group.  Python floats are IEEE doubles and
    int / int, float(int), math.sqrt and the four operations round correctly, as the C code's do."""
    w = acc.shape[1]
    gw = w // groups
    moments = mode == "moments"
    need = max(int(min_count), 2 if moments else 1)
    kb = np.zeros((w, 2))
    dead, ref = [], []
    for g in range(groups):
        mu, sigma = {}, {}
        for x in range(g * gw, (g + 1) * gw):
            n, s1, s2 = int(acc[0, x]), int(acc[1, x]), int(acc[2, x])
            if n < need:
                continue
            if moments:
                D = n * s2 - s1 * s1
                if D <= 0:
                    continue
                sigma[x] = math.sqrt(float(D)) / float(n)
            elif s1 == 0:
                continue
            mu[x] = float(s1) / float(n)
        if not mu:
            raise RuntimeError("group %d has no usable column" % g)
        mu_ref = 0.0
        for x in sorted(mu):
            mu_ref += mu[x]
        mu_ref /= float(len(mu))
        sigma_ref = 0.0
        if moments:
            for x in sorted(sigma):
                sigma_ref += sigma[x]
            sigma_ref /= float(len(sigma))
        for x in range(g * gw, (g + 1) * gw):
            if x not in mu:
                kb[x] = (1.0, 0.0)
            elif moments:
                k = sigma_ref / sigma[x]
                kb[x] = (k, mu_ref - k * mu[x])
            else:
                kb[x] = (mu_ref / mu[x], 0.0)
        dead.append(gw - len(mu))
        ref.append((mu_ref, sigma_ref))
    return kb, dead, np.array(ref)
