"""The restatement of `oip noise` (include/oip_c.h, section "noise"): the block keys in numpy int64 and, block by block, in
Python integers; the three host functions operation by operation in Python floats (IEEE fp64, one rounding per operation, as
the library's); the report's text; and the seeded scene of the estimator-recovery tests."""
import math

import numpy as np

NODATA, STRUCTURED = 0x00FF, 0x01FF


# ---- keys ---------------------------------------------------------------------------------------------------------------------
def key_of_block(block, level_shift, valid_min=1, valid_max=65535):
    """the key of one (B, B) block of one channel, in Python integers"""
    B = len(block)
    n = B * B
    v = [[int(x) for x in row] for row in block]
    if any(x < valid_min or x > valid_max for row in v for x in row):
        return NODATA
    S1 = sum(sum(row) for row in v)
    S2 = sum(x * x for row in v for x in row)
    D = n * S2 - S1 * S1
    h = B // 2
    Sq = [sum(v[j][i] for j in range(j0, j0 + h) for i in range(i0, i0 + h)) for j0 in (0, h) for i0 in (0, h)]
    E = 4 * sum(s * s for s in Sq) - S1 * S1
    assert 0 <= E <= D and E * (n - 4) < 1 << 56
    if E * (n - 4) > 12 * (D - E):
        return STRUCTURED
    level = min(255, (S1 // n) >> level_shift)
    q = min(254, math.isqrt((16 * D) // (n * (n - 1))))
    return level << 8 | q


def keys(img, spp, B, level_shift, valid_min=1, valid_max=65535):
    """(spp, floor(rows / B), floor(w / B)) uint16 keys of a (rows, w * spp) raster, numpy int64"""
    img = np.asarray(img)
    rows, w = img.shape[0], img.shape[1] // spp
    nby, nbx = rows // B, w // B
    n, h = B * B, B // 2
    x = img[:nby * B, :nbx * B * spp].astype(np.int64).reshape(nby, B, nbx, B, spp)
    x = x.transpose(4, 0, 2, 1, 3)                                      # (spp, nby, nbx, B, B)
    S1 = x.sum(axis=(3, 4))
    S2 = (x * x).sum(axis=(3, 4))
    D = n * S2 - S1 * S1
    Sq = x.reshape(spp, nby, nbx, 2, h, 2, h).sum(axis=(4, 6))          # (spp, nby, nbx, 2, 2)
    E = 4 * (Sq * Sq).sum(axis=(3, 4)) - S1 * S1
    assert (E >= 0).all() and (D >= E).all()
    nodata = ((x < valid_min) | (x > valid_max)).any(axis=(3, 4))
    structured = E * (n - 4) > 12 * (D - E)
    level = np.minimum(255, (S1 // n) >> level_shift)
    t = (16 * D) // (n * (n - 1))
    r = np.floor(np.sqrt(t.astype(np.float64))).astype(np.int64)
    r = np.where(r * r > t, r - 1, r)
    r = np.where((r + 1) * (r + 1) <= t, r + 1, r)
    assert ((r * r <= t) & ((r + 1) * (r + 1) > t)).all()
    key = level << 8 | np.minimum(254, r)
    key = np.where(structured, STRUCTURED, key)
    key = np.where(nodata, NODATA, key)
    return key.astype(np.uint16)


def histogram(key_plane):
    return np.bincount(np.asarray(key_plane).reshape(-1).astype(np.int64), minlength=65536).astype(np.uint64)


# ---- host functions -----------------------------------------------------------------------------------------------------------
def levels(hist, min_blocks):
    """(sigma (256,) with -1 where not usable, blocks (256,), usable levels)"""
    hist = [int(v) for v in np.asarray(hist).reshape(-1)]
    sigma, blocks, usable = [-1.0] * 256, [0] * 256, 0
    for lv in range(256):
        h = hist[lv * 256:lv * 256 + 256]
        N = sum(h[:255])
        blocks[lv] = N
        if N < max(min_blocks, 1):
            continue
        best = max(h[:254])
        if best == 0:
            continue
        k = h[:254].index(best)
        r = k // 8 + 1
        lo, hi = max(0, k - r), min(253, k + r)
        cw = sum(h[lo:hi + 1])
        if 10 * cw < 3 * N:
            continue
        s = 0.0
        for q in range(lo, hi + 1):
            s = s + (float(q) + 0.5) * float(h[q])
        sigma[lv] = 0.25 * s / float(cw)
        usable += 1
    return np.array(sigma), np.array(blocks, dtype=np.uint64), usable


def fit(sigma, blocks, level_shift):
    """(a, b, mu_ref); None without a usable level"""
    use = [lv for lv in range(256) if sigma[lv] >= 0.0]
    if not use or sum(int(blocks[lv]) for lv in use) == 0:
        return None
    scale = float(1 << level_shift)
    mu = {lv: (float(lv) + 0.5) * scale for lv in use}
    sw = swx = swv = swxv = swxx = 0.0
    for lv in use:
        m, v, w = mu[lv], float(sigma[lv]) * float(sigma[lv]), float(int(blocks[lv]))
        sw = sw + w
        swx = swx + w * m
        swv = swv + w * v
        swxv = swxv + w * m * v
        swxx = swxx + w * m * m
    mx, mv = swx / sw, swv / sw
    sxx = sxy = 0.0
    for lv in use:
        m, v, w = mu[lv], float(sigma[lv]) * float(sigma[lv]), float(int(blocks[lv]))
        sxx = sxx + w * (m - mx) * (m - mx)
        sxy = sxy + w * (m - mx) * (v - mv)
    a, b = mv, 0.0
    if len(use) >= 2 and sxx != 0.0:
        b = sxy / sxx
        a = mv - b * mx
        if b < 0.0:
            a, b = mv, 0.0
        elif a < 0.0:
            a, b = 0.0, swxv / swxx
    total, cum, mu_ref = sum(int(blocks[lv]) for lv in use), 0, None
    for lv in use:
        cum += int(blocks[lv])
        if 2 * cum >= total:
            mu_ref = mu[lv]
            break
    return a, b, mu_ref


def despike_threshold(a, b, mu_ref, k):
    """(thr_abs, thr_rel_q8); None where the library refuses"""
    st = math.sqrt(a + b * mu_ref)
    if st == 0.0:
        return None
    R = k * b / (2.0 * st)
    N0 = k * st - R * mu_ref
    q8, ta = math.ceil(256.0 * R), math.ceil(N0) + 1
    if q8 > 256 or ta > 65535:
        return None
    return ta, q8


# ---- the report ---------------------------------------------------------------------------------------------------------------
def report_rows(band, sigma, blocks, level_shift):
    """the report's rows of one band (1-based), as the tool prints them"""
    out = []
    for lv in range(256):
        if sigma[lv] >= 0.0:
            mu = (lv + 0.5) * (1 << level_shift)
            out.append("%d,%d,%d,%d,%.6f,%.4f" % (band, lv << level_shift, ((lv + 1) << level_shift) - 1, int(blocks[lv]), sigma[lv], mu / sigma[lv]))
    return out


def parse_report(path):
    """(rows as printed, {band: dict of the band line's fields, numbers as float})"""
    rows, bands = [], {}
    for line in open(path):
        line = line.rstrip("\n")
        if line.startswith("# band "):
            head, rest = line[7:].split(":", 1)
            tok = rest.split()
            bands[int(head)] = {tok[i]: float(tok[i + 1]) for i in range(0, len(tok), 2)}
        elif line and not line.startswith("#"):
            rows.append(line)
    return rows, bands


# ---- the scene of the recovery tests --------------------------------------------------------------------------------------------
RECOVERY_MODELS = ((4.0, 0.01), (1.0, 0.002), (30.0, 0.05))


def scene(a0, b0, seed, W=1024, L=512):
    """1024 x 512 lines: flat steps 52 pixels wide from 300 to 3800 DN, the last third of the lines with a texture of amplitude 200
    added, clipped to 50..4000; plus Gaussian noise of variance a0 + b0 * scene, rounded, clipped to 1..65535"""
    y, x = np.mgrid[0:L, 0:W].astype(np.float64)
    s = 300.0 + 3500.0 * ((x // 52) * 52) / (W - 1)
    s[L - L // 3:] += (200.0 * np.sin(0.9 * x) * np.sin(0.7 * y))[L - L // 3:]
    s = np.clip(s, 50.0, 4000.0)
    rng = np.random.default_rng(seed)
    noisy = s + rng.standard_normal(s.shape) * np.sqrt(a0 + b0 * s)
    return np.clip(np.rint(noisy), 1, 65535).astype(np.uint16)


def recovery_errors(sigma, a, b, a0, b0, level_shift):
    """(largest relative error of a usable level's sigma, of a, of b) against the truth sigma^2 = a0 + b0 mu + 1 / 12"""
    worst = 0.0
    for lv in range(256):
        if sigma[lv] >= 0.0:
            truth = math.sqrt(a0 + b0 * (lv + 0.5) * (1 << level_shift) + 1.0 / 12.0)
            worst = max(worst, abs(sigma[lv] - truth) / truth)
    return worst, abs(a - (a0 + 1.0 / 12.0)) / (a0 + 1.0 / 12.0), abs(b - b0) / b0
