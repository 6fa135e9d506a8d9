"""The definition of `oip mtf` restated in numpy and plain Python (include/oip_c.h states it): the tile records and the
edge-spread sums of oip_mtf_tiles_u16 / oip_mtf_esf_u16 in exact integers, the host steps oip_mtf_tile, oip_mtf_summary and
oip_mtf_tv_slack in fp64 in the stated order, and a planter of slanted edges with a known MTF at Nyquist."""
import math

import numpy as np

T = 32
DEN = 87296                                                            # 32 * sum r^2 - (sum r)^2, r = 0..31
OK, NODATA, FLAT, LOWCONTRAST, TEXTURED, OFFCENTRE, SLANT, CURVED = range(8)
STATUS_NAMES = ("ok", "nodata", "flat", "lowcontrast", "textured", "offcentre", "slant", "curved")
_R = np.arange(32, dtype=np.int64)


def tile_counts(w, rows, axis):
    """(tile lines, tiles per line) of a w x rows window"""
    if w < T or rows < T:
        return 0, 0
    return (rows // T, (w - T) // 16 + 1) if axis == 0 else ((rows - T) // 16 + 1, w // T)


def tiles(plane, axis):
    """(nty, ntx, 32 profiles, 32 samples) int64 of one channel's (rows, w) plane"""
    rows, w = plane.shape
    nty, ntx = tile_counts(w, rows, axis)
    if nty == 0 or ntx == 0:
        return np.zeros((nty, ntx, T, T), np.int64)
    v = np.lib.stride_tricks.sliding_window_view(plane, (T, T))
    v = v[::T, ::16] if axis == 0 else v[::16, ::T].transpose(0, 1, 3, 2)
    return v[:nty, :ntx].astype(np.int64)


def analyse(p, contrast_min=200, tv_slack=256, valid_min=1, valid_max=65535):
    """records (..., 4) int32, the fitted line f (..., 32) in Q7 and sum S0_r, of tiles p (..., 32, 32)"""
    p = np.asarray(p, dtype=np.int64)
    D = p[..., 31] - p[..., 0]
    d = np.diff(p, axis=-1)
    sD = D.sum(-1)
    s = np.sign(sD)
    S0 = s[..., None] * D
    TV = np.abs(d).sum(-1)
    S1 = s[..., None] * (d * (2 * _R[:31] + 1)).sum(-1)
    status = np.zeros(p.shape[:-2], np.int64)

    def fail(cond, code):
        status[(status == 0) & cond] = code
    fail(((p < valid_min) | (p > valid_max)).any((-1, -2)), NODATA)
    fail(sD == 0, FLAT)
    fail((S0 < contrast_min).any(-1), LOWCONTRAST)
    fail(((4 * TV > 5 * S0 + 4 * tv_slack) | (S1 < 0)).any(-1), TEXTURED)
    live = (status == 0)[..., None]
    c = np.where(live, 64 * S1 // np.where(live, S0, 1), 0)
    fail(((c < 1280) | (c > 2688)).any(-1), OFFCENTRE)
    Sc = c.sum(-1)
    Num = 32 * (c * _R).sum(-1) - 496 * Sc
    fail(~((4 * DEN <= np.abs(Num)) & (np.abs(Num) <= 32 * DEN)), SLANT)
    f = (2 * DEN * Sc[..., None] + 32 * Num[..., None] * (2 * _R - 31)) // (64 * DEN)
    fail((np.abs(c - f) > 64).any(-1), CURVED)
    ok = status == 0
    rec = np.stack([status, np.where(ok, s, 0), np.where(ok, Sc, 0), np.where(ok, Num, 0)], -1).astype(np.int32)
    return rec, f, S0.sum(-1)


def planes(img, spp):
    img = np.asarray(img)
    return [img[:, c::spp] for c in range(spp)]


def records(img, spp, axis, **kw):
    """(spp, nty, ntx, 4) int32: what oip_mtf_tiles_u16 writes for the (rows, w * spp) raster img"""
    return np.stack([analyse(tiles(pl, axis), **kw)[0] for pl in planes(img, spp)])


def esf_of_tile(p, **kw):
    """(128,) uint32: 64 sums then 64 counts; all zero unless the tile's status is 0"""
    rec, f, _ = analyse(p, **kw)
    out = np.zeros(128, np.int64)
    if rec[0] == 0:
        u = 128 * _R[None, :] - f[:, None]
        b = (u + 1024) >> 5
        m = (b >= 0) & (b < 64)
        np.add.at(out, b[m], np.asarray(p, dtype=np.int64)[m])
        np.add.at(out, 64 + b[m], 1)
    return out.astype(np.uint32)


def esf(img, spp, axis, entries, **kw):
    """(n, 128) uint32 for entries (channel, ty, tx): what oip_mtf_esf_u16 writes"""
    pl = planes(img, spp)
    tl = {}
    out = np.zeros((len(entries), 128), np.uint32)
    for k, (c, ty, tx) in enumerate(entries):
        if c not in tl:
            tl[c] = tiles(pl[c], axis)
        out[k] = esf_of_tile(tl[c][ty, tx], **kw)
    return out


def ok_list(rec):
    """the status-0 tiles of records (spp, nty, ntx, 4) in (channel, ty, tx) order, (n, 3) int32"""
    return np.argwhere(rec[..., 0] == 0).astype(np.int32).reshape(-1, 3)


_Q = math.sin(math.pi / 8.0) / (math.pi / 8.0)
_H = 0.70710678118654752
C8 = (1.0, _H, 0.0, -_H, -1.0, -_H, 0.0, _H)
S8 = (0.0, _H, 1.0, _H, 0.0, -_H, -1.0, -_H)
WINDOW = tuple(0.54 - 0.46 * math.cos(2.0 * math.pi * float(j) / 62.0) for j in range(63))


def tile_mtf(s, sums, cnts):
    """the MTF at Nyquist of one tile from its polarity and its 64 sums and counts, or None (EMPTYBIN)"""
    if any(int(c) == 0 for c in cnts):
        return None
    E = [float(s) * float(int(a)) / float(int(c)) for a, c in zip(sums, cnts)]
    A0 = Re = Im = 0.0
    for j in range(63):
        t = WINDOW[j] * (E[j + 1] - E[j])
        k = (j - 31) % 8
        A0 += t
        Re += t * C8[k]
        Im += t * S8[k]
    if not A0 > 0.0:
        return None
    return math.hypot(Re, Im) / A0 / (_Q * _Q)


def summary(values):
    """(median, p75, p90) of a non-empty list by the integer indices of include/oip_c.h"""
    v = sorted(float(x) for x in values)
    n = len(v)
    return v[(n - 1) // 2], v[3 * (n - 1) // 4], v[9 * (n - 1) // 10]


def tv_slack(sigma_ref):
    return int(min(65535.0, math.ceil(48.0 * sigma_ref)))


def analytic(sigma):
    """MTF at Nyquist of a Gaussian blur of sigma samples and the pixel box"""
    return math.exp(-2.0 * (math.pi * sigma / 2.0) ** 2) * 2.0 / math.pi


_erf = np.vectorize(math.erf, otypes=[float])


def _box_edge(x, sigma):
    """the unit edge blurred by a Gaussian of sigma, integrated over the pixel [x - 0.5, x + 0.5]"""
    def G(z):                                                          # the integral of the normal CDF
        return z * 0.5 * (1.0 + _erf(z / math.sqrt(2.0))) + np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    return sigma * (G((x + 0.5) / sigma) - G((x - 0.5) / sigma))


def edge_tile(sigma, centre, slant, polarity, contrast=2000.0, base=1000.0, noise=0.0, rng=None, bend=0.0):
    """(32 profiles, 32 samples) uint16: an edge that crosses `slant` samples over the 32 profiles, at `centre` half-way down,
    bent by `bend` samples at either end"""
    r, i = np.meshgrid(np.arange(32.0), np.arange(32.0), indexing="ij")
    x0 = centre + slant * (r - 15.5) / 32.0 + bend * ((r - 15.5) / 15.5) ** 2
    e = _box_edge(i - x0, sigma)
    v = base + contrast * (e if polarity > 0 else 1.0 - e)
    if noise:
        v = v + rng.normal(0.0, noise, v.shape)
    return np.clip(np.rint(v), 0, 65535).astype(np.uint16)


def planted(sigma, n, seed, noise=5.0):
    """n planted tiles (n, 32, 32): slant 1.2 to 7 samples either way, both polarities, centres up to 4 samples off the middle
    (those far off with a large slant leave the centring window and are OFFCENTRE)"""
    rng = np.random.default_rng(seed)
    out = np.empty((n, 32, 32), np.uint16)
    for k in range(n):
        slant = rng.uniform(1.2, 7.0) * rng.choice((-1.0, 1.0))
        out[k] = edge_tile(sigma, 15.5 + rng.uniform(-4.0, 4.0), slant, rng.choice((-1, 1)), noise=noise, rng=rng)
    return out


def empty_value_tile(slant=3.0, centre=15.5):
    """a tile that passes every integer test at a slack of 3100 or more and has A0 <= 0: a fall of 2000 DN on the edge between two
    rises of 3000 DN six samples to either side, where the window weighs them 0.19"""
    r, i = np.meshgrid(np.arange(32.0), np.arange(32.0), indexing="ij")
    x = i - (centre + slant * (r - 15.5) / 32.0)
    step = lambda z: np.clip(z + 0.5, 0.0, 1.0)                        # noqa: E731  the pixel box over a unit step
    return np.rint(1000.0 + 3000.0 * step(x + 6.0) - 2000.0 * step(x) + 3000.0 * step(x - 6.0)).astype(np.uint16)


FIELD_SLACK = 3200                                                     # the slack at which empty_value_tile passes the integer tests
KINDS = ("rise", "fall", "nodata", "flat", "lowcontrast", "textured", "offcentre", "upright", "steep", "curved", "emptyvalue", "noise")


def field_cell(kind, rng):
    """one 32 x 32 cell (profiles x samples) that is meant to end in the status its kind names at a slack of FIELD_SLACK"""
    slant = float(rng.uniform(1.5, 6.0) * rng.choice((-1.0, 1.0)))
    centre = 15.5 + float(rng.uniform(-2.0, 2.0))
    pol = 1 if kind == "rise" else -1 if kind == "fall" else int(rng.choice((-1, 1)))
    kw = dict(noise=3.0, rng=rng)
    if kind == "flat":
        return np.full((32, 32), int(rng.integers(100, 4000)), np.uint16)
    if kind == "noise":
        return rng.integers(1, 4096, (32, 32)).astype(np.uint16)
    if kind == "emptyvalue":
        return empty_value_tile(slant, centre)
    if kind == "lowcontrast":
        return edge_tile(0.5, centre, slant, pol, contrast=120.0, **kw)
    if kind == "textured":
        return edge_tile(0.5, centre, slant, pol, noise=300.0, rng=rng)
    if kind == "offcentre":
        return edge_tile(0.5, 5.0, slant, pol, **kw)
    if kind == "upright":
        return edge_tile(0.5, centre, 0.0, pol, **kw)
    if kind == "steep":
        return edge_tile(0.5, 15.5, 11.0, pol, **kw)
    if kind == "curved":
        return edge_tile(0.5, centre - 0.5, 3.0, pol, bend=1.6, **kw)
    t = edge_tile(0.5, centre, slant, pol, **kw)
    if kind == "nodata":
        t[int(rng.integers(0, 32)), int(rng.integers(0, 32))] = 0 if rng.random() < 0.5 else 65535
    return t


def field(rows, w, axis, seed, spp=1):
    """(rows, w * spp) uint16: 32 x 32 cells of every kind on the tile grid of the axis, another draw for every channel"""
    out = np.empty((rows, w * spp), np.uint16)
    for c in range(spp):
        rng = np.random.default_rng(1000 * seed + c)
        pl = rng.integers(900, 1100, (rows, w)).astype(np.uint16)
        k = int(rng.integers(0, len(KINDS)))
        for j in range(0, rows - 31, 32):
            for i in range(0, w - 31, 32):
                cell = field_cell(KINDS[k % len(KINDS)], rng)
                pl[j:j + 32, i:i + 32] = cell if axis == 0 else cell.T
                k += 1 + int(rng.integers(0, 2))
        out[:, c::spp] = pl
    return out


def _group_line(head, axis, tiles, status, emptybin, values):
    s = "%s axis %s: tiles %d ok %d nodata %d flat %d lowcontrast %d textured %d offcentre %d slant %d curved %d emptybin %d values %d" % (
        (head, "xy"[axis], tiles) + tuple(int(v) for v in status) + (emptybin, len(values)))
    if values:
        s += " median %.17g p75 %.17g p90 %.17g" % summary(values)
    return s


def report_body(img, spp, axes, slacks, tile_value=tile_mtf, **kw):
    """the lines of <stem>.MTF.CSV behind its first one, for the (rows, w * spp) raster img: axes a sequence of 0 / 1, slacks the
    tv_slack of every band; tile_value: the host step (the restatement's, or the library's, which test_mtf_cpu.py holds to it)"""
    rows, bands, pooled = [], [], {a: [0, np.zeros(8, np.int64), 0, []] for a in axes}
    pl = planes(img, spp)
    for c in range(spp):
        for a in axes:
            p = dict(kw, tv_slack=slacks[c])
            tl = tiles(pl[c], a)
            rec, _, s0 = analyse(tl, **p)
            status = np.bincount(rec[..., 0].ravel(), minlength=8)
            values, empty = [], 0
            for ty, tx in np.argwhere(rec[..., 0] == 0):
                e = esf_of_tile(tl[ty, tx], **p)
                m = tile_value(int(rec[ty, tx, 1]), e[:64], e[64:])
                if m is None:
                    empty += 1
                    continue
                values.append(m)
                rows.append("%d,%s,%d,%d,%d,%d,%.5f,%.17g" % (c + 1, "xy"[a], ty, tx, rec[ty, tx, 1], rec[ty, tx, 3], s0[ty, tx] / 32.0, m))
            bands.append(_group_line("band %d" % (c + 1), a, rec[..., 0].size, status, empty, values))
            g = pooled[a]
            g[0] += rec[..., 0].size
            g[1] += status
            g[2] += empty
            g[3] += values
    return rows + ["# " + b for b in bands] + ["# " + _group_line("all", a, *pooled[a]) for a in axes]
