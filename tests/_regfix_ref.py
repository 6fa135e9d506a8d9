"""The definition of `oip regfix` (include/oip_c.h: oip_warp_grid_bicubic_u16, oip_warp_grid_src_range, oip_regfix_load_report,
oip_regfix_fill, oip_regfix_smooth) restated in numpy with int64 arithmetic; the 16-tap sum is the oracle's
(oracle.remap_cubic: cv::remap(INTER_CUBIC, BORDER_CONSTANT 0)).  No GPU library is imported.

A lattice of nx x ny nodes at pixel (gx0 + i sx, gy0 + j sy) carries NX and NY, int Q10.  Per axis
    p = x - gx0;  ci = clamp(floor(p / sx), 0, nx - 2);  t = clamp(p - ci sx, 0, sx);  wx = (t 4096 + sx / 2) / sx
(one node: ci = 0, wx = 0), lerp(a, b, w) = a + (((b - a) w + 2048) >> 12), and per output sample, y first, then x,
    R[i] = lerp(N[cj][i], N[cj + 1][i], wy);  d = lerp(R[ci], R[ci + 1], wx);  s = 32 coordinate + ((d + 16) >> 5)
in 1/32 px.  out(y, x) = src(y + dy, x + dx): regcheck's convention."""
import numpy as np

import oracle

MAX_Q10 = 65536
MAX_STEP = 65536


def axis(first, count, g0, step, n):
    """(cell, Q12 weight) of the coordinates first .. first + count - 1, int64"""
    p = np.arange(first, first + count, dtype=np.int64) - g0
    if n == 1:
        return np.zeros(count, np.int64), np.zeros(count, np.int64)
    c = np.clip(p // step, 0, n - 2)
    t = np.clip(p - c * step, 0, step)
    return c, (t * 4096 + step // 2) // step


def lerp(a, b, w):
    return a + (((b - a) * w + 2048) >> 12)


def positions(NX, NY, W, gx0, gy0, sx, sy, row0, rows):
    """(s_x, s_y), (rows, W) int64 in 1/32 px, of output lines [row0, row0 + rows)"""
    NX, NY = np.asarray(NX, np.int64), np.asarray(NY, np.int64)
    ny, nx = NX.shape
    assert NY.shape == NX.shape and 1 <= sx <= MAX_STEP and 1 <= sy <= MAX_STEP
    assert np.abs(NX).max() <= MAX_Q10 and np.abs(NY).max() <= MAX_Q10
    cj, wy = axis(row0, rows, gy0, sy, ny)
    ci, wx = axis(0, W, gx0, sx, nx)
    cj1, ci1 = np.minimum(cj + 1, ny - 1), np.minimum(ci + 1, nx - 1)       # (never read where it matters: the weight is 0)
    out = []
    for N, coord in ((NX, np.arange(W, dtype=np.int64)[None, :]), (NY, np.arange(row0, row0 + rows, dtype=np.int64)[:, None])):
        R = lerp(N[cj], N[cj1], wy[:, None])
        d = lerp(R[:, ci], R[:, ci1], wx[None, :])
        out.append(32 * coord + ((d + 16) >> 5))
    return out[0], out[1]


def tap_lines(NY, W, gx0, gy0, sx, sy, row0, rows):
    """(lowest, highest) source line that output lines [row0, row0 + rows) tap, before any clamp to the raster"""
    _, s_y = positions(np.zeros_like(np.asarray(NY)), NY, W, gx0, gy0, sx, sy, row0, rows)
    return int((s_y >> 5).min()) - 1, int((s_y >> 5).max()) + 2


def warp(src, NX, NY, gx0, gy0, sx, sy, band_mask=None, row0=0, L=None, out_row0=None, out_rows=None):
    """src: lines [row0, row0 + src.shape[0]) of a raster of L lines (default: all of it), (lines, W) or (lines, W, spp).
    Returns output lines [out_row0, out_row0 + out_rows) (default: src's own lines).  Every line of the raster that they tap
    must be in src: asserted."""
    src = np.asarray(src)
    planar = src.ndim == 2
    img = src.reshape(src.shape[0], src.shape[1], -1)
    lines, W, spp = img.shape
    L = row0 + lines if L is None else L
    out_row0 = row0 if out_row0 is None else out_row0
    out_rows = lines if out_rows is None else out_rows
    band_mask = (1 << spp) - 1 if band_mask is None else band_mask
    assert row0 >= 0 and row0 + lines <= L and out_row0 >= 0 and out_row0 + out_rows <= L and 1 <= band_mask < (1 << spp)
    s_x, s_y = positions(NX, NY, W, gx0, gy0, sx, sy, out_row0, out_rows)
    lo, hi = int((s_y >> 5).min()) - 1, int((s_y >> 5).max()) + 2
    need_lo, need_hi = max(lo, 0), min(hi, L - 1)                # lines outside [0, L) are the constant border
    if need_lo <= need_hi:
        assert row0 <= need_lo and need_hi < row0 + lines, "src lacks tapped lines"
    s_yl = s_y - 32 * row0                                       # in src's own lines
    # the maps s / 32 are exact in f32 below 2^19 px, and the oracle's `short` clamp of coordinates never acts
    for s in (s_x, s_yl):
        assert (s >> 5).max() < 32767 and (s >> 5).min() > -32767 and np.abs(s).max() < (1 << 24)
    mapx, mapy = (s_x / 32.0).astype(np.float32), (s_yl / 32.0).astype(np.float32)
    assert np.array_equal(np.rint(mapx.astype(np.float64) * 32).astype(np.int64), s_x)
    assert np.array_equal(np.rint(mapy.astype(np.float64) * 32).astype(np.int64), s_yl)
    out = np.empty((out_rows, W, spp), np.uint16)
    for c in range(spp):
        if band_mask & (1 << c):
            out[:, :, c] = oracle.remap_cubic(np.ascontiguousarray(img[:, :, c]), mapx, mapy)
        else:
            assert out_row0 >= row0 and out_row0 + out_rows <= row0 + lines
            out[:, :, c] = img[out_row0 - row0:out_row0 - row0 + out_rows, :, c]
    return out[:, :, 0] if planar else out


# ---- the field of a regcheck report ------------------------------------------------------------------------------------------
def fill(NX, NY, is_set):
    """in passes, an unset node with k >= 1 set 4-neighbours (as of the pass's start) gets floor((2 sum + k) / (2 k))"""
    X, Y, m = np.array(NX, np.int64), np.array(NY, np.int64), np.array(is_set, bool)
    if not m.any():
        raise ValueError("no node is set")
    while not m.all():
        k = np.zeros(m.shape, np.int64)
        sx, sy = np.zeros(m.shape, np.int64), np.zeros(m.shape, np.int64)
        for sl_to, sl_from in (((slice(None), slice(1, None)), (slice(None), slice(None, -1))),
                               ((slice(None), slice(None, -1)), (slice(None), slice(1, None))),
                               ((slice(1, None), slice(None)), (slice(None, -1), slice(None))),
                               ((slice(None, -1), slice(None)), (slice(1, None), slice(None)))):
            k[sl_to] += m[sl_from]
            sx[sl_to] += np.where(m[sl_from], X[sl_from], 0)
            sy[sl_to] += np.where(m[sl_from], Y[sl_from], 0)
        new = ~m & (k > 0)
        kk = np.maximum(k, 1)
        X = np.where(new, (2 * sx + k) // (2 * kk), X)           # numpy's // floors
        Y = np.where(new, (2 * sy + k) // (2 * kk), Y)
        m = m | new
    return X.astype(np.int32), Y.astype(np.int32)


def smooth(N, passes):
    """`passes` times [1 2 1] along the node lines, then across them, replicated edges: (a + 2 b + c + 2) >> 2"""
    N = np.array(N, np.int64)
    for _ in range(passes):
        p = np.pad(N, ((0, 0), (1, 1)), mode="edge")
        N = (p[:, :-2] + 2 * p[:, 1:-1] + p[:, 2:] + 2) >> 2
        p = np.pad(N, ((1, 1), (0, 0)), mode="edge")
        N = (p[:-2] + 2 * p[1:-1] + p[2:] + 2) >> 2
    return N.astype(np.int32)


def parse_report(text, w=0, h=0, smooth_passes=0):
    """-> (NX, NY (ny, nx) int32, dict(gx0, gy0, sx, sy, band2, used)); ValueError for a report the tool refuses"""
    lines = text.split("\n")
    if not lines[0].startswith("# oip regcheck "):
        raise ValueError("first line")
    def key(name, limit):
        toks = [t for t in lines[0].rstrip("\r").split(" ")[1:] if t.startswith(name + "=")]
        if not toks:
            raise ValueError("the header lacks " + name)
        v = int(toks[-1][len(name) + 1:])
        if abs(v) > limit:
            raise ValueError(name)
        return v
    scale, shx, shy, band2 = key("scale", 64), key("shift-x", 1 << 40), key("shift-y", 1 << 40), key("band2", 4)
    if scale < 1 or band2 < 1:
        raise ValueError("scale / band2")
    tiles = []
    for ln in lines[1:]:
        ln = ln.rstrip("\r")
        if not ln or ln.startswith("#"):
            continue
        t = ln.split(",")
        if len(t) != 6:
            raise ValueError("tile line")
        x, y, fl = int(t[0]), int(t[1]), int(t[5])
        dx, dy, sc = float(t[2]), float(t[3]), float(t[4])
        if not (np.isfinite(dx) and np.isfinite(dy) and np.isfinite(sc)) or x < 0 or y < 0 or not 0 <= fl <= 15 or x % scale or y % scale:
            raise ValueError("tile value")
        tiles.append((x, y, dx, dy, fl))
    if not tiles:
        raise ValueError("no tile")
    n = len(tiles)
    nx = 1
    while nx < n and tiles[nx][1] == tiles[0][1]:
        nx += 1
    if n % nx:
        raise ValueError("ragged")
    ny = n // nx
    stx = tiles[1][0] - tiles[0][0] if nx > 1 else scale
    sty = tiles[nx][1] - tiles[0][1] if ny > 1 else scale
    if stx <= 0 or sty <= 0:
        raise ValueError("order")
    for q, t in enumerate(tiles):
        if t[0] != tiles[0][0] + (q % nx) * stx or t[1] != tiles[0][1] + (q // nx) * sty:
            raise ValueError("irregular")
    g = dict(gx0=tiles[0][0] // scale - shx, gy0=tiles[0][1] // scale - shy, sx=stx // scale, sy=sty // scale, band2=band2,
             used=sum(t[4] == 0 for t in tiles))
    if g["sx"] > MAX_STEP or g["sy"] > MAX_STEP:
        raise ValueError("step")
    if w > 0 and h > 0 and (g["gx0"] < 0 or g["gy0"] < 0 or g["gx0"] + (nx - 1) * g["sx"] >= w or g["gy0"] + (ny - 1) * g["sy"] >= h):
        raise ValueError("node outside the image")
    d = np.array([(t[2], t[3]) for t in tiles], np.float64).reshape(ny, nx, 2)
    ok = np.array([t[4] == 0 for t in tiles]).reshape(ny, nx)
    if (np.abs(d[ok]) > 64.0).any():
        raise ValueError("above 64 px")
    q = np.where(ok[..., None], np.rint(d * 1024.0), 0.0).astype(np.int64)
    NX, NY = fill(q[..., 0], q[..., 1], ok)
    return smooth(NX, smooth_passes), smooth(NY, smooth_passes), g


def report_text(dx, dy, score, flags, x0, y0, step, T, scale=1, shift=(0, 0), band2=1, origin=(0, 0)):
    """the report `oip regcheck` writes for (ny, nx) tiles (csrc/oip_regreport.hpp: WriteRegReport), without its summary lines"""
    ny, nx = np.asarray(dx).shape
    out = ["# oip regcheck image1=A image2=B band1=1 band2=%d scale=%d shift-x=%d shift-y=%d tile=%d columns=x,y,dx,dy,score,flags"
           % (band2, scale, shift[0], shift[1], T)]
    for j in range(ny):
        for i in range(nx):
            out.append("%d,%d,%.4f,%.4f,%.6f,%d" % ((origin[0] + x0 + i * step + T // 2) * scale, (origin[1] + y0 + j * step + T // 2) * scale,
                                                    dx[j][i], dy[j][i], score[j][i], flags[j][i]))
    return "\n".join(out) + "\n# summary\n"
