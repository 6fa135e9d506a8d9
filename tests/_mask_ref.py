"""numpy restatement of the mask (include/oip_c.h, section "mask"): the flag byte of every cell, the opening and the buffer on
the grid of cells, the eight counters and oip_mask_tile_flag -- written from the text of the header, not from the kernels.  Cells
by padded reshape and sum, morphology by brute force over the (2r+1)^2 offsets.  No GPU library is imported."""
import itertools

import numpy as np

NODATA, SATURATED, CLOUD, BUFFER, CANDIDATE = 1, 2, 4, 8, 16
DEFAULT_Q8 = (77, 38, 20, 51)                                          # rint(256 * (0.30, 0.15, 0.08, 0.20))
DEFAULT_BAND = (2, 1, 0, 3)                                            # the product's R, G, B, alpha order: blue is channel 2


def grid(w, h, C):
    return -(-w // C), -(-h // C)


def _cell_sums(a, C):
    """(h, w) -> (gh, gw) sums over the cells, int64; partial cells at the right and bottom edge sum what they hold"""
    h, w = a.shape
    gw, gh = grid(w, h, C)
    p = np.zeros((gh * C, gw * C), np.int64)
    p[:h, :w] = a
    return p.reshape(gh, C, gw, C).sum(axis=(1, 3))


def cells(img, spp, C, valid_min=1, sat_level=4095, full=4095, band=DEFAULT_BAND, q8=DEFAULT_Q8):
    """img: (rows, w * spp) uint16.  Returns (flags (gh, gw) uint8, counts (8,) uint64 as oip_mask_cells_u16 adds them)"""
    assert C in (4, 8, 16) and spp in (1, 4)
    rows = img.shape[0]
    px = np.asarray(img).reshape(rows, -1, spp).astype(np.int64)
    w = px.shape[1]
    nd = (px < valid_min).any(axis=2)
    sat = ~nd & (px >= sat_level).any(axis=2)
    good = ~nd & ~sat
    m, n_nd, n_sat = _cell_sums(good, C), _cell_sums(nd, C), _cell_sums(sat, C)
    n_cell = _cell_sums(np.ones((rows, w), np.int64), C)
    flags = np.where(n_nd > 0, NODATA, 0) | np.where(n_sat > 0, SATURATED, 0)
    tested = np.zeros(m.shape, bool)
    if spp == 4:
        assert sorted(band) == [0, 1, 2, 3]
        b, g, r, n = [_cell_sums(np.where(good, px[:, :, band[k]], 0), C) for k in range(4)]
        V = b + g + r
        mx, mn = np.maximum(np.maximum(b, g), r), np.minimum(np.minimum(b, g), r)
        tested = (2 * m >= n_cell) & (m >= 1)
        ok = tested.copy()
        if q8[0] >= 0:
            ok &= 256 * V >= 3 * m * full * q8[0]
        if q8[1] >= 0:
            ok &= 768 * (mx - mn) <= q8[1] * V
        if q8[2] >= 0:
            ok &= 256 * (2 * b - r) >= 2 * m * full * q8[2]
        if q8[3] >= 0:
            ok &= 256 * (n - r) <= q8[3] * (n + r)
        flags = flags | np.where(ok, CANDIDATE, 0)
    flags = flags.astype(np.uint8)
    counts = np.zeros(8, np.uint64)
    counts[0] = flags.size
    counts[1] = int((flags & NODATA != 0).sum())
    counts[2] = int((flags & SATURATED != 0).sum())
    counts[3] = int(tested.sum())
    counts[4] = int((flags & CANDIDATE != 0).sum())
    counts[7] = int(sat.sum())
    return flags, counts


def _square(x, r, erode):
    """AND (erode: what lies outside the grid does not constrain) or OR of x over the (2r+1)^2 offsets"""
    gh, gw = x.shape
    p = np.full((gh + 2 * r, gw + 2 * r), erode, bool)
    p[r:r + gh, r:r + gw] = x
    out = np.full(x.shape, erode, bool)
    for j in range(2 * r + 1):
        for i in range(2 * r + 1):
            s = p[j:j + gh, i:i + gw]
            out = out & s if erode else out | s
    return out


def opening(x, a):
    return _square(_square(x, a, True), a, False)


def morph(flags, a, d):
    """(flags with bits 4 and 8 rewritten, (CLOUD cells, BUFFER cells)) as oip_mask_morph_u8 leaves them"""
    assert 0 <= a <= 32 and 0 <= d <= 64
    f = np.asarray(flags, np.uint8)
    O = opening(f & CANDIDATE != 0, a)
    D = _square(O, d, False)
    out = (f & ~np.uint8(CLOUD | BUFFER)) | np.where(O, CLOUD, 0).astype(np.uint8) | np.where(D & ~O, BUFFER, 0).astype(np.uint8)
    return out, (int(O.sum()), int((D & ~O).sum()))


def mask(img, spp, C, a=1, d=2, **kw):
    """cells, then morph: (flags, the eight counters)"""
    f, counts = cells(img, spp, C, **kw)
    f, (n_cloud, n_buffer) = morph(f, a, d)
    counts[5], counts[6] = n_cloud, n_buffer
    return f, counts


def recount(flags):
    """the counters that can be counted from the flag bytes alone: indices 0, 1, 2, 4, 5, 6"""
    f = np.asarray(flags)
    return {0: f.size, 1: int((f & NODATA != 0).sum()), 2: int((f & SATURATED != 0).sum()), 4: int((f & CANDIDATE != 0).sum()),
            5: int((f & CLOUD != 0).sum()), 6: int((f & BUFFER != 0).sum())}


def tile_flag(flags, C, x, y, tw, th, bits):
    """whether a cell that intersects the pixel rectangle [x, x + tw) x [y, y + th) has a bit of `bits` set"""
    gh, gw = flags.shape
    for j in range(gh):
        for i in range(gw):
            if flags[j, i] & bits and max(x, i * C) < min(x + tw, i * C + C) and max(y, j * C) < min(y + th, j * C + C):
                return True
    return False


# ---- the scene of the ground-truth tests --------------------------------------------------------------------------------------
FULL10 = 1023
GROUND = ((.04, .07, .05, .45), (.12, .16, .22, .30), (.07, .06, .04, .02))      # vegetation, soil, water as (B, G, R, N)
ROOF = (.45, .47, .48, .50)
CLOUD_REFL = (.62, .60, .59, .58)
SCENE_BAND = (0, 1, 2, 3)                                              # the scene's channels are (B, G, R, N)


def scene(h, w, seed):
    """((h, w, 4) uint16 in (B, G, R, N) channel order, 10-bit; (h, w) bool: the cloud pixels; (h, w) bool: the roof pixels
    that no cloud covers).  64 x 64 blocks of three ground classes, forty 12 x 12 roofs, five discs of cloud of radius 40..89
    laid last, all multiplied by 1 + 0.05 N(0, 1) per sample; DN = clip(rint(refl * 1023) + 1, 1, 1023)"""
    rng = np.random.default_rng(seed)
    refl = np.zeros((h, w, 4))
    cls = rng.integers(0, 3, (-(-h // 64), -(-w // 64)))
    for j in range(cls.shape[0]):
        for i in range(cls.shape[1]):
            refl[j * 64:(j + 1) * 64, i * 64:(i + 1) * 64] = GROUND[cls[j, i]]
    roof = np.zeros((h, w), bool)
    for _ in range(40):
        y, x = int(rng.integers(0, h - 12)), int(rng.integers(0, w - 12))
        refl[y:y + 12, x:x + 12] = ROOF
        roof[y:y + 12, x:x + 12] = True
    cloud = np.zeros((h, w), bool)
    yy, xx = np.mgrid[0:h, 0:w]
    for _ in range(5):
        cy, cx, r = int(rng.integers(0, h)), int(rng.integers(0, w)), int(rng.integers(40, 90))
        cloud |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    refl[cloud] = CLOUD_REFL
    refl = refl * (1 + 0.05 * rng.standard_normal(refl.shape))
    dn = np.clip(np.rint(refl * FULL10) + 1, 1, FULL10).astype(np.uint16)
    return dn, cloud, roof & ~cloud


# ---- rasters of the kernel tests -----------------------------------------------------------------------------------------------
def random_raster(rows, ws, seed, full=4095):
    """(rows, ws) samples: full-range random with 3 % zeros and 1 % saturated samples"""
    rng = np.random.default_rng(seed)
    img = rng.integers(1, full, (rows, ws)).astype(np.uint16)
    u = rng.random(img.shape)
    img[u < 0.03] = 0
    img[u > 0.99] = full
    return img


def _flat_cell(C, sums):
    """(C, C, 4) samples >= 1 whose channel sums are `sums`: the quotient everywhere, the remainder spread one by one"""
    out = np.zeros((C, C, 4), np.int64)
    n = C * C
    for c, s in enumerate(sums):
        assert n <= s <= n * 60000, (c, s)
        v = np.full(n, s // n, np.int64)
        v[:s % n] += 1
        out[:, :, c] = v.reshape(C, C)
    return out.astype(np.uint16)


EDGE_FULL, EDGE_Q8 = 4096, (77, 38, 38, 51)
# The crafted cells use full_scale 4096 and these parameters.  m * 4096 is a multiple of 256, so 3 m full q / 256 and 2 m full q / 256 are
# whole and equality exists for the bright and the haze test.  hot_q8 is 38 and not the default 20: for a given spectral shape
# the bright and the haze threshold both scale with the level, so the two can only be decided alone, each with the other passed
# with room, if the cell at the bright edge is bluish (b = 1.1 r) and the cell at the haze edge is reddish (b = 0.9 r), which
# needs 0.42 bright_q8 <= hot_q8 <= 0.58 bright_q8 (white allows |b - r| <= 0.148 r).


def margins(sums, m, full, q8):
    """the four tests as numbers that pass iff >= 0, in Python integers"""
    b, g, r, n = [int(v) for v in sums]
    V = b + g + r
    return (256 * V - 3 * m * full * q8[0], q8[1] * V - 768 * (max(b, g, r) - min(b, g, r)), 256 * (2 * b - r) - 2 * m * full * q8[2],
            q8[3] * (n + r) - 256 * (n - r))


def edge_cases(C, full=EDGE_FULL, q8=EDGE_Q8):
    """[(test index, k, (b, g, r, n))]: channel sums of whole cells of m = C * C good pixels; at k = 0 test `index` is at
    equality (margin 0), at k = -1 and +1 one sum is moved by one so that it fails and passes; the other three tests pass with
    room in all three.  test_mask_cpu.py asserts exactly that of margins()."""
    m = C * C
    T = m * full
    assert (3 * T * q8[0]) % 256 == 0 and (2 * T * q8[2]) % 256 == 0
    V0, H0 = 3 * T * q8[0] // 256, 2 * T * q8[2] // 256
    out = []
    r = V0 * 10 // 31                                                  # bright: b = 1.1 r, g = r, V = V0 + k
    for k in (-1, 0, 1):
        out.append((0, k, (V0 + k - 2 * r, r, r, r)))
    t = -(-13 * V0 // (10 * 1152))                                     # white: (768 - q1) (b - r) = 3 q1 r: r = 365 t, b = 422 t at q1 = 38
    assert q8[1] == 38
    for k in (-1, 0, 1):
        out.append((1, k, (422 * t - k, 365 * t, 365 * t, 365 * t)))
    r = H0 * 10 // 8                                                   # haze: b = 0.9 r, 2 b - r = H0 + k through r
    r += (H0 + r) % 2
    for k in (-1, 0, 1):
        out.append((2, k, ((H0 + r) // 2, r, r - k, r - k)))
    t = -(-13 * V0 // (10 * 615))                                      # ndvi: (256 - q3) n = (256 + q3) r: r = 205 t, n = 307 t at q3 = 51
    assert q8[3] == 51
    for k in (-1, 0, 1):
        out.append((3, k, (205 * t, 205 * t, 205 * t, 307 * t - k)))
    return out


def edge_raster(C, full=EDGE_FULL, q8=EDGE_Q8, band=DEFAULT_BAND):
    """one cell line: the cells of edge_cases next to each other, (C, ncells * C * 4) uint16, channels placed by `band`"""
    cases = edge_cases(C, full, q8)
    img = np.zeros((C, len(cases) * C, 4), np.uint16)
    for i, (_, _, sums) in enumerate(cases):
        cell = _flat_cell(C, sums)
        for k in range(4):
            img[:, i * C:(i + 1) * C, band[k]] = cell[:, :, k]
    return img.reshape(C, -1), cases


def all_switches(q8=DEFAULT_Q8):
    """every combination of enabled / disabled tests as q8 tuples, all enabled first"""
    return [tuple(q if on else -1 for q, on in zip(q8, ons)) for ons in itertools.product((True, False), repeat=4)]


def flag_grid(gh, gw, density, seed):
    """flag bytes for the morphology: bit 16 at `density`, solid rectangles that an opening keeps (one across the border of a
    64-cell word), and bits 1, 2 and stale bits 4, 8 sprinkled over them"""
    rng = np.random.default_rng(seed)
    x = rng.random((gh, gw)) < density
    if 0 < density < 1:
        x[gh // 4:gh // 4 + 9, max(0, min(gw, 70) - 20):min(gw, 70)] = True
        x[gh // 2:gh // 2 + 5, :5] = True
    f = np.where(x, CANDIDATE, 0).astype(np.uint8)
    return f | rng.integers(0, 16, (gh, gw)).astype(np.uint8)
