"""Helpers of the tests that hand the kernels addresses past 2^31 elements (test_gpu_beyond_2g.py) and of the host test that
shows those checks bite (test_bigraster_cpu.py).  No GPU library is imported at module level: torch is looked up only when a
function is handed a tensor.

The probe raster: every line holds one valid constant, except a head band and a tail band of seeded noise.  An operation with a
vertical footprint of `halo` lines maps it onto: inside each band widened by halo, what the CPU restatement gives for the band
with 2 * halo constant lines around it; on every other line, the image of the constant (one row vector).  The two checks
together cover every output element and neither needs more than the bands on the host."""
import numpy as np

TWO31 = 1 << 31
CONST = 1500


class Geometry:
    """lines of `width` samples; head = [0, head), tail = [tail0, lines); `wrap` is the element index a 32-bit offset cannot
    reach (2^31 on the device, a small number in the host model)"""

    def __init__(self, width, lines, head, tail0, wrap=TWO31):
        self.W, self.L, self.head, self.tail, self.wrap = width, lines, (0, head), (tail0, lines), wrap
        assert head < tail0 < lines

    @property
    def first_line_beyond(self):
        """first line that starts at or past `wrap`"""
        return -(-self.wrap // self.W)

    def assert_crosses(self):
        """the geometry does what it is for: the tail band holds lines that lie wholly past `wrap`, all of them inside the
        raster, and the wrapped images of those lines meet the head band"""
        f = self.first_line_beyond
        assert self.tail[0] < f < self.L, (self.tail, f, self.L)
        assert (f * self.W - self.wrap) // self.W < self.head[1]
        return f


# W = 32760: the largest multiple of 8 under the 32767-column limit of the resampler; 65600 lines: 2 149 056 000 samples.
# 65552 * 32760 = 2^31 - 128: line 65552 straddles 2^31, lines 65553 .. 65599 lie wholly beyond it.
BIG = Geometry(32760, 65600, 24, 65520)
# the same band layout at a size the host affords: line 192 straddles `wrap`, lines 193 .. 239 lie beyond it (47, as in BIG)
SMALL = Geometry(64, 240, 24, 160, wrap=192 * 64 + 8)


def band_noise(geo, k, seed, lo=300, hi=3801, specials=(0, 65535), rate=0.02, impulses=0):
    """noise of band k (0 head, 1 tail): dense uniform values in [lo, hi) -- so that two bands, or a band and the constant, differ
    nearly everywhere --, a share `rate` of each of `specials`, and `impulses` isolated samples 20000 above their surroundings"""
    a, b = geo.tail if k else geo.head
    rng = np.random.default_rng(seed * 2 + k)
    x = rng.integers(lo, hi, (b - a, geo.W)).astype(np.uint16)
    for v in specials:
        x[rng.random(x.shape) < rate] = v
    if impulses:
        x[rng.integers(0, b - a, impulses), rng.integers(0, geo.W, impulses)] = 24000
    return x


def band_windows(geo, halo):
    """per band: (lo, hi, oa, ob) -- the restatement runs on input lines [lo, hi), its output is compared on [oa, ob)"""
    out = []
    for a, b in (geo.head, geo.tail):
        out.append((max(0, a - 2 * halo), min(geo.L, b + 2 * halo), max(0, a - halo), min(geo.L, b + halo)))
    return out


def band_input(geo, k, noise, lo, hi, const=CONST):
    """input lines [lo, hi) of the probe raster as the host sees them"""
    a, b = geo.tail if k else geo.head
    x = np.full((hi - lo, geo.W), const, np.uint16)
    x[a - lo:b - lo] = noise
    return x


def host_raster(geo, noises, const=CONST):
    """the whole probe raster on the host (the host model only)"""
    x = np.full((geo.L, geo.W), const, np.uint16)
    x[geo.head[0]:geo.head[1]] = noises[0]
    x[geo.tail[0]:geo.tail[1]] = noises[1]
    return x


def device_raster(geo, noises, const=CONST):
    """the probe raster on the device: filled there, only the bands cross the link"""
    import torch
    x = torch.full((geo.L, geo.W), const, dtype=torch.int16, device="cuda").view(torch.uint16)
    for (a, b), n in zip((geo.head, geo.tail), noises):
        x[a:b] = torch.from_numpy(n).cuda()
    return x


def _is_np(a):
    return isinstance(a, np.ndarray)


def check_rows(out, bands, const_row, chunk=8192):
    """The checker.  out: (L, Wo) uint16, numpy or torch.  bands: [(oa, ob, want)] -- lines [oa, ob) must equal `want` (host
    arrays, compared on the host).  Every other line must equal const_row (a scalar or (Wo,) uint16), compared where `out`
    lives in chunks of at most `chunk` lines.  Raises AssertionError naming the first line that is wrong."""
    L, Wo = out.shape
    row = np.broadcast_to(np.asarray(const_row, np.uint16), (Wo,))
    if not _is_np(out):
        import torch
        row_d = torch.from_numpy(np.array(row).view(np.int16)).to(out.device)
    pos = 0
    for oa, ob, want in sorted(bands, key=lambda t: t[0]) + [(L, L, None)]:
        assert pos <= oa, "bands overlap"
        for c0 in range(pos, oa, chunk):
            c1 = min(oa, c0 + chunk)
            blk = out[c0:c1]
            if _is_np(out):
                bad = (blk != row).any(axis=1)
                ok, first = not bad.any(), int(np.argmax(bad))
            else:
                bad = (blk.view(torch.int16) != row_d).any(dim=1)
                ok = not bool(bad.any())
                first = int(torch.nonzero(bad)[0]) if not ok else 0
            assert ok, "line %d is not the image of the constant" % (c0 + first)
        if want is not None:
            got = out[oa:ob] if _is_np(out) else out[oa:ob].cpu().numpy()
            assert got.shape == want.shape, (got.shape, want.shape)
            if not np.array_equal(got, want):
                r = int(np.argmax((got != want).any(axis=1)))
                raise AssertionError("line %d differs from the restatement (%d of %d samples in its band)"
                                     % (oa + r, int((got != want).sum()), got.size))
        pos = max(pos, ob)


def rejects(out, bands, const_row):
    try:
        check_rows(out, bands, const_row)
    except AssertionError:
        return True
    return False


# ---- what a 32-bit offset would have done (host model) ---------------------------------------------------------------------
def wrapped_read(x, wrap):
    """the raster a kernel sees whose load offsets wrap at `wrap`: element i >= wrap is element i - wrap"""
    flat = x.reshape(-1).copy()
    n = flat.size - wrap
    assert 0 < n <= wrap
    flat[wrap:] = x.reshape(-1)[:n]
    return flat.reshape(x.shape)


def wrapped_store(out, wrap, before):
    """what is in memory after a kernel whose store offsets wrap at `wrap` wrote `out` over a buffer that held `before`:
    elements >= wrap keep `before`, and their values land on elements 0 .. n - wrap"""
    flat = out.reshape(-1).copy()
    n = flat.size - wrap
    assert 0 < n <= wrap
    flat[wrap:] = np.broadcast_to(np.asarray(before, out.dtype), out.shape).reshape(-1)[wrap:]
    flat[:n] = out.reshape(-1)[wrap:]
    return flat.reshape(out.shape)


# ---- the resampler on column slabs -------------------------------------------------------------------------------------------
def slab_columns(c0, c1, W, dx):
    """columns [a, b) of the slab [c0, c1) of a W-wide image on which a constant-shift bicubic resampling of the slab alone
    equals that of the image: output column x reads source columns within ceil(|dx|) + 2 of x, so that many columns are
    dropped at a slab edge inside the image; an edge that is the image's own is compared through"""
    m = int(np.ceil(abs(dx))) + 2
    a = c0 if c0 == 0 else c0 + m
    b = c1 if c1 == W else c1 - m
    assert a < b
    return a, b


def slabs(W, width=96):
    """three slabs: the left edge, a middle one that does not start on a multiple of 8, the right edge"""
    mid = (W // 2) | 3
    return [(0, width), (mid, mid + width), (W - width, W)]


# ---- the probes: one per operation whose output has the lines of its input ---------------------------------------------------
class Probe:
    """inputs: one (noises, const) per input raster; ref(lo, *rasters) -> (lines, Wo) uint16 is the CPU restatement on input
    lines [lo, lo + lines); halo: the vertical footprint; extra: what the device call needs besides"""

    def __init__(self, name, geo, inputs, halo, ref, **extra):
        self.name, self.geo, self.inputs, self.halo, self.ref, self.extra = name, geo, inputs, halo, ref, extra

    def bands(self):
        return expected_bands(self.geo, self.inputs, self.halo, self.ref)

    def const_row(self):
        # far from the bands the restatement must not depend on the line: asked at two places
        n = 4 * self.halo + 1
        mid = (self.geo.head[1] + self.geo.tail[0]) // 2
        rows = [self.ref(lo, *[np.full((n, self.geo.W), c, np.uint16) for _, c in self.inputs])[n // 2] for lo in (mid, mid + 7)]
        assert np.array_equal(rows[0], rows[1])
        return rows[0]

    def host_inputs(self):
        return [host_raster(self.geo, noises, c) for noises, c in self.inputs]


def expected_bands(geo, inputs, halo, ref):
    """[(oa, ob, want)]: ref on each band with 2 * halo constant lines around it (fewer at the image border, which is then the
    window's border too), compared on the band widened by halo: the window's own border is out of reach of those lines"""
    out = []
    for k, (lo, hi, oa, ob) in enumerate(band_windows(geo, halo)):
        y = ref(lo, *[band_input(geo, k, noises[k], lo, hi, const) for noises, const in inputs])
        out.append((oa, ob, y[oa - lo:ob - lo]))
    return out


def _inp(geo, seed, const=CONST, **kw):
    return ([band_noise(geo, 0, seed, **kw), band_noise(geo, 1, seed, **kw)], const)


def lut(w, seed):
    """(w, 2) RRC coefficients that vary per column"""
    rng = np.random.default_rng(0xB16 + seed)
    return np.stack([np.round(rng.uniform(0.9, 1.1, w), 6), np.round(rng.uniform(-8, 8, w), 4)], 1)


def dc_taps(k, seed):
    """(k, k) signed, asymmetric Q12 taps with DC gain exactly 1: noise of 300 .. 3800 stays clear of both clamps, so a wrong
    neighbour shows in the output"""
    rng = np.random.default_rng(0x7A9 + seed)
    t = rng.integers(-60, 61, (k, k)).astype(np.int64)
    t[k // 2, k // 2] += 4096 - int(t.sum())
    assert int(t.sum()) == 4096 and int(np.abs(t).sum()) <= 32767 and not np.array_equal(t, t[::-1]) and not np.array_equal(t, t[:, ::-1])
    return t.astype(np.int32)


def convolve(img, taps, valid_min=1, spp=1):
    """_mtfc_ref.convolve (the yardstick; test_bigraster_cpu.py holds this one to it) with slices of an edge-padded copy in
    place of its index arrays and int32 sums in place of int64 ones -- sum |taps| <= 32767 keeps acc + 2048 inside int32, as
    include/oip_c.h states --: a tenth of the time on a band of 32760 columns"""
    img = np.asarray(img)
    taps = np.asarray(taps, dtype=np.int32)
    assert int(np.abs(taps.astype(np.int64)).sum()) <= 32767
    L = img.shape[0]
    src = img.reshape(L, -1, spp).astype(np.int32)
    W = src.shape[1]
    ky, kx = taps.shape
    ry, rx = ky // 2, kx // 2
    pad = np.pad(src, ((ry, ry), (rx, rx), (0, 0)), mode="edge")
    nodata = src < valid_min
    acc = np.zeros_like(src)
    for j in range(ky):
        for i in range(kx):
            n = pad[j:j + L, i:i + W]
            acc += taps[j, i] * np.where(n < valid_min, src, n)
    out = np.clip((acc + 2048) >> 12, valid_min, 65535)
    return np.where(nodata, src, out).astype(np.uint16).reshape(img.shape)


def line_tables(geo, spp, seed):
    """(L, spp) int32 gain / offset tables: one pair on the constant lines, a pair of its own on every line of the bands"""
    rng = np.random.default_rng(0x7AB + seed)
    G = np.full((geo.L, spp), 70000, np.int32)
    O = np.full((geo.L, spp), -3 << 16, np.int32)
    for a, b in (geo.head, geo.tail):
        G[a:b] = rng.integers(50000, 90000, (b - a, spp))
        O[a:b] = rng.integers(-40 << 16, 40 << 16, (b - a, spp))
    return G, O


def probes(geo, oracle_mod, folds=(100, 99)):
    """the probes of the raster -> raster entry points, by name.  `folds`: the fold of the vector and of the scalar stitch kernel
    (the stitched line 2 (W - fold) is, or is not, a multiple of 8)"""
    import _despike_ref
    import _seam_lines_ref
    import _seam_ref
    W = geo.W
    P = {}

    def add(name, inputs, halo, ref, **extra):
        P[name] = Probe(name, geo, inputs, halo, ref, **extra)

    kb = lut(W, 1)
    add("rrc", [_inp(geo, 1, specials=(0, 65535, 4095))], 0, lambda lo, x: oracle_mod.rrc(x, kb), kb=kb)
    kb4 = lut(W, 2)          # band-major: columns [b W/4, (b+1) W/4) of the BIL line are band b
    add("mss_split_rrc", [_inp(geo, 2)], 0, lambda lo, x: oracle_mod.rrc(x, kb4), kb=kb4)
    for f in folds:
        add("stitch_rows_f%d" % f, [_inp(geo, 3), _inp(geo, 4, const=1700)], 0,
            lambda lo, l, r, f=f: np.concatenate([l[:, :W - f], r[:, f:]], 1), fold=f)
    order = (2, 1, 0, 3)
    add("permute", [_inp(geo, 5)], 0, lambda lo, x: np.ascontiguousarray(x.reshape(x.shape[0], W // 4, 4)[:, :, list(order)]).reshape(x.shape),
        order=order)
    for ky, spp in ((9, 1), (3, 1), (9, 4), (3, 4)):
        taps = dc_taps(ky, 40 + ky + spp)
        add("convolve_%dx%d_spp%d" % (ky, ky, spp), [_inp(geo, 6 + ky + spp, specials=(0, 65535, 1))], ky // 2,
            lambda lo, x, taps=taps, spp=spp: convolve(x, taps, 1, spp), taps=taps, spp=spp)
    bad = sorted(set(int(v) for v in np.random.default_rng(9).integers(0, W, max(4, W // 400))) | {0, 1, W // 4 - 1, W // 4, W - 1})
    tab, _ = _despike_ref.column_table(bad, W, 4)
    for spp, groups, ct in ((1, 4, tab), (4, 1, None)):
        add("despike_spp%d" % spp, [_inp(geo, 20 + spp, specials=(0, 65535), impulses=geo.W)], 1,
            lambda lo, x, spp=spp, groups=groups, ct=ct: _despike_ref.despike(x, 600, 26, 1, spp, groups, ct)[0],
            spp=spp, groups=groups, coltab=ct, thr=(600, 26, 1),
            counts=lambda x, spp=spp, groups=groups, ct=ct: _despike_ref.despike(x, 600, 26, 1, spp, groups, ct)[1])
    fold = folds[0] if folds[0] % 4 == 0 else folds[0] - folds[0] % 4
    # fs = `fold` samples: the stitched line is a multiple of 8 samples (the vector kernels); fs = folds[1] at spp 1: it is not
    # (the scalar kernels; at spp 4 every legal fs leaves a multiple of 8)
    for spp, h, fs, tag in ((1, 16, fold, ""), (4, 0, fold, ""), (1, 0, fold, ""), (4, 16, fold, ""), (1, 16, folds[1], "_scalar")):
        fpx = fs // spp
        h = min(h, fpx)
        assert (2 * (W - fs) % 8 != 0) == bool(tag)
        rng = np.random.default_rng(60 + spp)
        G, O = rng.integers(60000, 72000, spp), rng.integers(-30 << 16, 30 << 16, spp)
        add("stitch_balanced_spp%d_h%d%s" % (spp, h, tag), [_inp(geo, 30 + spp + h), _inp(geo, 31 + spp + h, const=1700)], 0,
            lambda lo, l, r, spp=spp, h=h, G=G, O=O, fpx=fpx: _seam_ref.stitch(l, r, fpx, spp, G, O, h, 1),
            spp=spp, feather=h, fold=fpx, G=G.astype(np.int32), O=O.astype(np.int32))
        LG, LO = line_tables(geo, spp, spp + h)
        add("stitch_balanced_lines_spp%d_h%d%s" % (spp, h, tag), [_inp(geo, 40 + spp + h), _inp(geo, 41 + spp + h, const=1700)], 0,
            lambda lo, l, r, spp=spp, h=h, LG=LG, LO=LO, fpx=fpx: _seam_lines_ref.stitch_lines(l, r, fpx, spp, LG[lo:lo + l.shape[0]],
                                                                                                 LO[lo:lo + l.shape[0]], h, 1),
            spp=spp, feather=h, fold=fpx, LG=LG, LO=LO)
    return P


# ---- the checks that are not raster -> raster ---------------------------------------------------------------------------------
def seam_inputs(geo, spp):
    """the two rasters of the seam-moments check as (noises, const): the left one's constant is 1500, the right one's 1700"""
    return [_inp(geo, 70 + spp, const=1500), _inp(geo, 72 + spp, const=1700)]


def expected_block_moments(geo, ins, fold, spp, B, valid_min, valid_max):
    """(nb, 6, spp) uint64 totals of oip_seam_moments_blocks_u16 on the probe rasters `ins` without the rasters: the closed form
    for the constant lines (the totals of one such line times their number) plus _seam_ref.moments of each band line in place of
    a constant one"""
    import _seam_lines_ref
    import _seam_ref
    (ln, lc), (rn, rc) = ins
    one = _seam_ref.moments(np.full((1, geo.W), lc, np.uint16), np.full((1, geo.W), rc, np.uint16), fold, spp, valid_min, valid_max)
    blocks = _seam_lines_ref.blocks(geo.L, B)
    want = np.stack([one * np.uint64(b - a) for a, b in blocks])
    for j, (a, b) in enumerate((geo.head, geo.tail)):
        for r in range(a, b):
            k = min(r // B, len(blocks) - 1)
            want[k] += _seam_ref.moments(ln[j][r - a:r - a + 1], rn[j][r - a:r - a + 1], fold, spp, valid_min, valid_max) - one
    return want


def merge_tiles(raster, vp, hp, sl, sc):
    """the big-endian tiles (vp, hp, sl, sc) that oip_merge_subimages_be16 turns into `raster` (vp sl lines of hp sc samples)"""
    assert raster.shape == (vp * sl, hp * sc)
    return np.ascontiguousarray(raster.reshape(vp, sl, hp, sc).transpose(0, 2, 1, 3)).byteswap()


def lzw_lines(geo):
    """the lines whose strips the LZW check compares byte for byte: the first, the one that straddles `wrap`, the first wholly
    beyond it, the last"""
    return (0, geo.first_line_beyond - 1, geo.first_line_beyond, geo.L - 1)
