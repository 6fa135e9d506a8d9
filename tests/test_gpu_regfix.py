"""GPU: oip_warp_grid_bicubic_u16, the kernel of `oip regfix`, against the restatement in _regfix_ref.py.  The field is integer
arithmetic and the 16-tap sum is OpenCV's in its own order, so every comparison is equality.

The kernel takes a tile of 256 columns x 8 lines per block and one pixel per lane: the widths and heights below are a single
lane, fewer lanes than a wave, one and several line tiles, a last tile of one line (L = 1, 37 = 4 * 8 + 5 is several and a
partial one), and (300, 20) two tiles across.  Steps 5 and 7 put many node columns and lines into a tile, 64 and 100 one or two."""
import functools

import numpy as np
import pytest

import _regfix_ref as ref

pytestmark = pytest.mark.gpu

WIDTHS = [1, 3, 7, 8, 9, 64, 67, 200]
HEIGHTS = [1, 4, 37]
SHAPES = [(W, L) for W in WIDTHS for L in HEIGHTS] + [(300, 20)]


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _image(W, L, spp=1):
    """full-range data; shared by the tests of a shape, which leave it unchanged"""
    rng = np.random.default_rng(77 * W + L + 1000 * spp)
    img = rng.integers(0, 65536, (L, W * spp), dtype=np.uint16)
    return img if spp == 1 else img.reshape(L, W, spp)


def _lattice(W, L, sx, sy, gx0, gy0):
    """node counts that cover the raster from (gx0, gy0) on, at least 2 x 2"""
    return max(2, -(-(W - gx0) // sx) + 1), max(2, -(-(L - gy0) // sy) + 1)


def _random(W, L, sx, sy, gx0, gy0, amp, seed):
    nx, ny = _lattice(W, L, sx, sy, gx0, gy0)
    rng = np.random.default_rng(seed)
    return dict(NX=rng.integers(-amp, amp + 1, (ny, nx)).astype(np.int32), NY=rng.integers(-amp, amp + 1, (ny, nx)).astype(np.int32),
                gx0=gx0, gy0=gy0, sx=sx, sy=sy)


def _steep(W, L):
    """adjacent nodes 20 px apart in x and in y: neighbouring pixels read windows far from each other"""
    f = _random(W, L, 5, 5, -2, -1, 0, 0)
    ny, nx = f["NX"].shape
    chk = (np.add.outer(np.arange(ny), np.arange(nx)) & 1) * 2 - 1
    f["NX"], f["NY"] = (chk * 10240).astype(np.int32), (-chk * 10240 + 512).astype(np.int32)
    return f


def _const(W, L, vx, vy):
    f = _random(W, L, 64, 64, -1, -1, 0, 0)
    f["NX"], f["NY"] = np.full_like(f["NX"], vx), np.full_like(f["NY"], vy)
    return f


def _single(f, axis):
    """one node on an axis: the first node line / column of f alone"""
    g = dict(f)
    if axis == "x":
        g["NX"], g["NY"] = f["NX"][:, :1].copy(), f["NY"][:, :1].copy()
    else:
        g["NX"], g["NY"] = f["NX"][:1].copy(), f["NY"][:1].copy()
    return g


FIELDS = {
    "zero": lambda W, L: dict(_random(W, L, 64, 64, -5, -7, 0, 0)),
    "random16_steps_5_7": lambda W, L: _random(W, L, 5, 7, -3, -9, 16384, 1),           # origin left of and above the raster
    "random16_steps_7_5": lambda W, L: _random(W, L, 7, 5, W // 2, L // 2, 16384, 2),     # origin inside it: the edge value left of it
    "random16_steps_64_100": lambda W, L: _random(W, L, 64, 100, 2, 1, 16384, 3),
    "random16_steps_100_64": lambda W, L: _random(W, L, 100, 64, -250, -130, 16384, 4),
    "beyond_far_edge": lambda W, L: _random(W, L, 5, 7, W + 10, L + 3, 9000, 5),         # every pixel takes node (0, 0)
    "steep_20px": _steep,
    "nx1": lambda W, L: _single(_random(W, L, 5, 7, -3, -9, 12000, 6), "x"),
    "ny1": lambda W, L: _single(_random(W, L, 7, 5, -3, -9, 12000, 7), "y"),
    "one_node": lambda W, L: _single(_single(_random(W, L, 5, 7, 1, 1, 12000, 8), "x"), "y"),
    "minus_one_1024th": lambda W, L: _const(W, L, -1, -17),                                 # rounds to -1/32 px: phase 31 of the pixel before
}


def _warp(ctx, img, W, L, spp, f, band_mask=None):
    import torch
    out = torch.zeros(L, W * spp, dtype=torch.uint16, device="cuda")
    ctx.warp_grid_bicubic_u16(_cuda(img), out, W, L, spp, f["NX"], f["NY"], f["gx0"], f["gy0"], f["sx"], f["sy"], band_mask)
    ctx.sync()
    return out.cpu().numpy().reshape(img.shape)


def _ref(img, f, band_mask=None, **kw):
    return ref.warp(img, f["NX"], f["NY"], f["gx0"], f["gy0"], f["sx"], f["sy"], band_mask, **kw)


@pytest.mark.parametrize("name", sorted(FIELDS))
@pytest.mark.parametrize("W,L", SHAPES)
def test_equals_restatement(ctx, oracle_mod, W, L, name):
    img, f = _image(W, L), FIELDS[name](W, L)
    got = _warp(ctx, img, W, L, 1, f)
    assert np.array_equal(got, _ref(img, f)), name
    if name == "zero":
        assert np.array_equal(got, img)                          # a zero field is the identity


def test_fields_do_what_they_are_for():
    """reads cross all four borders, values are negative and positive, and the steep field separates neighbours' windows"""
    W, L = 200, 37
    f = FIELDS["random16_steps_5_7"](W, L)
    sx, sy = ref.positions(f["NX"], f["NY"], W, f["gx0"], f["gy0"], f["sx"], f["sy"], 0, L)
    X, Y = (sx >> 5) - 1, (sy >> 5) - 1
    assert X.min() < 0 and X.max() + 3 >= W and Y.min() < 0 and Y.max() + 3 >= L and f["NX"].min() < 0 < f["NX"].max()
    assert ((X >= 0) & (X + 3 < W) & (Y >= 0) & (Y + 3 < L)).any()            # ... and the interior order is taken as well
    f = FIELDS["steep_20px"](W, L)
    sx, _ = ref.positions(f["NX"], f["NY"], W, f["gx0"], f["gy0"], f["sx"], f["sy"], 0, L)
    assert np.abs(np.diff(sx >> 5, axis=1)).max() >= 4                        # neighbours' windows do not overlap


@pytest.mark.parametrize("mask", [1, 2, 4, 8, 5, 10, 15])
@pytest.mark.parametrize("W,L", [(9, 4), (67, 37), (300, 20)])
def test_four_samples_and_band_masks(ctx, oracle_mod, W, L, mask):
    img, f = _image(W, L, 4), FIELDS["random16_steps_5_7"](W, L)
    got = _warp(ctx, img, W, L, 4, f, mask)
    assert np.array_equal(got, _ref(img, f, mask))
    for c in range(4):
        if not mask & (1 << c):
            assert np.array_equal(got[:, :, c], img[:, :, c])    # bands outside the mask are the input's


@pytest.mark.parametrize("spp", [1, 4])
def test_unaligned_base_pointers(ctx, oracle_mod, spp):
    """source and destination one sample off a 16-byte boundary: no 8-byte access applies"""
    import torch
    W, L = 67, 37
    img, f = _image(W, L, spp), FIELDS["random16_steps_7_5"](W, L)
    n = L * W * spp
    sbuf = torch.zeros(n + 8, dtype=torch.uint16, device="cuda")
    dbuf = torch.zeros(n + 8, dtype=torch.uint16, device="cuda")
    for off_s, off_d in ((1, 0), (0, 3), (1, 1)):
        sbuf[off_s:off_s + n] = _cuda(img.reshape(-1))
        dbuf.zero_()
        ctx.warp_grid_bicubic_u16(sbuf[off_s:], dbuf[off_d:], W, L, spp, f["NX"], f["NY"], f["gx0"], f["gy0"], f["sx"], f["sy"])
        ctx.sync()
        d = dbuf.cpu().numpy()
        assert np.array_equal(d[off_d:off_d + n].reshape(img.shape), _ref(img, f))
        assert not d[:off_d].any() and not d[off_d + n:].any()                # nothing written around the raster


@pytest.mark.parametrize("name", ["random16_steps_5_7", "random16_steps_64_100", "steep_20px", "zero"])
@pytest.mark.parametrize("spp,mask", [(1, 1), (4, 6)])
def test_strip_in_three_calls(ctx, oracle_mod, name, spp, mask):
    """blocks of 13 lines, each call handed only the source lines oip_warp_grid_src_range names: the bytes of one call, and the
    range contains the extreme lines the restatement taps"""
    import torch
    import opticalimageprocessor_amd as oip
    W, L, B = 67, 37, 13
    img, f = _image(W, L, spp), FIELDS[name](W, L)
    want = _ref(img, f, mask)
    got = np.zeros_like(want)
    for r in range(0, L, B):
        m = min(B, L - r)
        a, b = oip.warp_grid_src_range(r, m, L, f["NY"], f["gy0"], f["sy"], include_output=mask != (1 << spp) - 1)
        lo, hi = ref.tap_lines(f["NY"], W, f["gx0"], f["gy0"], f["sx"], f["sy"], r, m)
        lo, hi = max(lo, 0), min(hi, L - 1)
        if lo <= hi:
            assert a <= lo and hi < b, (r, a, b, lo, hi)
        assert 0 <= a <= b <= L
        if mask != (1 << spp) - 1:
            assert a <= r and r + m <= b
        src = _cuda(img[a:b]) if b > a else torch.zeros(8, dtype=torch.uint16, device="cuda")
        part = torch.zeros(m, W * spp, dtype=torch.uint16, device="cuda")
        ctx.warp_grid_bicubic_u16(src, part, W, L, spp, f["NX"], f["NY"], f["gx0"], f["gy0"], f["sx"], f["sy"], mask, src_row0=a, src_rows=b - a,
                                  out_row0=r, out_rows=m)
        ctx.sync()
        got[r:r + m] = part.cpu().numpy().reshape(got[r:r + m].shape)
    assert np.array_equal(got, want)


def test_constant_field_equals_the_constant_shift_kernel(ctx, oracle_mod):
    """(dx, dy) = (13/32, -42/32) on every node against oip_remap_shift_bicubic_u16 inside a single section: the lines of its
    first section (390 lines of 400) that are out of reach of the section's lower edge -- the shift kernel resamples section by
    section, this one the whole raster"""
    import torch
    W, L = 64, 400
    img = _image(W, L)
    f = dict(NX=np.full((3, 2), 13 * 32, np.int32), NY=np.full((3, 2), -42 * 32, np.int32), gx0=5, gy0=-3, sx=64, sy=300)
    got = _warp(ctx, img, W, L, 1, f)
    dst = torch.zeros(L, W, dtype=torch.uint16, device="cuda")
    ctx.remap_shift_bicubic_u16(_cuda(img), dst, W, L, 13 / 32, -42 / 32, 390, 399)
    ctx.sync()
    assert np.array_equal(got[:380], dst.cpu().numpy()[:380])
    assert np.array_equal(got, _ref(img, f))


def test_invalid_arguments(ctx):
    import torch
    import opticalimageprocessor_amd as oip
    W, L = 64, 37
    src = _cuda(_image(W, L))
    dst = torch.zeros(L, W, dtype=torch.uint16, device="cuda")
    N = np.zeros((3, 3), np.int32)
    ok = dict(src=src, dst=dst, W=W, L=L, spp=1, nodes_x=N, nodes_y=N, gx0=0, gy0=0, sx=32, sy=16)
    ctx.warp_grid_bicubic_u16(**ok)                               # the base case is valid
    ctx.warp_grid_bicubic_u16(**dict(ok, out_row0=5, out_rows=0, src_row0=0, src_rows=0))      # no output lines: a no-op
    big = N.copy()
    big[1, 2] = 65537
    neg = N.copy()
    neg[0, 0] = -65537
    down = np.full((3, 3), 5 * 1024, np.int32)                    # reads 5 lines below
    bad = [dict(sx=0), dict(sy=0), dict(sx=65537), dict(sy=65537), dict(spp=2), dict(spp=4, band_mask=16), dict(band_mask=0), dict(band_mask=2),
           dict(W=0), dict(L=0), dict(nodes_x=big), dict(nodes_y=big), dict(nodes_x=neg), dict(dst=src),
           dict(out_row0=30, out_rows=8), dict(out_row0=-1, out_rows=2), dict(out_rows=L + 1), dict(src_row0=-1), dict(src_rows=L + 1),
           dict(src_row0=1, src_rows=L - 1),                                           # line 0 is read by line 0's window
           dict(src_rows=L - 1),                                                       # ... and line L - 1 by the last one's
           dict(nodes_y=down, out_row0=0, out_rows=8, src_row0=0, src_rows=12),        # lines up to 8 + 5 + 2 are needed
           dict(spp=4, W=W // 4, band_mask=1, nodes_y=down, out_row0=0, out_rows=8, src_row0=4, src_rows=20)]      # the copied bands read line 0
    for kw in bad:
        with pytest.raises(ValueError):
            ctx.warp_grid_bicubic_u16(**dict(ok, **kw))
    ctx.warp_grid_bicubic_u16(**dict(ok, nodes_y=down, out_row0=0, out_rows=8, src_row0=4, src_rows=12))        # exactly what is needed
    ctx.sync()
    for kw in (dict(out_row0=-1), dict(out_rows=L + 1), dict(sy=0), dict(sy=65537), dict(nodes_y=big)):
        with pytest.raises(ValueError):
            oip.warp_grid_src_range(**dict(dict(out_row0=0, out_rows=L, L=L, nodes_y=N, gy0=0, sy=16), **kw))
    assert oip.warp_grid_src_range(5, 0, L, N, 0, 16) == (0, 0)
    up = np.full((2, 2), -64 * 1024, np.int32)
    assert oip.warp_grid_src_range(0, 8, L, up, 0, 16) == (0, 0)                          # every window lies above the raster
    assert oip.warp_grid_src_range(0, 8, L, up, 0, 16, include_output=True) == (0, 8)
