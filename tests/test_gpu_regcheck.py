"""GPU: oip_match_tiles_u16, the kernel of `oip regcheck`, against the numpy restatement in _regcheck_ref.py.  The sums are
exact integers, so records and per-offset sums are compared by equality of every word; the peak index (and with it the words
that depend on it) wherever the restatement's two best scores differ by more than 1e-9 -- on the textures that is every tile,
which the tests assert.  Output buffers are pre-filled with a pattern no sum can equal and carry spare words behind the last
tile, so unwritten and overwritten words both show."""
import functools

import numpy as np
import pytest

import _regcheck_ref as ref

pytestmark = pytest.mark.gpu
FILL = 0x7BCDABCDABCDABCD
SPARE = 5
# (T, S, nx, ny): every T of {8, 16, 24, 64, 128} and every S of {1, 3, 4, 16}; S = 16 is the item loop (1089 offsets > 256 lanes),
# S = 1 the row partitions capped by T (T = 8) and by 256 / 9 (T >= 64), S = 3 and 4 partitions of 5 and 3
CASES = [(8, 1, 3, 2), (8, 3, 3, 2), (16, 4, 3, 2), (24, 3, 2, 3), (64, 4, 3, 2), (128, 16, 2, 1), (8, 16, 2, 2), (128, 1, 2, 2), (24, 16, 2, 1),
         (64, 1, 2, 2), (16, 3, 3, 3), (128, 4, 1, 2)]
LAYOUTS = [(1, 4), (4, 1), (4, 4)]                               # (stride of A, stride of B) per shift of a case; (1, 1) below


def _size(T, S, n, step):
    return T + 2 * S + (n - 1) * step


@functools.lru_cache(maxsize=None)
def _texture_case(T, S, nx, ny, k):
    """pair k of the case and its restatement, computed once"""
    step = ref.step_of(T)
    w, h = _size(T, S, nx, step), _size(T, S, ny, step)
    shift = ref.shifts(S)[k]
    A, B = ref.pair(h, w, shift, 1000 * T + 10 * S + k)
    g = ref.grid(w, h, T, S, step)
    assert g[2:] == (nx, ny)
    grid = (g[0], g[1], step, step, nx, ny)
    return A, B, grid, shift, ref.match_tiles(A, B, T, S, *grid)


def _plane(img, stride, pad, offset, band, seed):
    """img laid out with `stride` samples between its samples (band `band` of a chunky raster), lines w * stride + pad apart,
    `offset` samples into a buffer of seeded garbage -> (device buffer, byte address of the plane, pitch)"""
    import torch
    h, w = img.shape
    pitch = w * stride + pad
    rng = np.random.default_rng(seed)
    buf = rng.integers(0, 65536, offset + h * pitch + 8).astype(np.uint16)
    view = buf[offset:offset + h * pitch].reshape(h, pitch)
    view[:, band:band + w * stride:stride] = img
    d = torch.from_numpy(buf.view(np.int16)).cuda()
    return d, d.data_ptr() + 2 * (offset + band), pitch


def _match(ctx, a, b, w, rows, T, S, grid, valid=(1, 65535), with_sums=True):
    """a, b: (buffer, address, pitch, stride).  -> (records (n, 20), sums (n, K^2, 3) or None) as uint64"""
    import torch
    x0, y0, sx, sy, nx, ny = grid
    n, K2 = nx * ny, (2 * S + 1) ** 2
    fill = np.array(FILL, np.uint64).view(np.int64).item()
    rec = torch.full((n * 20 + SPARE,), fill, dtype=torch.int64, device="cuda")
    sums = torch.full((n * K2 * 3 + SPARE,), fill, dtype=torch.int64, device="cuda") if with_sums else None
    ctx.match_tiles_u16(a[1], a[2], a[3], b[1], b[2], b[3], w, rows, T, S, x0, y0, sx, sy, nx, ny, valid[0], valid[1], rec, sums)
    ctx.sync()
    r = rec.cpu().numpy().view(np.uint64)
    assert (r[n * 20:] == FILL).all(), "words behind the last record were written"
    s = None
    if with_sums:
        s = sums.cpu().numpy().view(np.uint64)
        assert (s[n * K2 * 3:] == FILL).all(), "words behind the last tile's sums were written"
        s = s[:n * K2 * 3].reshape(n, K2, 3)
    return r[:n * 20].reshape(n, 20), s


def _compare(got, want, min_gap=1e-9):
    """-> the number of tiles whose peak was compared"""
    (rec, sums), (wrec, wsums, gap) = got, want
    if sums is not None:
        assert np.array_equal(sums, wsums)
    assert np.array_equal(rec[:, :4], wrec[:, :4])
    sure = gap > min_gap
    assert np.array_equal(rec[sure], wrec[sure])
    return int(sure.sum())


@pytest.mark.parametrize("T,S,nx,ny", CASES)
def test_textures(ctx, T, S, nx, ny):
    """the three shifted pairs of a case at step max(T / 2, 5) (overlapping tiles), each in another layout: strides 1 and 4 mixed
    between A and B, pitches longer than the line, B (or A) starting one sample into its buffer; windows touch the last line and
    column; every tile's peak is compared, and is the shift"""
    for k, (sa, sb) in enumerate(LAYOUTS):
        A, B, grid, shift, want = _texture_case(T, S, nx, ny, k)
        h, w = A.shape
        a = _plane(A, sa, 3 * k, k % 2, 2 if sa == 4 else 0, 11 + k) + (sa,)
        b = _plane(B, sb, 5, 1 - k % 2, 3 if sb == 4 else 0, 21 + k) + (sb,)
        assert grid[0] + (nx - 1) * grid[2] + T + S == w and grid[1] + (ny - 1) * grid[3] + T + S == h
        assert _compare(_match(ctx, a, b, w, h, T, S, grid), want) == nx * ny, "a tile was excluded"
        K = 2 * S + 1
        assert (want[0][:, 4] == (shift[1] + S) * K + shift[0] + S).all()


def test_sums_null_gives_the_same_records(ctx):
    for T, S, nx, ny in (CASES[2], CASES[6]):
        A, B, grid, _, want = _texture_case(T, S, nx, ny, 1)
        h, w = A.shape
        a, b = _plane(A, 1, 0, 0, 0, 1) + (1,), _plane(B, 1, 0, 0, 0, 2) + (1,)
        rec, none = _match(ctx, a, b, w, h, T, S, grid, with_sums=False)
        assert none is None and np.array_equal(rec, want[0])
        assert np.array_equal(_match(ctx, a, b, w, h, T, S, grid)[0], rec)


@pytest.mark.parametrize("nx,ny,sx,sy", [(1, 1, 20, 20), (1, 4, 20, 7), (5, 1, 7, 20), (4, 3, 23, 17), (3, 3, 1, 1)])
def test_grid_shapes(ctx, nx, ny, sx, sy):
    """T = 16, S = 3: one tile, one column, one row, steps above and below T and different in x and y, a grid that does not
    start at (S, S), and an image with room to spare behind the last tile"""
    T, S = 16, 3
    for x0, y0, spare in ((S, S, 0), (S + 2, S + 5, 3)):
        w, h = x0 + (nx - 1) * sx + T + S + spare, y0 + (ny - 1) * sy + T + S + spare
        A, B = ref.pair(h, w, (2, -1), 300 + nx + ny + spare)
        grid = (x0, y0, sx, sy, nx, ny)
        want = ref.match_tiles(A, B, T, S, *grid)
        a, b = _plane(A, 1, 0, 0, 0, 1) + (1,), _plane(B, 4, 0, 0, 1, 2) + (4,)
        assert _compare(_match(ctx, a, b, w, h, T, S, grid), want) == nx * ny


def test_full_range_noise_breaks_32_bit_sums(ctx):
    """independent full-range noise with 30 % of the samples at 65535, T = 128: sum a b reaches 2^44, a row of it 2^39.  Only the
    sums are compared (the scores of noise against noise lie within rounding of each other)."""
    T, S, nx, ny = 128, 4, 2, 1
    w, h = _size(T, S, nx, 64), _size(T, S, ny, 64)
    rng = np.random.default_rng(77)
    A, B = (rng.integers(0, 65536, (h, w)).astype(np.uint16) for _ in range(2))
    A[rng.random(A.shape) < 0.3] = 65535
    B[rng.random(B.shape) < 0.3] = 65535
    grid = (S, S, 64, 64, nx, ny)
    wrec, wsums, _ = ref.match_tiles(A, B, T, S, *grid, valid_min=0)
    assert int(wsums[..., 2].max()) > 1 << 43 and int(wrec[:, 1].max()) > 1 << 44
    a, b = _plane(A, 1, 0, 0, 0, 1) + (1,), _plane(B, 1, 0, 0, 0, 2) + (1,)
    rec, sums = _match(ctx, a, b, w, h, T, S, grid, valid=(0, 65535))
    assert np.array_equal(sums, wsums) and np.array_equal(rec[:, :4], wrec[:, :4])
    # all samples at 65535: the largest sums there are
    A[:], B[:] = 65535, 65535
    wrec, wsums, _ = ref.match_tiles(A, B, T, S, *grid, valid_min=0)
    a, b = _plane(A, 1, 0, 0, 0, 1) + (1,), _plane(B, 1, 0, 0, 0, 2) + (1,)
    rec, sums = _match(ctx, a, b, w, h, T, S, grid, valid=(0, 65535))
    assert np.array_equal(sums, wsums) and np.array_equal(rec, wrec) and int(wsums[0, 0, 2]) == 128 * 128 * 65535 * 65535


def test_constant_image_is_flat_with_the_peak_at_the_centre(ctx):
    for T, S in ((16, 3), (8, 16)):
        w, h = _size(T, S, 2, T), _size(T, S, 2, T)
        A = np.full((h, w), 1000, np.uint16)
        grid = (S, S, T, T, 2, 2)
        want = ref.match_tiles(A, A, T, S, *grid)
        K = 2 * S + 1
        assert (want[0][:, 4] == S * K + S).all() and ref.peak(want[0][0], T, S)[3] == ref.FLAT | ref.WEAK
        a = _plane(A, 1, 0, 0, 0, 1) + (1,)
        rec, sums = _match(ctx, a, a, w, h, T, S, grid)
        assert np.array_equal(rec, want[0]) and np.array_equal(sums, want[1])
        # a constant B under a textured A: no offset has a score either
        X, _ = ref.pair(h, w, (0, 0), 5)
        want = ref.match_tiles(X, A, T, S, *grid)
        rec, sums = _match(ctx, _plane(X, 1, 0, 0, 0, 3) + (1,), a, w, h, T, S, grid)
        assert np.array_equal(rec, want[0]) and (rec[:, 4] == S * K + S).all()


@pytest.mark.parametrize("valid", [(1, 65535), (300, 3000), (0, 65535)])
def test_no_data_counts(ctx, valid):
    """zeros inside both images, and a valid range that cuts into the data: bad_a counts the template, bad_b the whole search
    window; the sums take every sample as it is"""
    T, S, nx, ny = 16, 4, 3, 3
    A, B, grid, _, _ = _texture_case(T, S, nx, ny, 2)
    A, B = A.copy(), B.copy()
    rng = np.random.default_rng(9)
    A[rng.random(A.shape) < 0.02] = 0
    B[rng.random(B.shape) < 0.02] = 0
    B[:, -1] = 0                                                 # the window's last column only: bad_b of the last tiles, no template
    h, w = A.shape
    want = ref.match_tiles(A, B, T, S, *grid, valid_min=valid[0], valid_max=valid[1])
    if valid[0]:
        assert want[0][:, 2].max() > 0 and (want[0][:, 3] > want[0][:, 2]).any()
    else:
        assert (want[0][:, 2:4] == 0).all()
    a, b = _plane(A, 4, 0, 0, 0, 1) + (4,), _plane(B, 1, 1, 0, 0, 2) + (1,)
    assert _compare(_match(ctx, a, b, w, h, T, S, grid, valid=valid), want) > 0


def test_invalid_arguments(ctx):
    import torch
    T, S = 16, 3
    w = h = _size(T, S, 2, 16)
    img = torch.zeros((h, 4 * w), dtype=torch.int16, device="cuda")
    rec = torch.zeros(4 * 20, dtype=torch.int64, device="cuda")
    ok = dict(a=img, pitch_a=w, stride_a=1, b=img, pitch_b=4 * w, stride_b=4, w=w, rows=h, T=T, S=S, x0=S, y0=S, step_x=16, step_y=16, nx=2, ny=2,
              valid_min=1, valid_max=65535, records=rec, sums=None)
    ctx.match_tiles_u16(**ok)
    ctx.sync()
    for bad in (dict(T=12), dict(T=0), dict(T=-8), dict(T=136), dict(T=4), dict(S=0), dict(S=17), dict(S=-1), dict(stride_a=2), dict(stride_b=3),
                dict(stride_a=0), dict(stride_b=8), dict(w=0), dict(rows=0), dict(nx=0), dict(ny=0), dict(nx=-1), dict(step_x=0), dict(step_y=0),
                dict(pitch_a=w - 1), dict(pitch_b=4 * w - 4), dict(valid_min=-1), dict(valid_max=65536), dict(valid_min=9, valid_max=8),
                dict(a=None), dict(b=None), dict(records=None), dict(a=img.data_ptr() + 1), dict(records=rec.data_ptr() + 4),
                dict(x0=S - 1), dict(y0=S - 1), dict(x0=S + 1), dict(y0=S + 1), dict(nx=3), dict(ny=3), dict(step_x=17), dict(step_y=17),
                dict(w=w - 1), dict(rows=h - 1), dict(T=24), dict(S=4), dict(nx=1 << 16, ny=1 << 15),dict(ny=1 << 40, step_y=1 << 30)):
        with pytest.raises(ValueError):
            ctx.match_tiles_u16(**dict(ok, **bad))
