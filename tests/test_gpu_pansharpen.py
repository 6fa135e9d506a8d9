"""GPU: oip_pansharpen_sfim_u16, the kernel of `oip pansharpen`, against the restatement in _pansharpen_ref.py.  The up-sampling is
integer arithmetic and the modulation three IEEE operations rounded one by one, so every comparison is equality, the two
counters included.  The low-resolution PAN comes from oip_decimate_box_u16, as in the tool.

The kernel gives a lane one MSS column cell (4 output pixels of a line) and a block 256 cells x 32 MSS lines (1024 x 128 output
pixels).  Besides the widths and heights the definition asks for, EXTRA holds what that tile calls for: one wave (64 cells), a
full tile, a tile and a partial one across (300 = 256 + 44) and down (35 = 32 + 3), and 33 lines on one wave."""
import functools

import numpy as np
import pytest

import _pansharpen_ref as ref

pytestmark = pytest.mark.gpu

WIDTHS = [1, 2, 3, 5, 16, 17, 64, 67, 130]
HEIGHTS = [1, 2, 5, 9]
EXTRA = [(256, 32), (300, 35), (64, 33)]
SHAPES = [(w, h) for w in WIDTHS for h in HEIGHTS] + EXTRA
FILL = 0x5A5A


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _data(w, h, kind):
    """PAN (4h, 4w) and MSS (h, w, 4); shared by the tests of a shape, which leave them unchanged.
    full: full-range noise; bits12: 12-bit noise; contrast: MSS-cell-sized patches of 200 .. 3200 or 50000 .. 53000 -- next to a
    bright patch the up-sampled low-resolution PAN undershoots to 0 or to a few counts, so gains pass every limit and UL == 0 occurs"""
    rng = np.random.default_rng(1000 * w + 10 * h + len(kind))
    if kind == "contrast":
        lvl = np.where(rng.random((h, w)) < 0.5, 200, 50000)
        P = (np.kron(lvl, np.ones((4, 4), np.int64)) + rng.integers(0, 3000, (4 * h, 4 * w))).astype(np.uint16)
        return P, rng.integers(0, 65536, (h, w, 4), dtype=np.uint16)
    top = 65536 if kind == "full" else 4096
    return rng.integers(0, top, (4 * h, 4 * w), dtype=np.uint16), rng.integers(0, top, (h, w, 4), dtype=np.uint16)


@functools.lru_cache(maxsize=None)
def _want(w, h, kind, G=4):
    P, M = _data(w, h, kind)
    return ref.fuse(P, M, G=G)


def _low(ctx, pan, w, h):
    import torch
    low = torch.zeros(h, w, dtype=torch.uint16, device="cuda")
    ctx.decimate_box_u16(pan, 4 * w, 4 * w, 4 * h, 1, 4, low, w)
    return low


def _fuse(ctx, P, M, G=4, stats=True, out_row0=0, out_rows=None):
    """(lines, counters) of one call on freshly uploaded rasters"""
    import torch
    h, w, _ = M.shape
    pan, mss = _cuda(P), _cuda(M)
    low = _low(ctx, pan, w, h)
    n = 4 * h - out_row0 if out_rows is None else out_rows
    out = torch.full((max(n, 1), 4 * w, 4), FILL, dtype=torch.int16, device="cuda").view(torch.uint16)
    st = torch.zeros(2, dtype=torch.int64, device="cuda") if stats else None
    ctx.pansharpen_sfim_u16(pan[out_row0:] if out_row0 < 4 * h else pan, mss, low, w, h, out, G, st, out_row0, n)
    ctx.sync()
    return out.cpu().numpy()[:n], (tuple(int(v) for v in st.cpu().numpy()) if stats else None)


@pytest.mark.parametrize("kind", ["full", "bits12"])
@pytest.mark.parametrize("w,h", SHAPES)
def test_equals_restatement(ctx, w, h, kind):
    P, M = _data(w, h, kind)
    got, counts = _fuse(ctx, P, M)
    want, wcounts = _want(w, h, kind)
    assert np.array_equal(got, want) and counts == wcounts


def test_low_resolution_pan_is_the_box_mean(ctx):
    for w, h in ((5, 9), (67, 5), (300, 35)):
        P, _ = _data(w, h, "full")
        assert np.array_equal(_low(ctx, _cuda(P), w, h).cpu().numpy(), ref.box4(P).astype(np.uint16))


@pytest.mark.parametrize("w,h,windows", [(67, 9, [(0, 1), (1, 6), (7, 13), (20, 16)]), (300, 35, [(0, 3), (3, 130), (133, 6), (139, 1)]),
                                         (5, 1, [(0, 1), (1, 1), (2, 1), (3, 1)]), (17, 40, [(0, 127), (127, 2), (129, 31)])])
def test_windows_and_shards(ctx, w, h, windows):
    """windows that start and end off multiples of 4 and windows of one line; the shards put together are the whole, counters too
    (G = 1: both counters count)"""
    P, M = _data(w, h, "contrast")
    want, wcounts = _want(w, h, "contrast", 1)
    assert wcounts[0] > 0 and wcounts[1] > 0 and sum(n for _, n in windows) == 4 * h
    parts, z, c = [], 0, 0
    for a, n in windows:
        got, (zz, cc) = _fuse(ctx, P, M, G=1, out_row0=a, out_rows=n)
        assert np.array_equal(got, want[a:a + n]), (a, n)
        parts.append(got)
        z, c = z + zz, c + cc
    assert np.array_equal(np.concatenate(parts), want) and (z, c) == wcounts


@pytest.mark.parametrize("w,h", [(5, 2), (67, 9), (300, 35)])
def test_odd_pitches_and_unaligned_bases(ctx, w, h):
    """every raster one or three samples off its alignment and with pitches that are no multiple of 4 or 8: the general kernel;
    nothing is written between or around the product's lines"""
    import torch
    P, M = _data(w, h, "full")
    want, wcounts = _want(w, h, "full")

    def pitched(a, pitch, off):
        """the (lines, samples) array at `off` of a buffer, lines `pitch` apart"""
        lines, n = a.shape
        buf = np.full(off + lines * pitch + 8, FILL, np.uint16)
        buf[off:off + lines * pitch].reshape(lines, pitch)[:, :n] = a
        return _cuda(buf)

    aligned_low = _low(ctx, _cuda(P), w, h).cpu().numpy()
    for (po, pp), (mo, mp), (lo, lp), (do, dp) in (((1, 4 * w + 1), (0, 4 * w), (0, w), (0, 16 * w)), ((0, 4 * w), (3, 4 * w + 2), (0, w), (0, 16 * w)),
                                                     ((0, 4 * w), (0, 4 * w), (1, w + 3), (1, 16 * w)), ((0, 4 * w), (0, 4 * w), (0, w), (0, 16 * w + 4)),
                                                     ((3, 4 * w + 3), (1, 4 * w + 1), (1, w + 1), (5, 16 * w + 7))):
        pan, mss, low = pitched(P, pp, po), pitched(M.reshape(h, 4 * w), mp, mo), pitched(aligned_low, lp, lo)
        dst = torch.full((do + 4 * h * dp + 8,), FILL, dtype=torch.int16, device="cuda").view(torch.uint16)
        st = torch.zeros(2, dtype=torch.int64, device="cuda")
        ctx.pansharpen_sfim_u16(pan[po:], mss[mo:], low[lo:], w, h, dst[do:], 4, st, pan_pitch=pp, mss_pitch=mp, low_pitch=lp, dst_pitch=dp)
        ctx.sync()
        d = dst.cpu().numpy()
        body = d[do:do + 4 * h * dp].reshape(4 * h, dp)
        assert np.array_equal(body[:, :16 * w].reshape(want.shape), want), (po, pp, mo, mp, lo, lp, do, dp)
        assert (body[:, 16 * w:] == FILL).all() and (d[:do] == FILL).all() and (d[do + 4 * h * dp:] == FILL).all()
        assert tuple(int(v) for v in st.cpu().numpy()) == wcounts


def test_zero_pan_blocks(ctx):
    """PAN is zero on a region of MSS cells: UL == 0 inside it, the gain is 1 there and the first counter says how often"""
    w, h = 67, 9
    P, M = _data(w, h, "bits12")
    P = P.copy()
    P[8:32, 40:120] = 0
    P[:, :8] = 0
    want, wcounts = ref.fuse(P, M)
    got, counts = _fuse(ctx, P, M)
    assert wcounts[0] > 300 and np.array_equal(got, want) and counts == wcounts
    UL = ref.upsample(ref.box4(P))
    assert np.array_equal(got[UL == 0], ref.plain(M)[UL == 0])


@pytest.mark.parametrize("G", [1, 64])
@pytest.mark.parametrize("w,h", [(67, 9), (300, 35)])
def test_gain_limits(ctx, w, h, G):
    P, M = _data(w, h, "contrast")
    got, counts = _fuse(ctx, P, M, G=G)
    want, wcounts = _want(w, h, "contrast", G)
    assert np.array_equal(got, want) and counts == wcounts
    assert 0 < _want(w, h, "contrast", 64)[1][1] < _want(w, h, "contrast", 4)[1][1] < _want(w, h, "contrast", 1)[1][1]      # the limits bite
    assert not np.array_equal(want, _want(w, h, "contrast", 4)[0])


def test_stats_null_and_added_into(ctx):
    import torch
    w, h = 67, 9
    P, M = _data(w, h, "contrast")
    want, wcounts = _want(w, h, "contrast")
    got, none = _fuse(ctx, P, M, stats=False)
    assert none is None and np.array_equal(got, want)
    pan, mss = _cuda(P), _cuda(M)
    low = _low(ctx, pan, w, h)
    out = torch.zeros(4 * h, 4 * w, 4, dtype=torch.uint16, device="cuda")
    st = torch.tensor([5, 1 << 40], dtype=torch.int64, device="cuda")
    for _ in range(2):
        ctx.pansharpen_sfim_u16(pan, mss, low, w, h, out, 4, st)
    ctx.sync()
    assert tuple(int(v) for v in st.cpu().numpy()) == (5 + 2 * wcounts[0], (1 << 40) + 2 * wcounts[1])


def test_invalid_arguments(ctx):
    import torch
    w, h = 16, 5
    P, M = _data(w, h, "full")
    pan, mss = _cuda(P), _cuda(M)
    low = _low(ctx, pan, w, h)
    out = torch.zeros(4 * h, 4 * w, 4, dtype=torch.uint16, device="cuda")
    st = torch.zeros(2, dtype=torch.int64, device="cuda")
    ok = dict(pan=pan, mss=mss, low=low, w=w, h=h, dst=out, max_gain=4, stats=st)
    ctx.pansharpen_sfim_u16(**ok)                                 # the base case is valid
    ctx.pansharpen_sfim_u16(**dict(ok, out_row0=7, out_rows=0))   # no output lines: a no-op
    ctx.pansharpen_sfim_u16(**dict(ok, out_row0=4 * h, out_rows=0))
    ctx.sync()
    assert np.array_equal(out.cpu().numpy(), _want(w, h, "full")[0])
    bad = [dict(pan=None), dict(mss=None), dict(low=None), dict(dst=None),
           dict(pan=pan.data_ptr() + 1), dict(mss=mss.data_ptr() + 1), dict(low=low.data_ptr() + 1), dict(dst=out.data_ptr() + 1),
           dict(stats=st.data_ptr() + 4),
           dict(pan_pitch=4 * w - 1), dict(mss_pitch=4 * w - 1), dict(low_pitch=w - 1), dict(dst_pitch=16 * w - 1),
           dict(w=0), dict(h=0), dict(w=-3), dict(out_row0=-1, out_rows=2), dict(out_row0=4 * h - 1, out_rows=2), dict(out_rows=4 * h + 1),
           dict(out_row0=4 * h + 1, out_rows=0), dict(out_rows=-1), dict(max_gain=0), dict(max_gain=65), dict(max_gain=-4),
           dict(dst=pan), dict(dst=mss), dict(dst=low), dict(dst=pan.data_ptr() + 8 * w * (4 * h - 1)),     # the product's first line on PAN's last
           dict(dst=out, pan=out.data_ptr() + 2 * (16 * w * 4 * h - 4 * w)), dict(stats=out.data_ptr() + 64)]
    for kw in bad:
        with pytest.raises(ValueError):
            ctx.pansharpen_sfim_u16(**dict(ok, **kw))
    ctx.sync()
