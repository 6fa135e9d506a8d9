"""GPU: oip_colstats_u16 -- per-column count / sum / sum of squares -- against numpy's integer sums.  The sums are exact
integers, so every comparison is equality of all 3*w values."""
import numpy as np
import pytest

from _colstats_ref import totals

pytestmark = pytest.mark.gpu


def _acc(w):
    import torch
    return torch.zeros(3, w, dtype=torch.int64, device="cuda")        # the bits of the library's uint64 planes


def _host(acc):
    return acc.cpu().numpy().view(np.uint64)


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _random(rows, w, seed, lo=0, hi=65536):
    return np.random.default_rng(seed).integers(lo, hi, (rows, w), dtype=np.uint16)


@pytest.mark.parametrize("rows,w", [(3200, 1280), (4096, 30000), (777, 4093)])
def test_exact_totals_whole_raster(ctx, rows, w):
    """1280 x 3200; 30000 px lines (60000 B: 16-byte but not 128-byte aligned); a width that is not a multiple of 8"""
    img = _random(rows, w, 100 + w)
    acc = _acc(w)
    ctx.colstats_u16(_cuda(img), w, w, rows, acc)
    ctx.sync()
    assert np.array_equal(_host(acc), totals(img))


@pytest.mark.parametrize("col0,w", [(3, 1000), (8, 1000), (16, 4077)])
def test_exact_totals_window(ctx, col0, w):
    """a window of a 4096-wide raster (pitch > w): misaligned start; aligned start with w % 8 == 0; aligned start whose
    last 8-column group is partial (the vector kernel reads, and must not count, the 3 columns behind the window)"""
    rows, pitch = 1500, 4096
    img = _random(rows, pitch, 5)
    d = _cuda(img)
    acc = _acc(w)
    ctx.colstats_u16(d.data_ptr() + 2 * col0, pitch, w, rows, acc)
    ctx.sync()
    assert np.array_equal(_host(acc), totals(img[:, col0:col0 + w]))


def test_exact_totals_beyond_32_bits(ctx):
    """2048 x 70000 of constant 65535: S1 > 2^32, S2 > 2^48, more lines than one row block may hold (65536)"""
    import torch
    rows, w = 70000, 2048
    d = torch.full((rows, w), -1, dtype=torch.int16, device="cuda").view(torch.uint16)
    acc = _acc(w)
    ctx.colstats_u16(d, w, w, rows, acc)
    ctx.sync()
    got = _host(acc)
    assert (got[0] == rows).all() and (got[1] == rows * 65535).all() and (got[2] == rows * 65535 * 65535).all()
    assert rows * 65535 > 2 ** 32 and rows * 65535 * 65535 > 2 ** 48


def test_no_rows_leaves_the_totals(ctx):
    img = _random(64, 256, 3)
    acc = _acc(256)
    ctx.colstats_u16(_cuda(img), 256, 256, 64, acc)
    ctx.colstats_u16(_cuda(img), 256, 256, 0, acc)
    ctx.sync()
    assert np.array_equal(_host(acc), totals(img))
    with pytest.raises(ValueError):
        ctx.colstats_u16(_cuda(img), 100, 256, 64, acc)            # pitch < w
    with pytest.raises(ValueError):
        ctx.colstats_u16(_cuda(img), 256, 256, 64, acc, 5, 4)      # empty valid range


@pytest.mark.parametrize("w", [2048, 1001])
def test_valid_range(ctx, w):
    """[64, 4095] on data that holds 0 and 65535 (and both bounds): masked sums, n differs between columns"""
    rows = 1333
    rng = np.random.default_rng(17)
    img = rng.integers(0, 8192, (rows, w), dtype=np.uint16)
    img[rng.random((rows, w)) < 0.05] = 0
    img[rng.random((rows, w)) < 0.05] = 65535
    img[0, :4] = (63, 64, 4095, 4096)
    acc = _acc(w)
    ctx.colstats_u16(_cuda(img), w, w, rows, acc, 64, 4095)
    ctx.sync()
    got = _host(acc)
    assert np.array_equal(got, totals(img, 64, 4095))
    assert len(np.unique(got[0])) > 1 and got[0].max() < rows


def test_additive_over_calls(ctx):
    rows, w = 5001, 12288
    img = _random(rows, w, 23, 0, 4096)
    d = _cuda(img)
    whole, halves = _acc(w), _acc(w)
    ctx.colstats_u16(d, w, w, rows, whole)
    ctx.colstats_u16(d.data_ptr() + 2 * w * 2500, w, w, rows - 2500, halves)      # order of the calls does not matter
    ctx.colstats_u16(d, w, w, 2500, halves)
    ctx.sync()
    assert np.array_equal(_host(whole), _host(halves)) and np.array_equal(_host(whole), totals(img))


def test_bil_mss_totals_are_the_four_planes(ctx):
    """column x of a BIL line is column x % (W/4) of band x / (W/4): one call on the raw MSS raster gives the statistics of
    the four planes the existing split (d_kb4 = NULL) produces"""
    import torch
    W, lines = 1280, 900
    bw = W // 4
    bil = _cuda(_random(lines, W, 31, 64, 4096))
    planes = torch.zeros(4, lines, bw, dtype=torch.uint16, device="cuda")
    ctx.mss_split_rrc_u16(bil, planes, lines * bw, W, lines, None)
    acc, per = _acc(W), [_acc(bw) for _ in range(4)]
    ctx.colstats_u16(bil, W, W, lines, acc)
    for b in range(4):
        ctx.colstats_u16(planes[b], bw, bw, lines, per[b])
    ctx.sync()
    got = _host(acc).reshape(3, 4, bw)
    for b in range(4):
        assert np.array_equal(got[:, b], _host(per[b]))
        assert np.array_equal(got[:, b], totals(planes[b].cpu().numpy()))


def test_profiler_sees_the_kernel(ctx):
    img = _cuda(_random(256, 512, 1))
    acc = _acc(512)
    ctx.profile_enable(True)
    ctx.profile_reset()
    ctx.colstats_u16(img, 512, 512, 256, acc)
    ctx.sync()
    prof = ctx.profile()
    ctx.profile_enable(False)
    assert prof["colstats_u16_kernel"][1] == 1
