"""GPU: oip_match_tiles_u16 at addresses past 2^31 samples, on the probe raster of tests/_bigraster.py (32760 x 65600 =
2 149 056 000 samples: one constant on every line but a head and a tail band of seeded noise).  A and B are the same buffer;
T = 16, S = 4, so a tile's search window is 24 lines high: one row of tiles has its windows on lines [0, 24), the head band, the
other on lines [65576, 65600), the last of the tail band, all of which lie wholly past 2^31 samples (from line 65553 on).  The
expectation is the restatement on the 48 lines of the two bands, which is all the host needs.  A kernel that computed
`row * pitch` in 32 bits would read lines of the head and of the constant for the second row; the CPU twin at the bottom (not
`gpu`) shows on _bigraster.SMALL that the comparison rejects that."""
import gc

import numpy as np
import pytest

import _bigraster as br
import _regcheck_ref as ref

SEED = 53
T, S = 16, 4
WIN = T + 2 * S


def _grid(geo, nx):
    """(x0, y0, step_x, step_y, nx, 2): nx tiles across the line, the second row's windows ending on the last line"""
    step_x = (geo.W - WIN) // (nx - 1)
    return S, S, step_x, geo.L - WIN, nx, 2


def _expected(geo, noises, grid):
    """the restatement on the head band's first and the tail band's last WIN lines, stacked: the same tiles at step_y = WIN"""
    assert geo.head[1] >= WIN and geo.tail[1] - geo.tail[0] >= WIN
    x = np.concatenate([noises[0][:WIN], noises[1][-WIN:]])
    x0, y0, sx, _, nx, ny = grid
    return ref.match_tiles(x, x, T, S, x0, y0, sx, WIN, nx, ny)


@pytest.mark.gpu
def test_tiles_in_the_head_and_past_2g(ctx):
    """peak device memory: 4.3 GB (the raster)"""
    import torch
    geo = br.BIG
    f = geo.assert_crosses()
    grid = _grid(geo, 8)
    assert grid[1] + grid[3] - S >= f and (grid[1] + grid[3] - S) * geo.W >= br.TWO31      # the second row's windows start past 2^31
    assert grid[0] + 7 * grid[2] + T + S <= geo.W and grid[1] + grid[3] + T + S == geo.L
    noises = [br.band_noise(geo, k, SEED) for k in (0, 1)]
    wrec, wsums, gap = _expected(geo, noises, grid)
    assert gap.min() > 1e-9 and (wrec[:, 4] == S * (2 * S + 1) + S).all() and (wrec[:, 2] > 0).any()
    src = br.device_raster(geo, noises)
    n, K2 = 16, (2 * S + 1) ** 2
    rec = torch.full((n * 20,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    sums = torch.full((n * K2 * 3,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    ctx.match_tiles_u16(src, geo.W, 1, src, geo.W, 1, geo.W, geo.L, T, S, *grid, 1, 65535, rec, sums)
    ctx.sync()
    assert np.array_equal(sums.cpu().numpy().view(np.uint64).reshape(n, K2, 3), wsums)
    assert np.array_equal(rec.cpu().numpy().view(np.uint64).reshape(n, 20), wrec)
    del src
    gc.collect()
    torch.cuda.empty_cache()


def test_check_rejects_a_wrapped_read():
    """the same comparison on the host at _bigraster.SMALL (64 x 240, offsets wrap at element 192 * 64 + 8): the restatement on
    the whole raster equals the expectation made from the bands; on the raster read through a wrapping offset the first row of
    tiles still does, and every tile of the second row differs"""
    geo = br.SMALL
    f = geo.assert_crosses()
    grid = _grid(geo, 3)
    assert grid[1] + grid[3] - S >= f and grid[0] + 2 * grid[2] + T + S <= geo.W
    noises = [br.band_noise(geo, k, SEED) for k in (0, 1)]
    wrec, wsums, _ = _expected(geo, noises, grid)
    x = br.host_raster(geo, noises)
    rec, sums, _ = ref.match_tiles(x, x, T, S, *grid)
    assert np.array_equal(rec, wrec) and np.array_equal(sums, wsums)
    y = br.wrapped_read(x, geo.wrap)
    rec, sums, _ = ref.match_tiles(y, y, T, S, *grid)
    assert np.array_equal(rec[:3], wrec[:3]) and np.array_equal(sums[:3], wsums[:3])
    assert (rec[3:, :2] != wrec[3:, :2]).all() and (sums[3:, :, 2] != wsums[3:, :, 2]).all()
