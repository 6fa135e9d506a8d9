"""GPU: the peak search of the spectral correlation route skips the inverse column passes of lane tiles that cannot
hold a maximum -- and changes no bit of any result.

After the inverse row transform, column x of an output array can hold no surface value above B(x) = sum_ky |Re| + |Im|
of its entries; tiles whose bound lies below a value already found are not transformed.  Every case runs
interband_correlate_units on 3000-column units twice, as it is and with OIP_PEAK_PRUNE=0 (every tile searched, through
the same kernels), and compares the bits; oip_peak_prune_stats tells how many tiles were searched.  Line counts: 64
(one column pass, 32-column tiles), 400 (two generic column passes) and, once, 16000 (the specialised 125- and 128-point
passes of the BASELINE shape, 16-column tiles)."""
import functools
import os

import numpy as np
import pytest

import _synth

pytestmark = pytest.mark.gpu

SHIFTS = [(2, -1), (1, 1), (-1, -2), (-2, 1)]
N = 3000


def _cuda(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()            # a copy: the shared scenes are read-only


@functools.lru_cache(maxsize=None)
def _scene(rows, seed, W=9000):
    """the scenes of test_spectral_upsampling_route_equals_the_image_route (read-only, shared by the cases)"""
    pan, bands = _synth.pan_mss(rows, W, SHIFTS, seed=seed)
    pan.setflags(write=False)
    for b in bands:
        b.setflags(write=False)
    return pan, bands


def _units_of(pan, bands, n):
    """n units as device windows of one raster (pitch W)"""
    W = pan.shape[1]
    dpan, dplanes = _cuda(pan), [_cuda(b) for b in bands]
    pp = [dpan[:, N * u:] for u in range(n)]
    bp = [[dplanes[b][:, N // 4 * u:] for b in range(4)] for u in range(n)]
    return pp, [W] * n, bp, [W // 4] * n, (dpan, dplanes)


def _both(ctx, pp, qp, bp, qb, rows):
    """(result, exhaustive result, (tiles searched, tiles in all) of the first)"""
    ctx.peak_prune_stats()
    got = ctx.interband_correlate_units(pp, qp, bp, qb, rows, N)
    stats = ctx.peak_prune_stats()
    os.environ["OIP_PEAK_PRUNE"] = "0"
    try:
        full = ctx.interband_correlate_units(pp, qp, bp, qb, rows, N)
    finally:
        os.environ.pop("OIP_PEAK_PRUNE", None)
    fs = ctx.peak_prune_stats()
    assert fs[0] == fs[1] == stats[1] > 0, (fs, stats)          # the switch searched every tile of the same arrays
    return got, full, stats


@pytest.mark.parametrize("rows,seed", [(64, 4), (400, 5)])
def test_pair_plus_single_unit_prunes_and_keeps_the_bits(ctx, rows, seed):
    pan, bands = _scene(rows, seed)
    pp, qp, bp, qb, keep = _units_of(pan, bands, 3)
    got, full, (searched, total) = _both(ctx, pp, qp, bp, qb, rows)
    print("rows %d: %d of %d tiles searched" % (rows, searched, total))
    assert np.isfinite(got).all(), got
    assert np.array_equal(got, full)
    # a condition, not a measurement: on the CPU these scenes need 1 to 2 of 188 16-column tiles per surface
    assert searched <= total / 4, (searched, total)


@pytest.mark.parametrize("s", [0, 1, 15, 16, 17, -1, -2, 31, 32, 33])
def test_peak_column_at_tile_edges_and_wrapping_through_column_zero(ctx, s):
    """The PAN window rolled by s columns moves the peak column by s: onto the edges of 16- and 32-column tiles and
    through column 0 / N - 1, so that the 5 x 5 window reaches into the neighbour tile (the unrolled scenes peak at
    columns 0 .. 2 and 2998, 2999 already)."""
    rows = 64
    pan, bands = _scene(rows, 4)
    win = np.roll(pan[:, :N], s, axis=1)
    pp, bp = [_cuda(win)], [[_cuda(b[:, :N // 4]) for b in bands]]
    got, full, (searched, total) = _both(ctx, pp, [N], bp, [N // 4], rows)
    print("s %d: %d of %d tiles searched, dx %s" % (s, searched, total, got[0, :, 0]))
    assert np.array_equal(got, full)
    assert searched <= total / 4, (searched, total)


def test_no_peak_searches_every_tile(ctx):
    """PAN and bands of independent noise: the bound exceeds every surface value, nothing is pruned"""
    rows = 64
    rng = np.random.default_rng(11)
    pan = rng.integers(0, 4096, (rows, 2 * N), dtype=np.uint16)
    bands = [rng.integers(0, 4096, (rows // 4, 2 * N // 4), dtype=np.uint16) for _ in range(4)]
    pp, qp, bp, qb, keep = _units_of(pan, bands, 2)
    got, full, (searched, total) = _both(ctx, pp, qp, bp, qb, rows)
    assert np.array_equal(got, full)
    assert searched == total, (searched, total)


def test_two_peaks_of_near_equal_height(ctx):
    """a PAN window that repeats with period 1500 correlates at two columns 1500 apart"""
    rows = 64
    pan, bands = _scene(rows, 4)
    win = np.tile(pan[:, :N // 2], (1, 2))
    pp, bp = [_cuda(win)], [[_cuda(b[:, :N // 4]) for b in bands]]
    got, full, stats = _both(ctx, pp, [N], bp, [N // 4], rows)
    assert np.array_equal(got, full)


@pytest.mark.parametrize("kind", ["constant", "ramp"])
def test_degenerate_inputs_equal_the_exhaustive_search(ctx, kind):
    """constant images (0 / 0 in every bin) and the +-1000 DN ramp of test_gpu_overflow.py (an overflowing interior bin):
    whatever NaN or zero response the exhaustive search reports, this one reports"""
    rows = 64
    if kind == "constant":
        pan = np.full((rows, N), 1000, np.uint16)
        bands = [np.full((rows // 4, N // 4), 1000 + 10 * b, np.uint16) for b in range(4)]
    else:
        pan, bands = _scene(rows, 4)
        ramp = np.linspace(-1000.0, 1000.0, N)
        small = ramp.reshape(N // 4, 4).mean(axis=1)
        pan = np.clip(np.rint(pan[:, :N] + ramp), 0, 65535).astype(np.uint16)
        bands = [np.clip(np.rint(b[:, :N // 4] + small), 0, 65535).astype(np.uint16) for b in bands]
    pp, bp = [_cuda(pan)], [[_cuda(b) for b in bands]]
    got, full, stats = _both(ctx, pp, [N], bp, [N // 4], rows)
    print(kind, got[0], stats)
    assert np.array_equal(got, full, equal_nan=True)


def test_unit_counts_and_repeated_calls(ctx):
    """one unit (two output arrays), five units (two pairs plus one), and the same call again on the same context: the
    workspace, the flags and the lists start clean"""
    rows = 64
    pan, bands = _synth.pan_mss(rows, 5 * N, SHIFTS, seed=7)
    pp, qp, bp, qb, keep = _units_of(pan, bands, 5)
    five, five_full, (searched, total) = _both(ctx, pp, qp, bp, qb, rows)
    assert np.array_equal(five, five_full)
    assert total == 10 * ((N + 31) // 32) and searched <= total / 4, (searched, total)
    one, one_full, (s1, t1) = _both(ctx, pp[:1], qp[:1], bp[:1], qb[:1], rows)
    assert np.array_equal(one, one_full)
    assert t1 == 2 * ((N + 31) // 32) and s1 <= t1 / 4, (s1, t1)
    again, again_full, st = _both(ctx, pp, qp, bp, qb, rows)
    assert np.array_equal(again, five) and np.array_equal(again_full, five) and st == (searched, total)


def test_baseline_shape_prunes_and_keeps_the_bits(ctx):
    """16000 lines: the 125-point pass and the register-staged 128-point peak pass over tile lists, 16-column tiles (one
    unit: most of this test's time is the scene's synthesis on the CPU)"""
    rows = 16000
    pan, bands = _synth.pan_mss(rows, N, SHIFTS, seed=9)
    pp, qp, bp, qb, keep = _units_of(pan, bands, 1)
    got, full, (searched, total) = _both(ctx, pp, qp, bp, qb, rows)
    print("rows %d: %d of %d tiles searched" % (rows, searched, total))
    assert np.isfinite(got).all(), got
    assert np.array_equal(got, full)
    assert total == 2 * 188 and searched <= total / 4, (searched, total)
