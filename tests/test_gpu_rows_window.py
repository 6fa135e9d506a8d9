"""GPU: the row stage of the pruned spectral correlation stores only a circular window of lane tiles around column 0
("stored window") -- and changes no bit of any result.

The pruned peak search reads a handful of lane tiles of each output array, and for inter-band shifts of a few pixels they
lie at column 0 or across the wrap; the row stage stores the tiles 0 .. R and T - R .. T - 1 only.  A pair of units whose
search lists a tile outside of that window (or next to its end: the column passes run on a tile's two neighbours as well)
is flagged on the device and run again inside the same call with every column stored.  Every case runs
interband_correlate_units on 3000-column units three times -- as built, with OIP_ROWS_WINDOW=0 (every column stored: the
reference) and with OIP_ROWS_WINDOW_POISON=1 (NaN wherever the row stage does not store) -- and compares the bits;
oip_rows_window_stats tells how many pairs were run again, oip_peak_prune_stats must count every pair once.  Line counts:
64 (32-column tiles), 400 (two generic column passes) and 16000 (16-column tiles, the 125- and 128-point list passes)."""
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
    """the scenes of tests/test_gpu_peak_prune.py (read-only, shared by the cases)"""
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


def _with_env(name, value, f):
    os.environ[name] = value
    try:
        return f()
    finally:
        os.environ.pop(name, None)


def _three(ctx, pp, qp, bp, qb, rows):
    """(result, (pairs, pairs run again), (tiles searched, tiles in all), (tile columns, tiles, radius)) of the call as
    built, after comparing it with the full store and with itself over poisoned arrays"""
    run = lambda: ctx.interband_correlate_units(pp, qp, bp, qb, rows, N)
    ctx.rows_window_stats()
    ctx.peak_prune_stats()
    got = run()
    ws, ps, geom = ctx.rows_window_stats(), ctx.peak_prune_stats(), ctx.rows_window_geometry()
    ref = _with_env("OIP_ROWS_WINDOW", "0", run)
    assert ctx.rows_window_geometry()[2] == -1
    assert ctx.rows_window_stats() == (0, 0)
    ps_ref = ctx.peak_prune_stats()
    poisoned = _with_env("OIP_ROWS_WINDOW_POISON", "1", run)
    ws_p, ps_p = ctx.rows_window_stats(), ctx.peak_prune_stats()
    print("rows %d: window %s, pairs/rerun %s, tiles searched/total %s (full store %s)" % (rows, geom, ws, ps, ps_ref))
    assert np.isfinite(ref).all(), ref
    assert np.array_equal(got, ref)
    assert np.array_equal(poisoned, ref)
    assert ps == ps_ref == ps_p, (ps, ps_ref, ps_p)         # a pair that is run again is counted once
    assert ws == ws_p, (ws, ws_p)
    return got, ws, ps, geom


def _geometry(ctx, rows):
    """(tile columns V, tiles T, radius R) of the window at this line count"""
    pan, bands = _scene(64, 4) if rows == 64 else _scene(rows, 5)
    ctx.interband_correlate_units([_cuda(pan[:, :N])], [N], [[_cuda(b[:, :N // 4]) for b in bands]], [N // 4], rows, N)
    V, T, R = ctx.rows_window_geometry()
    assert V >= 2 and T == (N + V - 1) // V and 0 < R and 2 * R + 1 < T, (V, T, R)
    stored = (R + 1) * V + N - (T - R) * V
    print("rows %d: tiles of %d columns, R = %d: %d of %d columns stored" % (rows, V, R, stored, N))
    return V, T, R


@pytest.mark.parametrize("rows,seed", [(64, 4), (400, 5)])
def test_scenes_of_the_peak_prune_tests_hit_the_window(ctx, rows, seed):
    pan, bands = _scene(rows, seed)
    pp, qp, bp, qb, keep = _units_of(pan, bands, 3)
    got, (pairs, rerun), (searched, total), geom = _three(ctx, pp, qp, bp, qb, rows)
    assert (pairs, rerun) == (2, 0), (pairs, rerun)
    assert searched <= total / 4, (searched, total)


def test_default_window_stores_under_a_tenth_of_the_columns_of_the_baseline_shape(ctx):
    """16-column tiles at 16000 lines (T = 188): checked on the geometry alone, through a 64-line call for R"""
    V, T, R = _geometry(ctx, 64)
    assert ((R + 1) * 16 + N - (188 - R) * 16) < N / 10, R


# peak tile of the rolled PAN window, as (side, offset): side +1 counts tiles from tile 0 upwards, side -1 from tile T - 1
# downwards through the wrap; offset is relative to the window's radius R.  The column passes run on the peak tile and its
# two neighbours, so the peak tile R - 1 is the last one that hits.
EDGE_CASES = [(+1, -1, False), (+1, 0, True), (+1, 1, True), (-1, -1, False), (-1, 0, True), (-1, 1, True)]


def _roll_onto_tile(V, T, R, side, off):
    """columns to roll the PAN window by so that all four surfaces (peaks within two columns of the roll) peak in the
    middle of tile R + off (side +1) or of tile T - R - off (side -1: the mirror image; tile T - 1 is the partial one)"""
    t = R + off if side > 0 else T - R - off
    col = t * V + V // 2
    return col if side > 0 else col - N


@pytest.mark.parametrize("side,off,miss", EDGE_CASES)
def test_peak_tile_at_the_ends_of_the_window(ctx, side, off, miss):
    rows = 64
    V, T, R = _geometry(ctx, rows)
    s = _roll_onto_tile(V, T, R, side, off)
    pan, bands = _scene(rows, 4)
    win = np.roll(pan[:, :N], s, axis=1)
    pp, bp = [_cuda(win)], [[_cuda(b[:, :N // 4]) for b in bands]]
    got, (pairs, rerun), (searched, total), geom = _three(ctx, pp, [N], bp, [N // 4], rows)
    print("s %d: dx %s" % (s, got[0, :, 0]))
    assert (pairs, rerun) == (1, 1 if miss else 0), (s, pairs, rerun)
    assert searched <= total / 4, (searched, total)


def test_peak_half_a_window_away_is_a_miss(ctx):
    rows = 64
    pan, bands = _scene(rows, 4)
    win = np.roll(pan[:, :N], 1500, axis=1)
    pp, bp = [_cuda(win)], [[_cuda(b[:, :N // 4]) for b in bands]]
    got, ws, (searched, total), geom = _three(ctx, pp, [N], bp, [N // 4], rows)
    assert ws == (1, 1), ws
    assert searched <= total / 4, (searched, total)


def test_only_the_single_unit_misses(ctx):
    """three units, the PAN window of the last one rolled far away: the pair is not run again and keeps its bits"""
    rows = 64
    pan, bands = _scene(rows, 4)
    pp, qp, bp, qb, keep = _units_of(pan, bands, 3)
    pair = ctx.interband_correlate_units(pp[:2], qp[:2], bp[:2], qb[:2], rows, N)
    pp[2] = _cuda(np.roll(pan[:, 2 * N:3 * N], 1500, axis=1))
    qp[2] = N
    got, ws, ps, geom = _three(ctx, pp, qp, bp, qb, rows)
    assert ws == (2, 1), ws
    assert np.array_equal(got[:2], pair)


def test_no_peak_runs_every_pair_again_and_counts_it_once(ctx):
    """PAN and bands of independent noise (test_no_peak_searches_every_tile): every tile is listed"""
    rows = 64
    rng = np.random.default_rng(11)
    pan = rng.integers(0, 4096, (rows, 3 * N), dtype=np.uint16)
    bands = [rng.integers(0, 4096, (rows // 4, 3 * N // 4), dtype=np.uint16) for _ in range(4)]
    pp, qp, bp, qb, keep = _units_of(pan, bands, 3)
    got, ws, (searched, total), (V, T, R) = _three(ctx, pp, qp, bp, qb, rows)
    assert ws == (2, 2), ws
    assert searched == total == 6 * T, (searched, total, T)


def test_second_peak_outside_the_window_is_a_miss(ctx):
    """a PAN window that repeats with period 1500 correlates at two columns 1500 apart: the first round's tile is
    inside the window or not, the second round lists the other one"""
    rows = 64
    pan, bands = _scene(rows, 4)
    win = np.tile(pan[:, :N // 2], (1, 2))
    pp, bp = [_cuda(win)], [[_cuda(b[:, :N // 4]) for b in bands]]
    got, ws, ps, geom = _three(ctx, pp, [N], bp, [N // 4], rows)
    assert ws == (1, 1), ws


def test_calls_in_a_row_do_not_see_each_others_window(ctx):
    """hit, miss, another hit elsewhere in the window, the first again: what a call left in the arrays outside its window
    (and inside it) is not the next call's data"""
    rows = 64
    pan, bands = _scene(rows, 4)
    V, T, R = _geometry(ctx, rows)
    bp = [[_cuda(b[:, :N // 4]) for b in bands]]
    wins = [_cuda(np.roll(pan[:, :N], s, axis=1)) for s in (0, 1500, 2 * V + V // 2, 0)]
    run = lambda w: ctx.interband_correlate_units([w], [N], bp, [N // 4], rows, N)
    refs = _with_env("OIP_ROWS_WINDOW", "0", lambda: [run(w) for w in wins])
    ctx.rows_window_stats()
    gots = [run(w) for w in wins]
    assert ctx.rows_window_stats() == (4, 1)
    poisoned = _with_env("OIP_ROWS_WINDOW_POISON", "1", lambda: [run(w) for w in wins])
    assert ctx.rows_window_stats() == (4, 1)
    for g, p, r in zip(gots, poisoned, refs):
        assert np.isfinite(r).all()
        assert np.array_equal(g, r) and np.array_equal(p, r)
    assert np.array_equal(gots[0], gots[3]) and not np.array_equal(gots[0], gots[2])


def test_exhaustive_search_stores_every_column(ctx):
    rows = 64
    pan, bands = _scene(rows, 4)
    pp, qp, bp, qb, keep = _units_of(pan, bands, 3)
    run = lambda: ctx.interband_correlate_units(pp, qp, bp, qb, rows, N)
    ref = _with_env("OIP_ROWS_WINDOW", "0", run)
    ctx.rows_window_stats()
    ctx.peak_prune_stats()
    got = _with_env("OIP_PEAK_PRUNE", "0", run)
    assert ctx.rows_window_geometry()[2] == -1
    assert ctx.rows_window_stats() == (0, 0)
    searched, total = ctx.peak_prune_stats()
    assert searched == total > 0
    assert np.isfinite(ref).all() and np.array_equal(got, ref)
    # poisoned arrays: every column must have been written by the row stage itself
    poisoned = _with_env("OIP_ROWS_WINDOW_POISON", "1", lambda: _with_env("OIP_PEAK_PRUNE", "0", run))
    assert ctx.rows_window_stats() == (0, 0) and ctx.peak_prune_stats() == (searched, total)
    assert np.array_equal(poisoned, ref)


@functools.lru_cache(maxsize=None)
def _baseline_scene():
    pan, bands = _synth.pan_mss(16000, N, SHIFTS, seed=9)
    pan.setflags(write=False)
    for b in bands:
        b.setflags(write=False)
    return pan, bands


@pytest.mark.parametrize("off,miss", [(-1, False), (0, True)])
def test_baseline_shape(ctx, off, miss):
    """16000 lines, 16-column tiles, the 125- and 128-point list passes: the peak tile R - 1 hits, R misses (one unit: most
    of this test's time is the scene's synthesis on the CPU, shared by the two cases)"""
    rows = 16000
    pan, bands = _baseline_scene()
    dbands = [[_cuda(b) for b in bands]]
    ctx.interband_correlate_units([_cuda(pan)], [N], dbands, [N // 4], rows, N)
    V, T, R = ctx.rows_window_geometry()
    assert (V, T) == (16, 188) and R > 0, (V, T, R)
    s = _roll_onto_tile(V, T, R, +1, off)
    got, ws, (searched, total), geom = _three(ctx, [_cuda(np.roll(pan, s, axis=1))], [N], dbands, [N // 4], rows)
    assert ws == (1, 1 if miss else 0), (s, ws)
    assert total == 2 * 188 and searched <= total / 4, (searched, total)
