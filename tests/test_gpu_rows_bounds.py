"""GPU: the row stage of the spectral correlation sums its column bounds in registers and writes each workgroup's four
rows once, after its last line pair ("Sums") -- and changes no bit of any result, nor which tiles the
pruned peak search lists.

Before, the sums were added to memory with the hardware's f32 add and a memset cleared the rows in front of every launch.
The register sums are the same additions in the same order, so the tile counts of the peak search
(oip_peak_prune_stats) must equal what the parent commit counted for the same scenes: they are constants below.  Scenes
and helpers are those of tests/test_gpu_rows_window.py (3000 columns).  Line counts: 64 and 400 give every workgroup one
line pair (M / 2 + 1 <= CUs); 1600 gives the 256 workgroups three or four line pairs each (801 = 3 * 256 + 33), so the
sums are carried over iterations and the lines come through the prefetch; a PAN window rolled by half a row sends the same
line count through the instance that stores every column."""
import numpy as np
import pytest

from test_gpu_rows_window import N, _cuda, _scene, _units_of, _with_env

pytestmark = pytest.mark.gpu

# (tiles searched, tiles in all) of the call as built, printed by the parent commit 72f2221 for the same scenes (three
# units: a pair and a single).  Equality is expected: if a count differs, find out why before changing the constant.
PARENT_TILES = {
    (64, 4, 0): (12, 564),
    (400, 5, 0): (12, 564),
    (1600, 5, 0): (12, 564),
    (1600, 5, 1500): (6, 564),
}


def _units(rows, seed, roll):
    """three units of the scene; roll: columns every PAN window is rolled by (1500: the peaks miss the stored window)"""
    pan, bands = _scene(rows, seed)
    pp, qp, bp, qb, keep = _units_of(pan, bands, 3)
    if roll:
        pp = [_cuda(np.roll(pan[:, N * u:N * (u + 1)], roll, axis=1)) for u in range(3)]
        qp = [N] * 3
    return pp, qp, bp, qb, keep


def measure(ctx, rows, seed, roll):
    """the call as built, with every tile searched (OIP_PEAK_PRUNE=0) and with every column stored (OIP_ROWS_WINDOW=0):
    results, tile counts, (pairs, pairs run again) and the window's geometry"""
    pp, qp, bp, qb, keep = _units(rows, seed, roll)
    run = lambda: ctx.interband_correlate_units(pp, qp, bp, qb, rows, N)
    ctx.rows_window_stats()
    ctx.peak_prune_stats()
    got = run()
    ws, ps, geom = ctx.rows_window_stats(), ctx.peak_prune_stats(), ctx.rows_window_geometry()
    exhaustive = _with_env("OIP_PEAK_PRUNE", "0", run)
    ps_ex = ctx.peak_prune_stats()
    full_store = _with_env("OIP_ROWS_WINDOW", "0", run)
    ps_full = ctx.peak_prune_stats()
    print("rows %d seed %d roll %d: window %s, pairs/rerun %s, tiles searched/total %s (exhaustive %s, full store %s)"
          % (rows, seed, roll, geom, ws, ps, ps_ex, ps_full))
    return dict(got=got, exhaustive=exhaustive, full_store=full_store, ps=ps, ps_ex=ps_ex, ps_full=ps_full, ws=ws, geom=geom)


def _check(m, rows, seed, roll, rerun):
    V, T, R = m["geom"]
    assert T > 0 and R > 0, "no tile lists / no stored window at %d lines: %s" % (rows, (V, T, R))
    assert np.isfinite(m["exhaustive"]).all(), m["exhaustive"]
    assert np.array_equal(m["got"], m["exhaustive"])
    assert np.array_equal(m["got"], m["full_store"])
    assert m["ws"] == (2, rerun), m["ws"]
    # three units, two output arrays each: the exhaustive search lists every tile of every array
    assert m["ps_ex"] == (6 * T, 6 * T), (m["ps_ex"], T)
    assert m["ps"] == m["ps_full"], (m["ps"], m["ps_full"])
    assert m["ps"] == PARENT_TILES[(rows, seed, roll)], (m["ps"], PARENT_TILES[(rows, seed, roll)])


@pytest.mark.parametrize("rows,seed", [(64, 4), (400, 5)])
def test_one_line_pair_per_workgroup(ctx, rows, seed):
    """a pair (four outputs) and a single unit (two): nothing is carried over iterations"""
    _check(measure(ctx, rows, seed, 0), rows, seed, 0, rerun=0)


def test_sums_carried_over_iterations_and_prefetched_lines(ctx):
    """1600 lines: 801 line pairs over 256 workgroups, three or four each -- more than two rounds, not a multiple"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    pairs = 1600 // 2 + 1
    assert pairs > 2 * cus and pairs % cus, (pairs, cus)
    _check(measure(ctx, 1600, 5, 0), 1600, 5, 0, rerun=0)


def test_sums_carried_over_iterations_with_every_column_stored(ctx):
    """the same line count with peaks half a row away: both groups miss the window and run again through the instance
    that stores every column"""
    _check(measure(ctx, 1600, 5, 1500), 1600, 5, 1500, rerun=2)


def test_unpaired_lines_count_once(ctx):
    """ky = 0 and ky = M / 2 have no mirror line: their |Re| + |Im| enters the bound once (the mirror slot of LDS holds
    zeros then, and the kernel skips it).  Left out, the bound would stop being one -- at 64 lines the two lines are 1/32
    of the terms, eight times the selection's margin of 2^-8 -- and a tile holding a maximum could go unsearched; counted
    twice, more tiles than the parent's would be listed.  The parent's tile count and the exhaustive search's bits, on
    the single unit (two outputs) as on the pair, are the check."""
    rows, seed = 64, 4
    pan, bands = _scene(rows, seed)
    pp, qp, bp, qb, keep = _units_of(pan, bands, 3)
    run = lambda k: ctx.interband_correlate_units(pp[k:], qp[k:], bp[k:], qb[k:], rows, N)
    for k in (0, 2):                                    # pair + single, single alone
        ctx.peak_prune_stats()
        got = run(k)
        ps = ctx.peak_prune_stats()
        ref = _with_env("OIP_PEAK_PRUNE", "0", lambda: run(k))
        ctx.peak_prune_stats()
        assert np.array_equal(got, ref)
        if k == 0:
            assert ps == PARENT_TILES[(rows, seed, 0)], ps


@pytest.mark.parametrize("order", ["two_then_one", "one_then_two"])
def test_no_stale_rows_without_the_memset(ctx, order):
    """a two-unit call on scene A (four outputs) and a one-unit call on scene B (two: rows 2 and 3 of every workgroup must
    read as zero, not as A's sums) in one context, in both orders: each equals what a fresh context returns for it alone"""
    import torch
    import opticalimageprocessor_amd as oip
    rows = 64
    (panA, bandsA), (panB, bandsB) = _scene(rows, 4), _scene(rows, 7)
    ppA, qpA, bpA, qbA, keepA = _units_of(panA, bandsA, 2)
    ppB, qpB, bpB, qbB, keepB = _units_of(panB, bandsB, 1)
    calls = {"two": (ppA, qpA, bpA, qbA), "one": (ppB, qpB, bpB, qbB)}

    def call(c, name):
        pp, qp, bp, qb = calls[name]
        c.peak_prune_stats()
        return c.interband_correlate_units(pp, qp, bp, qb, rows, N), c.peak_prune_stats()

    fresh = {}
    for name in calls:
        c = oip.Context(0)
        try:
            c.set_stream(torch.cuda.current_stream())
            fresh[name] = call(c, name)
        finally:
            torch.cuda.synchronize()
            c.close()
    for name in (["two", "one"] if order == "two_then_one" else ["one", "two"]):
        got, ps = call(ctx, name)
        assert np.isfinite(got).all()
        assert np.array_equal(got, fresh[name][0]), name
        assert ps == fresh[name][1], (name, ps, fresh[name][1])
