"""GPU: oip_mask_cells_u16 and oip_mask_morph_u8 against the restatement (_mask_ref.py).  The flag bytes and the counters are
exact integer functions of the samples, so every comparison is equality.  The shapes are the smallest that can go wrong: partial
cells at the right and bottom edge, a last vector that leaves the line, one partial cell, more than one workgroup, the vector and
the cell-per-lane kernel on the same data, grids around the 64-cell word, radii beyond the grid."""
import itertools

import numpy as np
import pytest

import _mask_ref as ref

pytestmark = pytest.mark.gpu
FILL = 0xEE                                                            # what the flag buffer holds before a call: no flag byte (bits 32..128)
KW = dict(valid_min=1, sat_level=4095, full=4095, band=ref.DEFAULT_BAND, q8=ref.DEFAULT_Q8)


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def _cells(ctx, img, spp, C, mode="vector", slack=3, counts=None, **kw):
    """the flags of one call as (gh, gw + slack) uint8 and the 8 counters.  mode: "vector" (a pitch that is a multiple of 8 and an
    aligned base), "pitch" (a pitch that is not), "base" (a base off by one sample)"""
    import torch
    k = dict(KW, **kw)
    rows, ws = img.shape
    w = ws // spp
    pitch = -(-ws // 8) * 8 if mode != "pitch" else -(-ws // 8) * 8 + 3
    off = 1 if mode == "base" else 0
    host = np.full(rows * pitch + 8, 0x7777, np.uint16)                # what lies between the lines is never data
    host[off:off + rows * pitch].reshape(rows, pitch)[:, :ws] = img
    dev = _cuda(host)
    gw, gh = ref.grid(w, rows, C)
    out = torch.full((max(gh, 1), gw + slack), FILL, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(8, dtype=torch.int64, device="cuda") if counts is None else counts
    ctx.mask_cells_u16(dev.data_ptr() + 2 * off, pitch, w, rows, spp, C, out, gw + slack, cnt, k["valid_min"], k["sat_level"], k["full"], k["band"],
                       *k["q8"])
    ctx.sync()
    return out.cpu().numpy(), cnt.cpu().numpy().astype(np.uint64)


def _check(got, counts, want, want_counts):
    gh, gw = want.shape
    assert np.array_equal(got[:gh, :gw], want), "%d of %d flag bytes differ" % (int((got[:gh, :gw] != want).sum()), want.size)
    assert (got[:, gw:] == FILL).all() and (got[gh:] == FILL).all()                      # nothing written beside the flags
    assert np.array_equal(counts, want_counts), (counts, want_counts)


# ---- cells ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,rows,spp", [(202, 77, 4), (203, 77, 1), (8, 8, 4), (8, 8, 1), (3, 3, 4), (3, 3, 1), (1024, 64, 4), (1024, 64, 1)])
@pytest.mark.parametrize("C", [4, 8, 16])
def test_cells_random(ctx, w, rows, spp, C):
    """202 x 77 x 4 and 203 x 77: partial cells right and bottom, at spp 1 a last vector that leaves the line.  8 x 8 and 3 x 3: one
    cell (partial at C 16, and always at 3 x 3).  1024 x 64: the aligned fast path, two workgroups at spp 4.  The same data
    through a pitch that is not a multiple of 8 and through a base off by one sample: the cell-per-lane kernel.  valid_min 0, 1."""
    img = ref.random_raster(rows, w * spp, 31 * w + C + spp)
    seen = 0
    for vmin in (1, 0):
        want, wc = ref.cells(img, spp, C, **dict(KW, valid_min=vmin))
        seen |= int(np.bitwise_or.reduce(want.reshape(-1)))
        assert wc[0] == want.size
        for mode in ("vector", "pitch", "base"):
            got, counts = _cells(ctx, img, spp, C, mode, valid_min=vmin)
            _check(got, counts, want, wc)
    if w >= 200:
        assert seen == (19 if spp == 4 else 3)                          # every bit of a cells call occurs


@pytest.mark.parametrize("C", [4, 8, 16])
def test_cells_at_equality_of_each_test(ctx, C):
    """the crafted cells of _mask_ref.edge_cases: each test alone decides a cell at -1, 0, +1 of equality"""
    img, cases = ref.edge_raster(C)
    kw = dict(sat_level=65535, full=ref.EDGE_FULL, q8=ref.EDGE_Q8)
    want, wc = ref.cells(img, 4, C, **dict(KW, **kw))
    assert [bool(v & ref.CANDIDATE) for v in want[0]] == [k >= 0 for _, k, _ in cases] and len(cases) == 12
    for mode in ("vector", "pitch"):
        _check(*_cells(ctx, img, 4, C, mode, **kw), want, wc)


def test_cells_every_band_permutation_and_every_disabled_test(ctx):
    C = 8
    kw = dict(sat_level=65535, full=ref.EDGE_FULL)
    flags = set()
    for band in itertools.permutations(range(4)):
        img, cases = ref.edge_raster(C, band=band)
        want, wc = ref.cells(img, 4, C, **dict(KW, band=band, q8=ref.EDGE_Q8, **kw))
        assert [bool(v & ref.CANDIDATE) for v in want[0]] == [k >= 0 for _, k, _ in cases]
        _check(*_cells(ctx, img, 4, C, band=band, q8=ref.EDGE_Q8, **kw), want, wc)
        # the same samples read with the default roles: another answer, and still the restatement's
        want2, wc2 = ref.cells(img, 4, C, **dict(KW, q8=ref.EDGE_Q8, **kw))
        _check(*_cells(ctx, img, 4, C, q8=ref.EDGE_Q8, **kw), want2, wc2)
        flags.add(want2.tobytes())
    assert len(flags) > 1
    img, cases = ref.edge_raster(C)
    for q8 in ref.all_switches(ref.EDGE_Q8):
        want, wc = ref.cells(img, 4, C, **dict(KW, q8=q8, **kw))
        assert [bool(v & ref.CANDIDATE) for v in want[0]] == [k >= 0 or q8[t] < 0 for t, k, _ in cases]
        _check(*_cells(ctx, img, 4, C, q8=q8, **kw), want, wc)


@pytest.mark.parametrize("spp,C,mode", [(4, 8, "vector"), (1, 4, "vector"), (4, 16, "pitch"), (1, 16, "vector")])
def test_cells_cut_into_calls(ctx, spp, C, mode):
    """a strip cut at multiples of C, each call writing from cell line first / C on and adding into the same counters"""
    import torch
    rows, w = 7 * C + 5, 10 * C + 3
    img = ref.random_raster(rows, w * spp, 77 + C)
    want, wc = ref.cells(img, spp, C, **KW)
    gw, gh = ref.grid(w, rows, C)
    cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
    parts = []
    for a, b in ((0, 2 * C), (2 * C, 3 * C), (3 * C, rows)):
        got, _ = _cells(ctx, img[a:b], spp, C, mode, slack=0, counts=cnt)
        parts.append(got)
    assert np.array_equal(np.concatenate(parts), want)
    assert np.array_equal(cnt.cpu().numpy().astype(np.uint64), wc)


# ---- morphology ------------------------------------------------------------------------------------------------------------------
RADII = [(0, 0), (1, 1), (2, 5), (7, 64), (32, 1), (1, 64), (0, 5)]   # every a of 0, 1, 2, 7, 32 and every d of 0, 1, 5, 64


@pytest.mark.parametrize("gw", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("gh", [1, 2, 70])
def test_morph(ctx, gw, gh):
    """grids around the word size, one and two lines, radii beyond the grid; a flag_pitch wider than gw whose bytes behind each
    line survive; the counters; a second call is a no-op"""
    import torch
    slack = 5
    kept = 0
    for density in (0.0, 0.5, 0.97, 1.0):
        f = ref.flag_grid(gh, gw, density, 1000 * gw + gh)
        for a, d in (RADII if 0 < density < 1 else [(1, 2), (32, 64)]):
            want, (n_cloud, n_buffer) = ref.morph(f, a, d)
            host = np.full((gh, gw + slack), 0xA5, np.uint8)
            host[:, :gw] = f
            dev = torch.from_numpy(host).cuda()
            cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
            ctx.mask_morph_u8(dev, gw + slack, gw, gh, a, d, cnt)
            ctx.sync()
            got = dev.cpu().numpy()
            assert np.array_equal(got[:, :gw], want), (density, a, d, int((got[:, :gw] != want).sum()))
            assert (got[:, gw:] == 0xA5).all()
            assert cnt.cpu().numpy().tolist() == [0, 0, 0, 0, 0, n_cloud, n_buffer, 0]
            ctx.mask_morph_u8(dev, gw + slack, gw, gh, a, d, cnt)                         # again: the same bytes, the counts once more
            ctx.sync()
            assert np.array_equal(dev.cpu().numpy(), got) and cnt.cpu().numpy().tolist() == [0, 0, 0, 0, 0, 2 * n_cloud, 2 * n_buffer, 0]
            kept += n_cloud
    assert kept > 0


def test_morph_more_than_one_workgroup(ctx):
    """300 x 400 cells: 2000 words, the grid-stride loops of every kernel take more than one workgroup"""
    import torch
    gh, gw = 400, 300
    f = ref.flag_grid(gh, gw, 0.97, 5)
    want, (n_cloud, n_buffer) = ref.morph(f, 2, 3)
    dev = torch.from_numpy(f).cuda()
    cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
    ctx.mask_morph_u8(dev, gw, gw, gh, 2, 3, cnt)
    ctx.sync()
    assert np.array_equal(dev.cpu().numpy(), want) and cnt.cpu().numpy().tolist()[5:7] == [n_cloud, n_buffer] and n_cloud > 0 and n_buffer > 0


# ---- arguments ---------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_launch_nothing(ctx):
    import torch
    img = _cuda(ref.random_raster(16, 64, 1))
    flags = torch.full((4, 8), FILL, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
    ok = dict(src=img, pitch=64, w=16, rows=16, spp=4, cell=8, flags=flags, flag_pitch=8, counts=cnt, valid_min=1, sat_level=4095, full_scale=4095,
              band=(2, 1, 0, 3), bright_q8=77, white_q8=38, hot_q8=20, ndvi_q8=51)
    bad = [dict(cell=5), dict(cell=32), dict(spp=2), dict(spp=3), dict(w=-1), dict(rows=-1), dict(pitch=63), dict(flag_pitch=1), dict(valid_min=-1),
           dict(valid_min=65536), dict(sat_level=0), dict(sat_level=65536), dict(full_scale=0), dict(full_scale=65536), dict(band=(0, 0, 1, 2)),
           dict(band=(0, 1, 2, 4)), dict(band=(-1, 1, 2, 3)), dict(band=None), dict(bright_q8=-2), dict(bright_q8=257), dict(white_q8=257),
           dict(hot_q8=-2), dict(ndvi_q8=300), dict(src=None), dict(flags=None), dict(src=img.data_ptr() + 1)]
    for b in bad:
        with pytest.raises(ValueError):
            ctx.mask_cells_u16(**dict(ok, **b))
    m = dict(flags=flags, flag_pitch=8, gw=8, gh=4, open_radius=1, buffer_radius=2, counts=cnt)
    for b in [dict(open_radius=-1), dict(open_radius=33), dict(buffer_radius=-1), dict(buffer_radius=65), dict(flag_pitch=7), dict(gw=-1), dict(gh=-1),
              dict(flags=None)]:
        with pytest.raises(ValueError):
            ctx.mask_morph_u8(**dict(m, **b))
    ctx.sync()
    assert (flags.cpu().numpy() == FILL).all() and cnt.cpu().numpy().tolist() == [0] * 8
    # empty windows and grids are no-ops; spp 1 ignores the band roles
    ctx.mask_cells_u16(**dict(ok, w=0, pitch=0))
    ctx.mask_cells_u16(**dict(ok, rows=0))
    ctx.mask_morph_u8(**dict(m, gw=0))
    ctx.mask_morph_u8(**dict(m, gh=0))
    ctx.sync()
    assert (flags.cpu().numpy() == FILL).all() and cnt.cpu().numpy().tolist() == [0] * 8
    ctx.mask_cells_u16(**dict(ok, spp=1, w=64, band=None))
    ctx.sync()
    assert cnt.cpu().numpy().tolist()[0] == 16
