"""GPU: oip_block_moments_u16 and oip_wallis_apply_u16 against the restatement (_wallis_ref.py).  Moments, samples and counters
are exact integer functions of the input, so every comparison is equality, and a fill pattern beside every output shows that
nothing else is written.  The shapes are the smallest that can go wrong: partial blocks right and bottom, a last vector that
leaves the line, one whole and one partial block, more than one workgroup, blocks of one whole wave and of two (spp 4, B 128 and 256),
the vector kernels and the plain ones on the same data, grids of one and two nodes per axis, node values at the extremes."""
import numpy as np
import pytest

import _wallis_ref as ref

pytestmark = pytest.mark.gpu
FILL = -0x0123456789ABCDF                                                # what the moment planes hold before a call
PAD = 0x7777                                                           # what lies between the lines and around the rasters
SHAPES = [(203, 77, 1), (202, 77, 4), (32, 32, 1), (3, 3, 4), (1024, 64, 1), (1024, 64, 4)]
MODES = ("vector", "pitch", "base")


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def _raster(w, rows, spp, B, seed):
    """random 12-bit samples with zeros and 65535 among them and, where the raster has more than one block, one block of zeros"""
    img = ref.random_raster(rows, w * spp, seed)
    if w > B and rows > B:
        img[:B, :B * spp] = 0
    return img


def _moments(ctx, img, spp, B, mode="vector", slack=2, acc=None, first=0, vmin=1, vmax=65535, total_rows=None):
    """the planes of one call as (3 * spp, gh + 1, gw + slack) int64.  mode: "vector" (a pitch that is a multiple of 8 and an
    aligned base), "pitch" (a pitch that is not), "base" (a base off by one sample)"""
    import torch
    rows, ws = img.shape
    w = ws // spp
    pitch = -(-ws // 8) * 8 if mode != "pitch" else -(-ws // 8) * 8 + 3
    off = 1 if mode == "base" else 0
    host = np.full(rows * pitch + 8, PAD, np.uint16)
    host[off:off + rows * pitch].reshape(rows, pitch)[:, :ws] = img
    dev = _cuda(host)
    gw, gh = ref.grid(w, rows if total_rows is None else total_rows, B)
    if acc is None:
        acc = torch.full((3 * spp, gh + 1, gw + slack), FILL, dtype=torch.int64, device="cuda")
    ctx.block_moments_u16(dev.data_ptr() + 2 * off, pitch, w, rows, spp, B, acc.data_ptr() + 8 * (first // B) * (gw + slack), gw + slack,
                          (gh + 1) * (gw + slack), vmin, vmax)
    ctx.sync()
    return acc


def _check_moments(acc, want):
    got = acc.cpu().numpy()
    _, spp, gh, gw = want.shape
    w = want.reshape(3 * spp, gh, gw).astype(np.int64)
    assert np.array_equal(got[:, :gh, :gw], w), "%d of %d entries differ" % (int((got[:, :gh, :gw] != w).sum()), w.size)
    assert (got[:, gh:] == FILL).all() and (got[:, :, gw:] == FILL).all()                   # nothing written beside the entries


# ---- moments -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,rows,spp", SHAPES)
@pytest.mark.parametrize("B", [32, 64])
def test_moments_random(ctx, w, rows, spp, B):
    img = _raster(w, rows, spp, B, 17 * w + B + spp)
    for vmin, vmax in ((1, 65535), (0, 4000)):
        want = ref.moments(img, spp, B, vmin, vmax)
        if w > B and rows > B and vmin == 1:
            assert (want[:, :, 0, 0] == 0).all() and (want[0] > 0).sum() == want[0].size - spp     # the block without a valid sample
        for mode in MODES:
            _check_moments(_moments(ctx, img, spp, B, mode, vmin=vmin, vmax=vmax), want)


@pytest.mark.parametrize("B", [128, 256])
def test_moments_blocks_wider_than_a_wave(ctx, B):
    """520 x 300 x 4: at B 128 a block is the 64 lanes of one whole wave, at B 256 the 128 lanes of two waves whose totals meet in
    LDS; partial blocks right and bottom"""
    w, rows, spp = 520, 300, 4
    img = _raster(w, rows, spp, B, B)
    want = ref.moments(img, spp, B)
    for mode in MODES:
        _check_moments(_moments(ctx, img, spp, B, mode), want)


@pytest.mark.parametrize("spp,B,mode", [(1, 32, "vector"), (4, 32, "vector"), (4, 128, "vector"), (4, 256, "vector"), (1, 64, "pitch")])
def test_moments_cut_into_calls(ctx, spp, B, mode):
    """a strip of 5 B + 3 lines cut at B and 3 B, each call writing from block line first / B on: the entries of one call"""
    rows, w = 5 * B + 3, 2 * B + 5
    img = _raster(w, rows, spp, B, 5 + B)
    want = ref.moments(img, spp, B)
    acc = None
    for a, b in ((0, B), (B, 3 * B), (3 * B, rows)):
        acc = _moments(ctx, img[a:b], spp, B, mode, acc=acc, first=a, total_rows=rows)
    _check_moments(acc, want)


def test_moments_full_scale_block(ctx):
    """a whole 256 x 256 block of 65535: S1 = 2^32 - 65536 and S2 = 65536 * 65535^2 are the largest entries there are"""
    img = np.full((256, 256), 65535, np.uint16)
    want = ref.moments(img, 1, 256)
    assert int(want[1, 0, 0, 0]) == (1 << 32) - 65536 and int(want[2, 0, 0, 0]) == 65536 * 65535 ** 2
    for mode in ("vector", "pitch"):
        _check_moments(_moments(ctx, img, 1, 256, mode), want)


def test_moments_refusals(ctx):
    import torch
    img = _cuda(np.zeros((64, 64), np.uint16))
    acc = torch.zeros(3 * 4 * 4, dtype=torch.int64, device="cuda")
    good = dict(src=img, pitch=64, w=64, rows=64, spp=1, block=32, acc=acc, acc_pitch=2, acc_plane_stride=4, valid_min=1, valid_max=65535)
    ctx.block_moments_u16(**good)
    ctx.block_moments_u16(**dict(good, w=0))
    ctx.block_moments_u16(**dict(good, rows=0))
    for bad in (dict(block=16), dict(block=48), dict(spp=2), dict(w=-1), dict(rows=-1), dict(pitch=63), dict(acc_pitch=1), dict(valid_min=5, valid_max=4),
                dict(valid_min=-1), dict(valid_max=65536), dict(spp=4, w=16, acc_pitch=1, acc_plane_stride=1)):
        with pytest.raises(ValueError):
            ctx.block_moments_u16(**dict(good, **bad))
    ctx.sync()


# ---- apply ---------------------------------------------------------------------------------------------------------------------
def _apply(ctx, img, spp, G, O, B, mode="vector", row0=0, L=None, in_place=False, stats=None, vmin=1, vmax=65535, cmax=65535):
    """(out (rows, ws) uint16, the three counters) of one call; the output lies between two guard bands that must stay"""
    import torch
    rows, ws = img.shape
    W = ws // spp
    L = rows if L is None else L
    off = 1 if mode == "base" else 0
    guard = 64
    n = rows * ws
    src = np.full(n + 2 * guard + 8, PAD, np.uint16)
    src[guard + off:guard + off + n] = img.reshape(-1)
    d_src = _cuda(src)
    d_dst = d_src if in_place else _cuda(np.full(n + 2 * guard + 8, PAD, np.uint16))
    gh, gw, _ = G.shape
    dG, dO = torch.from_numpy(np.ascontiguousarray(G, np.int32)).cuda(), torch.from_numpy(np.ascontiguousarray(O, np.int32)).cuda()
    st = torch.zeros(3, dtype=torch.int64, device="cuda") if stats is None else stats
    at = 2 * (guard + off)
    ctx.wallis_apply_u16(d_src.data_ptr() + at, d_dst.data_ptr() + at, row0, rows, W, L, spp, B, dG, dO, gw, gh, vmin, vmax, cmax, st)
    ctx.sync()
    got = d_dst.cpu().numpy().view(np.uint16)
    assert (got[:guard + off] == PAD).all() and (got[guard + off + n:] == PAD).all()        # nothing written beside the lines
    return got[guard + off:guard + off + n].reshape(rows, ws), st.cpu().numpy().astype(np.uint64)


def _fitted(img, spp, B):
    G, O, _, _ = ref.fit(ref.moments(img, spp, B), 1.0, 1.0, 0.25, 4.0)
    return G, O


@pytest.mark.parametrize("w,rows,spp", SHAPES + [(520, 300, 4)])
@pytest.mark.parametrize("B", [32, 64])
def test_apply_random_and_fitted_nodes(ctx, w, rows, spp, B):
    """203 x 77 and 3 x 3 x 4 have lines that are no multiple of 8 samples: the plain kernel; every other shape runs the vector
    kernel and, with the base off by one sample, the plain one.  Nodes over the whole allowed range (G up to 2^20, O +-2^28) and
    nodes fitted to the raster; clamp_max 4095, so that results are cut at both ends"""
    img = _raster(w, rows, spp, B, 3 * w + B + spp)
    gw, gh = ref.grid(w, rows, B)
    tables = [ref.random_nodes(gh, gw, spp, w + B), ref.mild_nodes(gh, gw, spp, w + B + 1)]
    if w > B:
        tables.append(_fitted(img, spp, B))
    for k, (G, O) in enumerate(tables):
        want, wc = ref.apply(img, spp, G, O, B, 1, 65535, 4095)
        assert wc[0] == ((img >= 1) & (img <= 65535)).sum()
        if k == 1 and w >= 200:
            assert wc[1] > 0 and wc[2] > 0 and wc[0] > wc[1] + wc[2]                        # both clamps occur, and results in between
        for mode in ("vector", "base"):
            got, counts = _apply(ctx, img, spp, G, O, B, mode, cmax=4095)
            assert np.array_equal(got, want), "%s: %d of %d samples differ" % (mode, int((got != want).sum()), want.size)
            assert np.array_equal(counts, wc), (counts, wc)


@pytest.mark.parametrize("B", [128, 256])
def test_apply_wide_blocks(ctx, B):
    w, rows, spp = 520, 300, 4
    img = _raster(w, rows, spp, B, B + 1)
    gw, gh = ref.grid(w, rows, B)
    G, O = ref.random_nodes(gh, gw, spp, B)
    want, wc = ref.apply(img, spp, G, O, B, 1, 4000, 65535)
    for mode in ("vector", "base"):
        got, counts = _apply(ctx, img, spp, G, O, B, mode, vmax=4000)
        assert np.array_equal(got, want) and np.array_equal(counts, wc)
    assert np.array_equal(want[img > 4000], img[img > 4000]) and (img > 4000).any()         # saturation passes through


@pytest.mark.parametrize("w,rows,spp,B", [(64, 20, 1, 32), (24, 100, 4, 32), (40, 64, 1, 32), (16, 16, 4, 64), (2048, 9, 1, 32), (512, 9, 4, 32)])
def test_apply_small_grids(ctx, w, rows, spp, B):
    """gh == 1, gw == 1, gh == 2, one node in all; and a workgroup's widest span of node columns (2048 samples of B 32)"""
    img = _raster(w, rows, spp, B, w + rows)
    gw, gh = ref.grid(w, rows, B)
    G, O = ref.random_nodes(gh, gw, spp, w)
    want, wc = ref.apply(img, spp, G, O, B)
    for mode in ("vector", "base"):
        got, counts = _apply(ctx, img, spp, G, O, B, mode)
        assert np.array_equal(got, want) and np.array_equal(counts, wc)


@pytest.mark.parametrize("spp,mode", [(1, "vector"), (4, "vector"), (4, "base")])
def test_apply_in_place_and_cut_anywhere(ctx, spp, mode):
    """in place; and a strip cut at lines that are multiples of nothing, the counters adding up"""
    import torch
    B, w, rows = 32, 200, 101
    img = _raster(w, rows, spp, B, 41 + spp)
    gw, gh = ref.grid(w, rows, B)
    G, O = ref.mild_nodes(gh, gw, spp, 7)
    want, wc = ref.apply(img, spp, G, O, B, 1, 65535, 4095)
    got, counts = _apply(ctx, img, spp, G, O, B, mode, in_place=True, cmax=4095)
    assert np.array_equal(got, want) and np.array_equal(counts, wc)
    st = torch.zeros(3, dtype=torch.int64, device="cuda")
    parts = []
    for a, b in ((0, 13), (13, 14), (14, 77), (77, rows)):
        part, _ = _apply(ctx, img[a:b], spp, G, O, B, mode, row0=a, L=rows, stats=st, cmax=4095)
        parts.append(part)
    assert np.array_equal(np.concatenate(parts), want)
    assert np.array_equal(st.cpu().numpy().astype(np.uint64), wc)


@pytest.mark.parametrize("w,spp", [(64, 1), (16, 4)])
def test_apply_long_strip_many_rounds_per_workgroup(ctx, w, spp):
    """70000 lines of 64 samples: one column of workgroups, which the launch gives more rounds of 8 lines than it has workgroups
    (8750 rounds against at most 8 per CU), so that every workgroup walks several consecutive rounds -- what every real strip
    does and no small shape can.  The state a workgroup keeps between rounds is then in use: the two node lines held in registers
    (the nodes differ from line to line of the grid and a line passes a node every 32 lines, inside a workgroup's walk as well as
    between two) and the two halves of the LDS table.  As one call, and cut at odd lines with the counters adding up."""
    import torch
    B, rows = 32, 70000
    img = ref.random_raster(rows, w * spp, 19 + spp)
    gw, gh = ref.grid(w, rows, B)
    assert gh > 2048
    G, O = ref.random_nodes(gh, gw, spp, 23)
    assert (np.diff(G.astype(np.int64), axis=0) != 0).all()             # no two node lines alike
    want, wc = ref.apply(img, spp, G, O, B, 1, 65535, 4095)
    got, counts = _apply(ctx, img, spp, G, O, B, cmax=4095)
    assert np.array_equal(got, want), "%d of %d samples differ, first at line %d" % (
        int((got != want).sum()), want.size, int(np.argmax((got != want).any(axis=1))))
    assert np.array_equal(counts, wc) and wc[1] > 0 and wc[2] > 0
    st = torch.zeros(3, dtype=torch.int64, device="cuda")
    for a, b in ((0, 33333), (33333, 33340), (33340, rows)):
        part, _ = _apply(ctx, img[a:b], spp, G, O, B, row0=a, L=rows, stats=st, cmax=4095)
        assert np.array_equal(part, want[a:b]), (a, b)
    assert np.array_equal(st.cpu().numpy().astype(np.uint64), wc)


@pytest.mark.parametrize("spp", [1, 4])
def test_apply_identity_and_constant_nodes(ctx, spp):
    B, w, rows = 64, 136, 70
    img = ref.random_raster(rows, w * spp, 3, 0, 65536)
    gw, gh = ref.grid(w, rows, B)
    one = np.ones((gh, gw, spp), np.int32)
    for mode in ("vector", "base"):
        got, counts = _apply(ctx, img, spp, 65536 * one, 0 * one, B, mode)
        assert np.array_equal(got, img) and counts[1] == 0 and counts[2] == 0
        got, _ = _apply(ctx, img, spp, 40000 * one, -123456 * one, B, mode)
        assert np.array_equal(got, ref.plain(img, 40000, -123456))


def test_apply_refusals(ctx):
    import torch
    img = _cuda(np.zeros((64, 64), np.uint16))
    tab = torch.zeros(64, dtype=torch.int32, device="cuda")
    good = dict(src=img, dst=img, row0=0, rows=64, W=64, L=64, spp=1, block=32, gain_q16=tab, offset_q8=tab, gw=2, gh=2, valid_min=1, valid_max=65535,
                clamp_max=65535)
    ctx.wallis_apply_u16(**good)
    ctx.wallis_apply_u16(**dict(good, rows=0))
    for bad in (dict(block=16), dict(spp=3), dict(gw=3), dict(gh=1), dict(row0=-1), dict(row0=1), dict(rows=65), dict(valid_min=9, valid_max=8),
                dict(valid_max=65536), dict(clamp_max=0), dict(clamp_max=65536), dict(W=0), dict(L=0)):
        with pytest.raises(ValueError):
            ctx.wallis_apply_u16(**dict(good, **bad))
    ctx.sync()
