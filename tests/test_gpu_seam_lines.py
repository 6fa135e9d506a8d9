"""GPU: oip_seam_moments_blocks_u16 and oip_stitch_balanced_lines_u16 against the integer restatement (_seam_lines_ref.py on
_seam_ref.py).  All sums and the per-sample arithmetic are exact integers, so every comparison is equality.

The stitch shapes are test_gpu_seam.py's STITCH_SHAPES (its docstring says which kernel each takes: (520, 257, 13, 1) the
per-sample one, the others the vector one) and its (4200, 2200, 100, 1), whose 2 255 000 chunks take lanes of the vector
kernel through its outer loop a second time."""
import functools

import numpy as np
import pytest

import _seam_ref as ref
import _seam_lines_ref as lref

pytestmark = pytest.mark.gpu

STITCH_SHAPES = [(96, 64, 8, 1), (520, 257, 13, 1), (131, 1000, 3, 4), (64, 1, 4, 1), (1024, 37, 100, 1), (256, 300, 25, 4)]
MOMENT_SHAPES = STITCH_SHAPES[:4]                                      # test_gpu_seam.py's
# (W, L, fold, spp, B).  The last one is not the issue's: 2500 line ranges are more than the 2048 workgroups a column group gets
# on 256 CUs, so workgroups take a second range (the kernel's grid-stride loop, with its second barrier)
MOMENT_CASES = [(96, 64, 8, 1, 16), (96, 64, 8, 1, 1), (520, 257, 13, 1, 50), (131, 1000, 3, 4, 64), (64, 1, 4, 1, 8), (131, 1000, 3, 4, 5000),
                (64, 5000, 4, 1, 2)]


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _acc(nb, spp):
    import torch
    return torch.zeros(nb, 6, spp, dtype=torch.int64, device="cuda")   # the bits of the library's uint64 planes


def _host(acc):
    return acc.cpu().numpy().view(np.uint64)


@functools.lru_cache(maxsize=None)
def _pair(W, L, fold, spp):
    """test_gpu_seam.py's recipe: two full-range images with 3 % zeros in each, and zeros in the two columns either side of
    the seam: in image 1 on lines 0, 3, 6 .., in image 2 on lines 1, 4 .., in both on lines 2, 5 ..  Shared, left unchanged."""
    rng = np.random.default_rng(1000 * W + L)
    left, right = (rng.integers(0, 65536, (L, W * spp), dtype=np.uint16) for _ in range(2))
    for img in (left, right):
        img[rng.random(img.shape) < 0.03] = 0
    l3, r3 = left.reshape(L, W, spp), right.reshape(L, W, spp)
    for k in (0, 2):
        l3[k::3, W - fold - 1:W - fold + 1] = 0
    for k in (1, 2):
        r3[k::3, fold - 1:fold + 1] = 0
    return left, right


@functools.lru_cache(maxsize=None)
def _tables(L, spp, seed=0):
    """a (G, O) per line and channel: gains of 0.8 .. 1.2, offsets of +-20000 DN"""
    rng = np.random.default_rng(77 + L + seed)
    return (rng.integers(52429, 78644, (L, spp)).astype(np.int32), rng.integers(-20000 * 65536, 20000 * 65536 + 1, (L, spp)).astype(np.int32))


# ---- moments per block --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,L,fold,spp,B", MOMENT_CASES)
def test_block_moments_equal_restatement(ctx, W, L, fold, spp, B):
    left, right = _pair(W, L, fold, spp)
    dl, dr = _cuda(left), _cuda(right)
    nb = max(1, L // B)
    acc, whole = _acc(nb, spp), _acc(1, spp)
    ctx.seam_moments_blocks_u16(dl, dr, W * spp, L, fold * spp, spp, B, acc)
    ctx.seam_moments_u16(dl, dr, W * spp, L, fold * spp, spp, whole)
    ctx.sync()
    want = lref.block_moments(left, right, fold, spp, B)
    assert want.shape == (nb, 6, spp) and np.array_equal(_host(acc), want)
    assert np.array_equal(_host(acc).sum(0, dtype=np.uint64), _host(whole)[0])
    assert [int(n) for n in want[:, 0, 0]] == [2 * fold * (b - a) for a, b in lref.blocks(L, B)]
    # a second call doubles every plane
    ctx.seam_moments_blocks_u16(dl, dr, W * spp, L, fold * spp, spp, B, acc)
    ctx.sync()
    assert np.array_equal(_host(acc), 2 * want)


def test_block_moments_valid_window(ctx):
    """[64, 4095] on data in 0..8191 with zeros planted in each image (test_gpu_seam.py's recipe): pairs are rejected by a
    alone, by b alone and by both; 5 blocks, the last of 57 lines"""
    W, L, fold, spp, B = 520, 257, 13, 1, 50
    rng = np.random.default_rng(5)
    left, right = (rng.integers(0, 8192, (L, W), dtype=np.uint16) for _ in range(2))
    left[rng.random((L, W)) < 0.05] = 0
    right[rng.random((L, W)) < 0.05] = 0
    a, b = ref.overlap(left, right, fold, spp)
    bad_a, bad_b = (a < 64) | (a > 4095), (b < 64) | (b > 4095)
    assert (bad_a & ~bad_b).any() and (~bad_a & bad_b).any() and (bad_a & bad_b).any()
    acc, whole = _acc(5, spp), _acc(1, spp)
    ctx.seam_moments_blocks_u16(_cuda(left), _cuda(right), W, L, fold, spp, B, acc, 64, 4095)
    ctx.seam_moments_u16(_cuda(left), _cuda(right), W, L, fold, spp, whole, 64, 4095)
    ctx.sync()
    want = lref.block_moments(left, right, fold, spp, B, 64, 4095)
    assert np.array_equal(_host(acc), want) and int(want[:, 0, 0].sum()) == np.count_nonzero(~bad_a & ~bad_b)
    assert np.array_equal(_host(acc).sum(0, dtype=np.uint64), _host(whole)[0])


@pytest.mark.parametrize("B", [70000, 300])
def test_block_moments_top_of_the_range(ctx, B):
    """65535 throughout, 70000 lines.  B = 70000: one block, Sab = n * 65535^2 > 2^48, several line ranges, many lines per
    lane.  B = 300: 233 blocks, the last of 400 lines.  The closed-form totals are per block."""
    import torch
    W, L, fold = 64, 70000, 4
    d = torch.full((L, W), -1, dtype=torch.int16, device="cuda").view(torch.uint16)
    nb = max(1, L // B)
    acc = _acc(nb, 1)
    ctx.seam_moments_blocks_u16(d, d, W, L, fold, 1, B, acc)
    ctx.sync()
    got = _host(acc)
    for k, (r0, r1) in enumerate(lref.blocks(L, B)):
        n = 2 * fold * (r1 - r0)
        assert got[k, :, 0].tolist() == [n, n * 65535, n * 65535, n * 65535 ** 2, n * 65535 ** 2, n * 65535 ** 2], k
    assert len(lref.blocks(L, B)) == nb and (B != 70000 or 2 * fold * L * 65535 ** 2 > 2 ** 48)


@pytest.mark.parametrize("window", [(), (64, 4095)])
@pytest.mark.parametrize("W,L,fold,spp", MOMENT_SHAPES)
def test_strip_moments_are_plane_0_of_one_block(ctx, W, L, fold, spp, window):
    """the strip entry and the blocks entry are one kernel: with B = L and with B = L + 1 there is one block, and its plane
    holds the strip entry's 6 * spp words; unmasked and with the valid window [64, 4095]"""
    left, right = _pair(W, L, fold, spp)
    dl, dr = _cuda(left), _cuda(right)
    strip = _acc(1, spp)
    ctx.seam_moments_u16(dl, dr, W * spp, L, fold * spp, spp, strip[0], *window)
    for B in (L, L + 1):
        acc = _acc(1, spp)
        ctx.seam_moments_blocks_u16(dl, dr, W * spp, L, fold * spp, spp, B, acc, *window)
        ctx.sync()
        assert np.array_equal(_host(acc)[0], _host(strip)[0]), B
    assert window or (_host(strip)[0, 0] == 2 * fold * L).all()


def test_strip_and_block_moments_keep_their_profiler_names(ctx):
    W, L, fold = 96, 64, 8
    left, right = _pair(W, L, fold, 1)
    dl, dr = _cuda(left), _cuda(right)
    ctx.profile_enable(True)
    ctx.profile_reset()
    strip, acc = _acc(1, 1), _acc(4, 1)
    ctx.seam_moments_u16(dl, dr, W, L, fold, 1, strip[0])
    ctx.seam_moments_blocks_u16(dl, dr, W, L, fold, 1, 16, acc)
    ctx.sync()
    prof = ctx.profile()
    ctx.profile_enable(False)
    assert prof["seam_moments_kernel"][1] == 1 and prof["seam_moments_blocks_kernel"][1] == 1


# ---- the stitch with a (G, O) per line ------------------------------------------------------------------------------------------
def _stitch_lines(ctx, left, right, W, L, fold, spp, LG, LO, h, valid_min=1, table_offset=0):
    """table_offset: the tables start that many int32 into their allocations"""
    import torch
    out = torch.zeros(L, 2 * (W - fold) * spp, dtype=torch.uint16, device="cuda")
    pad = np.zeros(table_offset, np.int32)
    dg = _cuda(np.concatenate([pad, np.asarray(LG, np.int32).reshape(-1)]))
    do = _cuda(np.concatenate([pad, np.asarray(LO, np.int32).reshape(-1)]))
    ctx.stitch_balanced_lines_u16(_cuda(left), _cuda(right), out, W * spp, L, fold * spp, spp, dg.data_ptr() + 4 * table_offset,
                                  do.data_ptr() + 4 * table_offset, h, valid_min)
    ctx.sync()
    return out.cpu().numpy()


@pytest.mark.parametrize("h", ["0", "1", "fold"])
@pytest.mark.parametrize("W,L,fold,spp", STITCH_SHAPES)
def test_stitch_lines_equals_restatement(ctx, W, L, fold, spp, h):
    h = fold if h == "fold" else int(h)
    left, right = _pair(W, L, fold, spp)
    LG, LO = _tables(L, spp)
    got = _stitch_lines(ctx, left, right, W, L, fold, spp, LG, LO, h)
    assert np.array_equal(got, lref.stitch_lines(left, right, fold, spp, LG, LO, h, 1))
    # preconditions: the balance clamps at both ends, offsets of both signs, "no data" of either image inside the blend zone
    if L > 1:
        b = right.reshape(L, W, spp)[:, fold:]
        bb = np.stack([ref.balance(b[r], LG[r], LO[r]) for r in range(L)])
        assert (bb[b > 0] == 0).any() and (bb == 65535).any() and (LO < 0).any() and (LO > 0).any()
        a, b = ref.overlap(left, right, fold, spp)
        za, zb = a[:, fold - h:fold + h] == 0, b[:, fold - h:fold + h] == 0
        assert not h or ((za & ~zb).any() and (~za & zb).any() and (za & zb).any())


def test_stitch_lines_more_than_one_trip_per_lane(ctx):
    W, L, fold, spp = 4200, 2200, 100, 1
    assert (2 * (W - fold) // 8) * L > 256 * 8 * 256 * 4
    left, right = _pair(W, L, fold, spp)
    LG, LO = _tables(L, spp)
    got = _stitch_lines(ctx, left, right, W, L, fold, spp, LG, LO, fold)
    assert np.array_equal(got, lref.stitch_lines(left, right, fold, spp, LG, LO, fold, 1))


def test_stitch_lines_four_sample_tables_off_16_bytes(ctx):
    """4-sample tables that start 4 bytes past a 16-byte boundary cannot be read 16 bytes at a time: the per-sample kernel
    takes the call, with the same result"""
    W, L, fold, spp = 256, 300, 25, 4
    left, right = _pair(W, L, fold, spp)
    LG, LO = _tables(L, spp)
    got = _stitch_lines(ctx, left, right, W, L, fold, spp, LG, LO, fold, 1, table_offset=1)
    assert np.array_equal(got, lref.stitch_lines(left, right, fold, spp, LG, LO, fold, 1))


@pytest.mark.parametrize("W,L,fold,spp", STITCH_SHAPES)
def test_constant_tables_give_the_balanced_stitch(ctx, W, L, fold, spp):
    """one (G, O) repeated on every line: oip_stitch_balanced_u16's bytes; the identity with h = 0: oip_stitch_rows_u16's"""
    import torch
    left, right = _pair(W, L, fold, spp)
    dl, dr = _cuda(left), _cuda(right)
    G = np.array([70124, 60948, 52429, 78643][:spp], np.int32)
    O = np.array([41 * 65536, -300 * 65536, 20000 * 65536, -70000][:spp], np.int32)
    for h in (0, 1, fold):
        want = torch.zeros(L, 2 * (W - fold) * spp, dtype=torch.uint16, device="cuda")
        ctx.stitch_balanced_u16(dl, dr, want, W * spp, L, fold * spp, spp, _cuda(G), _cuda(O), h, 1)
        got = _stitch_lines(ctx, left, right, W, L, fold, spp, np.tile(G, (L, 1)), np.tile(O, (L, 1)), h)
        assert got.tobytes() == want.cpu().numpy().tobytes(), h
    plain = torch.zeros(L, 2 * (W - fold) * spp, dtype=torch.uint16, device="cuda")
    ctx.stitch_rows_u16(dl, dr, plain, W * spp, L, fold * spp)
    got = _stitch_lines(ctx, left, right, W, L, fold, spp, np.full((L, spp), 65536), np.zeros((L, spp)), 0)
    assert got.tobytes() == plain.cpu().numpy().tobytes()
    assert np.array_equal(got, np.concatenate([left[:, :(W - fold) * spp], right[:, fold * spp:]], 1))


def test_stitch_lines_valid_min_zero_blends_everything(ctx):
    W, L, fold, spp = 256, 300, 25, 4
    left, right = _pair(W, L, fold, spp)
    LG, LO = _tables(L, spp)
    got = _stitch_lines(ctx, left, right, W, L, fold, spp, LG, LO, fold, 0)
    assert np.array_equal(got, lref.stitch_lines(left, right, fold, spp, LG, LO, fold, 0))
    assert not np.array_equal(got, _stitch_lines(ctx, left, right, W, L, fold, spp, LG, LO, fold, 1))


def test_bad_arguments_and_profiler(ctx):
    import torch
    W, L, fold = 96, 64, 8
    left, right = _pair(W, L, fold, 1)
    dl, dr = _cuda(left), _cuda(right)
    out = torch.zeros(L, 2 * (W - fold), dtype=torch.uint16, device="cuda")
    g, o = _cuda(np.full(L, 65536, np.int32)), _cuda(np.zeros(L, np.int32))
    with pytest.raises(ValueError):
        ctx.stitch_balanced_lines_u16(dl, dr, out, W, L, fold, 2, g, o, 0, 1)            # spp
    with pytest.raises(ValueError):
        ctx.stitch_balanced_lines_u16(dl, dr, out, W, L, fold, 1, g, o, fold + 1, 1)     # h > fold
    with pytest.raises(ValueError):
        ctx.stitch_balanced_lines_u16(dl, dr, out, W, L, fold, 1, None, o, 0, 1)         # null tables
    with pytest.raises(ValueError):
        ctx.stitch_balanced_lines_u16(dl, dr, out, W, L, fold, 1, g, None, 0, 1)
    with pytest.raises(ValueError):
        ctx.seam_moments_blocks_u16(dl, dr, W, L, fold, 1, 0, _acc(1, 1))                # B = 0
    with pytest.raises(ValueError):
        ctx.seam_moments_blocks_u16(dl, dr, W, L, fold, 2, 16, _acc(4, 1))               # spp
    with pytest.raises(ValueError):
        ctx.seam_moments_blocks_u16(dl, dr, W, L, 49, 1, 16, _acc(4, 1))                 # 2 fold > W
    ctx.profile_enable(True)
    ctx.profile_reset()
    ctx.stitch_balanced_lines_u16(dl, dr, out, W, L, fold, 1, g, o, 2, 1)
    ctx.seam_moments_blocks_u16(dl, dr, W, L, fold, 1, 16, _acc(4, 1))
    ctx.sync()
    prof = ctx.profile()
    ctx.profile_enable(False)
    assert prof["stitch_balanced_lines_kernel"][1] == 1 and prof["seam_moments_blocks_kernel"][1] == 1
