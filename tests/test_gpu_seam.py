"""GPU: oip_seam_moments_u16 and oip_stitch_balanced_u16 against the integer restatement (_seam_ref.py).  All sums and the
per-sample arithmetic are exact integers, so every comparison is equality.

Which kernel a stitch shape takes (the vector kernel needs an output line of 2 (W - fold) spp samples that is a multiple of
8; the bases torch hands out are aligned and W * L * spp is even in every case):
    (96, 64, 8, 1)       176 samples  vector          (131, 1000, 3, 4)   1024  vector (odd pixel pitch)
    (520, 257, 13, 1)   1014 samples  per-sample      (64, 1, 4, 1)        120  vector, a single line
    (1024, 37, 100, 1)  1848 samples  vector          (256, 300, 25, 4)   1848  vector
    (4200, 2200, 100, 1)  8200 samples, 2 255 000 chunks of 16 bytes: more than the 8 blocks per CU x 256 lanes x 4 chunks
                          (2 097 152 on the 256 CUs of an MI355X) one trip of the vector kernel's outer loop covers"""
import functools

import numpy as np
import pytest

import _seam_ref as ref

pytestmark = pytest.mark.gpu

MOMENT_SHAPES = [(96, 64, 8, 1), (520, 257, 13, 1), (131, 1000, 3, 4), (64, 1, 4, 1)]
STITCH_SHAPES = MOMENT_SHAPES + [(1024, 37, 100, 1), (256, 300, 25, 4)]
# gains on both sides of 1; offsets that clamp at 0 (small samples, first set) and at 65535 (large ones, second set)
PARAMS = {"low": ([60948, 70124, 78643, 52429], [-300 * 65536, -5 * 65536, -1000 * 65536, -70000]),
          "high": ([70124, 60948, 52429, 78643], [41 * 65536, 6000 * 65536, 20000 * 65536, 12345])}


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _acc(spp):
    import torch
    return torch.zeros(6, spp, dtype=torch.int64, device="cuda")       # the bits of the library's uint64 planes


def _host(acc):
    return acc.cpu().numpy().view(np.uint64)


@functools.lru_cache(maxsize=None)
def _pair(W, L, fold, spp):
    """two full-range images with 3 % zeros in each, and zeros in the two columns either side of the seam (inside every
    blend zone with h > 0): in image 1 on lines 0, 3, 6 .., in image 2 on lines 1, 4 .., in both on lines 2, 5 ..
    Shared by the tests of a shape, which leave them unchanged."""
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


# ---- moments ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,L,fold,spp", MOMENT_SHAPES)
def test_moments_equal_restatement(ctx, W, L, fold, spp):
    left, right = _pair(W, L, fold, spp)
    acc = _acc(spp)
    ctx.seam_moments_u16(_cuda(left), _cuda(right), W * spp, L, fold * spp, spp, acc)
    ctx.sync()
    want = ref.moments(left, right, fold, spp)
    assert np.array_equal(_host(acc), want)
    assert (want[0] == 2 * fold * L).all()


def test_moments_valid_window(ctx):
    """[64, 4095] on data in 0..8191 with zeros planted in each image: pairs are rejected by a alone, by b alone and by both"""
    W, L, fold, spp = 520, 257, 13, 1
    rng = np.random.default_rng(5)
    left, right = (rng.integers(0, 8192, (L, W), dtype=np.uint16) for _ in range(2))
    left[rng.random((L, W)) < 0.05] = 0
    right[rng.random((L, W)) < 0.05] = 0
    left[0, W - 2 * fold:W - 2 * fold + 4] = (63, 64, 4095, 4096)   # the bounds themselves, against valid partners
    right[0, :4] = 100
    a, b = ref.overlap(left, right, fold, spp)
    bad_a, bad_b = (a < 64) | (a > 4095), (b < 64) | (b > 4095)
    assert (bad_a & ~bad_b).any() and (~bad_a & bad_b).any() and (bad_a & bad_b).any() and (a == 0).any() and (b == 0).any()
    acc = _acc(spp)
    ctx.seam_moments_u16(_cuda(left), _cuda(right), W, L, fold, spp, acc, 64, 4095)
    ctx.sync()
    want = ref.moments(left, right, fold, spp, 64, 4095)
    assert np.array_equal(_host(acc), want) and want[0, 0] == np.count_nonzero(~bad_a & ~bad_b)


def test_moments_add_over_calls(ctx):
    W, L, fold, spp = 131, 1000, 3, 4
    left, right = _pair(W, L, fold, spp)
    dl, dr = _cuda(left), _cuda(right)
    whole, halves = _acc(spp), _acc(spp)
    ctx.seam_moments_u16(dl, dr, W * spp, L, fold * spp, spp, whole)
    off = 2 * W * spp * 499                                         # the second part first: the order does not matter
    ctx.seam_moments_u16(dl.data_ptr() + off, dr.data_ptr() + off, W * spp, L - 499, fold * spp, spp, halves)
    ctx.seam_moments_u16(dl, dr, W * spp, 499, fold * spp, spp, halves)
    ctx.seam_moments_u16(dl, dr, W * spp, 0, fold * spp, spp, halves)       # no lines: nothing added
    ctx.sync()
    assert np.array_equal(_host(whole), _host(halves)) and np.array_equal(_host(whole), ref.moments(left, right, fold, spp))


def test_moments_top_of_the_range(ctx):
    """65535 throughout, 70000 lines: Sab = n * 65535^2 > 2^48, Sa > 2^32; several line ranges, many lines per lane"""
    import torch
    W, L, fold = 64, 70000, 4
    d = torch.full((L, W), -1, dtype=torch.int16, device="cuda").view(torch.uint16)
    acc = _acc(1)
    ctx.seam_moments_u16(d, d, W, L, fold, 1, acc)
    ctx.sync()
    n = 2 * fold * L
    assert _host(acc)[:, 0].tolist() == [n, n * 65535, n * 65535, n * 65535 ** 2, n * 65535 ** 2, n * 65535 ** 2]
    assert n * 65535 ** 2 > 2 ** 48


def test_moments_bad_arguments(ctx):
    left, right = _pair(96, 64, 8, 1)
    dl, dr, acc = _cuda(left), _cuda(right), _acc(1)
    with pytest.raises(ValueError):
        ctx.seam_moments_u16(dl, dr, 96, 64, 49, 1, acc)            # 2 fold > W
    with pytest.raises(ValueError):
        ctx.seam_moments_u16(dl, dr, 96, 64, 8, 3, acc)             # spp
    with pytest.raises(ValueError):
        ctx.seam_moments_u16(dl, dr, 96, 64, 8, 1, acc, 5, 4)       # empty valid range


# ---- balanced stitch ------------------------------------------------------------------------------------------------------------
def _stitch(ctx, left, right, W, L, fold, spp, G, O, h, valid_min=1):
    import torch
    out = torch.zeros(L, 2 * (W - fold) * spp, dtype=torch.uint16, device="cuda")
    ctx.stitch_balanced_u16(_cuda(left), _cuda(right), out, W * spp, L, fold * spp, spp, _cuda(np.asarray(G, np.int32)),
                            _cuda(np.asarray(O, np.int32)), h, valid_min)
    ctx.sync()
    return out.cpu().numpy()


@pytest.mark.parametrize("params", sorted(PARAMS))
@pytest.mark.parametrize("h", ["0", "1", "fold"])
@pytest.mark.parametrize("W,L,fold,spp", STITCH_SHAPES)
def test_stitch_equals_restatement(ctx, W, L, fold, spp, h, params):
    h = fold if h == "fold" else int(h)
    G, O = (v[:spp] for v in PARAMS[params])
    left, right = _pair(W, L, fold, spp)
    got = _stitch(ctx, left, right, W, L, fold, spp, G, O, h)
    assert np.array_equal(got, ref.stitch(left, right, fold, spp, G, O, h, 1))
    # preconditions: the balance clamps at the end the set aims at, and both images have "no data" inside the blend zone
    if L > 1:
        b = right.reshape(L, W, spp)[:, fold:]
        bb = ref.balance(b, G, O)
        assert (bb[b > 0] == 0).any() if params == "low" else (bb == 65535).any()
        a, b = ref.overlap(left, right, fold, spp)
        za, zb = a[:, fold - h:fold + h] == 0, b[:, fold - h:fold + h] == 0
        assert not h or ((za & ~zb).any() and (~za & zb).any() and (za & zb).any())


@pytest.mark.parametrize("W,L,fold,spp", STITCH_SHAPES)
def test_identity_without_feather_is_the_plain_stitch(ctx, W, L, fold, spp):
    import torch
    left, right = _pair(W, L, fold, spp)
    plain = torch.zeros(L, 2 * (W - fold) * spp, dtype=torch.uint16, device="cuda")
    ctx.stitch_rows_u16(_cuda(left), _cuda(right), plain, W * spp, L, fold * spp)
    got = _stitch(ctx, left, right, W, L, fold, spp, [65536] * spp, [0] * spp, 0)
    assert np.array_equal(got, plain.cpu().numpy())
    assert np.array_equal(got, np.concatenate([left[:, :(W - fold) * spp], right[:, fold * spp:]], 1))


def test_stitch_more_than_one_trip_per_lane(ctx):
    """2 255 000 chunks: lanes of the vector kernel go through its outer loop a second time (module docstring)"""
    W, L, fold, spp = 4200, 2200, 100, 1
    assert (2 * (W - fold) // 8) * L > 256 * 8 * 256 * 4
    left, right = _pair(W, L, fold, spp)
    G, O = [70124], [-300 * 65536]
    got = _stitch(ctx, left, right, W, L, fold, spp, G, O, fold)
    assert np.array_equal(got, ref.stitch(left, right, fold, spp, G, O, fold, 1))


def test_valid_min_zero_blends_everything(ctx):
    """valid_min = 0: a zero is data like any other; a different result from valid_min = 1 on the same images"""
    W, L, fold, spp = 256, 300, 25, 4
    left, right = _pair(W, L, fold, spp)
    G, O = PARAMS["high"]
    got = _stitch(ctx, left, right, W, L, fold, spp, G, O, fold, 0)
    assert np.array_equal(got, ref.stitch(left, right, fold, spp, G, O, fold, 0))
    assert not np.array_equal(got, ref.stitch(left, right, fold, spp, G, O, fold, 1))


def test_stitch_bad_arguments_and_profiler(ctx):
    import torch
    W, L, fold = 96, 64, 8
    left, right = _pair(W, L, fold, 1)
    dl, dr = _cuda(left), _cuda(right)
    out = torch.zeros(L, 2 * (W - fold), dtype=torch.uint16, device="cuda")
    g, o = _cuda(np.array([65536], np.int32)), _cuda(np.array([0], np.int32))
    with pytest.raises(ValueError):
        ctx.stitch_balanced_u16(dl, dr, out, W, L, fold, 1, g, o, fold + 1, 1)     # h > fold
    with pytest.raises(ValueError):
        ctx.stitch_balanced_u16(dl, dr, out, W, L, fold, 2, g, o, 0, 1)            # spp
    ctx.profile_enable(True)
    ctx.profile_reset()
    ctx.stitch_balanced_u16(dl, dr, out, W, L, fold, 1, g, o, 2, 1)
    ctx.seam_moments_u16(dl, dr, W, L, fold, 1, _acc(1))
    ctx.sync()
    prof = ctx.profile()
    ctx.profile_enable(False)
    assert prof["stitch_balanced_kernel"][1] == 1 and prof["seam_moments_kernel"][1] == 1
