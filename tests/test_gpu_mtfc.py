"""GPU: oip_convolve_u16 against the integer restatement (_mtfc_ref.py).  The arithmetic is exact, so every comparison is
equality.

Which kernel a shape takes (the aligned form needs a line of W * spp samples that is a multiple of 8; the bases torch hands
out are 16-byte aligned), and how it meets the 512-sample x 16-line tiles:
    (5, 1, 1), (1, 7, 1)  per-sample   smaller than a 9 x 9 kernel: every neighbour is a replicated border sample
    (96, 64, 1)           aligned      one tile across, four down
    (131, 100, 4)         per-sample   524 samples: two tiles across (the second 12 samples wide), seven down (the last 4 lines)
    (521, 257, 1)         per-sample   two tiles across (the second 9 samples wide), 17 down (the last a single line)
    (1024, 37, 1)         aligned      two full tiles across, three down (the last 5 lines)
    (256, 300, 4)         aligned      1024 samples: the horizontal halo of 4 * rx samples crosses the tile edge
    (8, 5000, 1)          aligned      one lane of a wave has work, 313 tiles down
The kernel takes one tile per block and has no grid-stride loop, so no shape is needed for a second trip."""
import functools

import numpy as np
import pytest

import _mtfc_ref as ref

pytestmark = pytest.mark.gpu

SHAPES = [(5, 1, 1), (1, 7, 1), (96, 64, 1), (131, 100, 4), (521, 257, 1), (1024, 37, 1), (256, 300, 4), (8, 5000, 1)]


def _identity(ky, kx):
    t = np.zeros((ky, kx), np.int32)
    t[ky // 2, kx // 2] = 4096
    return t


TAPS = {
    "design3": lambda: ref.quantise(ref.design3(0.25, 0.4, 2.0)),
    "random9x5": lambda: ref.random_taps(9, 5, 95),
    "random5x9": lambda: np.ascontiguousarray(ref.random_taps(9, 5, 95).T),
    "random7x3": lambda: ref.random_taps(7, 3, 73),
}


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _image(W, L, spp):
    """full-range data with 3 % zeros; shared by the tests of a shape, which leave it unchanged"""
    rng = np.random.default_rng(1000 * W + L)
    img = rng.integers(0, 65536, (L, W * spp), dtype=np.uint16)
    img[rng.random(img.shape) < 0.03] = 0
    return img


@functools.lru_cache(maxsize=None)
def _want(W, L, spp, name, valid_min):
    return ref.convolve(_image(W, L, spp), TAPS[name](), valid_min, spp)


def _convolve(ctx, img, W, L, spp, taps, valid_min=1):
    import torch
    out = torch.zeros(L, W * spp, dtype=torch.uint16, device="cuda")
    ctx.convolve_u16(_cuda(img), out, W, L, spp, taps, valid_min)
    ctx.sync()
    return out.cpu().numpy()


@pytest.mark.parametrize("name", sorted(TAPS))
@pytest.mark.parametrize("W,L,spp", SHAPES)
def test_equals_restatement(ctx, W, L, spp, name):
    img = _image(W, L, spp)
    got1 = _convolve(ctx, img, W, L, spp, TAPS[name](), 1)
    assert np.array_equal(got1, _want(W, L, spp, name, 1))
    got0 = _convolve(ctx, img, W, L, spp, TAPS[name](), 0)
    assert np.array_equal(got0, _want(W, L, spp, name, 0))
    if (img == 0).any():
        assert not np.array_equal(got0, got1)                       # no-data handling changes the result on the same image


@pytest.mark.parametrize("W,L,spp", SHAPES)
def test_identity_returns_the_input(ctx, W, L, spp):
    img = _image(W, L, spp)
    for ky, kx in [(1, 1), (3, 3), (9, 9)]:
        for vmin in (0, 1):
            assert np.array_equal(_convolve(ctx, img, W, L, spp, _identity(ky, kx), vmin), img)


def test_flipped_and_transposed_taps_differ(ctx):
    """the 9 x 5 set and its transpose are asymmetric: a kernel applied flipped or transposed gives another image"""
    W, L, spp = 96, 64, 1
    t = TAPS["random9x5"]()
    want = _want(W, L, spp, "random9x5", 1)
    assert np.abs(t.astype(np.int64)).sum() == 32767
    assert not np.array_equal(ref.convolve(_image(W, L, spp), t[::-1, ::-1], 1, spp), want)
    assert not np.array_equal(_want(W, L, spp, "random5x9", 1), want)


@pytest.mark.parametrize("W,L,spp", [(96, 64, 1), (131, 100, 4), (521, 257, 1)])
def test_tiles_without_no_data(ctx, W, L, spp):
    """no sample below valid_min anywhere: every tile takes the loop without the no-data select"""
    img = np.maximum(_image(W, L, spp), 5)
    t = TAPS["random9x5"]()
    assert np.array_equal(_convolve(ctx, img, W, L, spp, t, 5), ref.convolve(img, t, 5, spp))


@pytest.mark.parametrize("W,L,spp", [(96, 64, 1), (131, 100, 4)])
def test_top_and_bottom_of_int32(ctx, W, L, spp):
    img = np.full((L, W * spp), 65535, np.uint16)
    pos = np.full((9, 9), 404, np.int32)                            # 81 * 404 = 32724
    pos[4, 4] += 32767 - 81 * 404
    assert pos.sum() == 32767 and 32767 * 65535 + 2048 < 2 ** 31
    assert (_convolve(ctx, img, W, L, spp, pos, 1) == 65535).all()  # the top of int32, clamped to 65535
    neg = np.array([[-32767]], np.int32)                            # a negative sum: the shift floors, the clamp gives valid_min
    assert (_convolve(ctx, img, W, L, spp, neg, 1) == 1).all()
    assert (_convolve(ctx, img, W, L, spp, neg, 0) == 0).all()
    assert (_convolve(ctx, img, W, L, spp, neg, 300) == 300).all()


@pytest.mark.parametrize("W,L,spp,name", [(96, 64, 1, "random9x5"), (131, 100, 4, "random5x9"), (1024, 37, 1, "design3")])
def test_strip_cut_into_three_calls(ctx, W, L, spp, name):
    """each call sees only the lines it needs (its output lines and ry halo lines inside the image), uploaded to a buffer of
    their own, and writes at the start of a buffer of its own: together the bytes of one call"""
    import torch
    img, t = _image(W, L, spp), TAPS[name]()
    ry = t.shape[0] // 2
    cuts = [0, L // 3 + 1, 2 * L // 3 - 2, L]
    parts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        s0, s1 = max(0, a - ry), min(L, b + ry)
        out = torch.zeros(b - a, W * spp, dtype=torch.uint16, device="cuda")
        ctx.convolve_u16(_cuda(img[s0:s1]), out, W, L, spp, t, 1, src_row0=s0, src_rows=s1 - s0, out_row0=a, out_rows=b - a)
        parts.append(out)
    ctx.sync()
    assert cuts[1] > 0 and max(0, cuts[1] - ry) > 0                  # src_row0 > 0 is exercised
    assert np.array_equal(np.concatenate([p.cpu().numpy() for p in parts]), _want(W, L, spp, name, 1))


def test_misaligned_bases_take_the_per_sample_kernel(ctx):
    import torch
    W, L, spp = 96, 64, 1
    img, t = _image(W, L, spp), TAPS["design3"]()
    src = torch.zeros(L * W + 8, dtype=torch.uint16, device="cuda")
    src[1:1 + L * W] = _cuda(img).reshape(-1)
    out = torch.zeros(L * W + 8, dtype=torch.uint16, device="cuda")
    ctx.convolve_u16(src.data_ptr() + 2, out.data_ptr() + 6, W, L, spp, t, 1)
    ctx.sync()
    got = out.cpu().numpy()
    assert np.array_equal(got[3:3 + L * W].reshape(L, W), _want(W, L, spp, "design3", 1))
    assert not got[:3].any() and not got[3 + L * W:].any()          # nothing outside the destination raster


def test_bad_arguments_and_profiler(ctx):
    import torch
    W, L = 96, 64
    img = _cuda(_image(W, L, 1))
    out = torch.zeros(L, W, dtype=torch.uint16, device="cuda")
    ok = TAPS["design3"]()
    big = _identity(3, 3)
    big[0, 0], big[2, 2] = 14336, -14336                            # sum |t| = 32768
    for kw in [dict(taps=big), dict(valid_min=-1), dict(valid_min=65536), dict(spp=2), dict(spp=3), dict(W=0), dict(L=0),
               dict(taps=np.zeros((2, 3), np.int32)), dict(taps=np.zeros((3, 4), np.int32)), dict(taps=np.zeros((11, 1), np.int32)),
               dict(taps=np.zeros((1, 11), np.int32)),
               dict(src_row0=1, src_rows=L - 1),                    # output line 0 needs source line 0
               dict(src_rows=L - 1),                                # the last line is missing
               dict(out_row0=10, out_rows=20, src_row0=10, src_rows=20),        # no halo resident
               dict(out_row0=10, out_rows=20, src_row0=9, src_rows=21),         # the lower halo line is missing
               dict(out_row0=L - 4, out_rows=5),                    # output lines beyond the raster
               dict(dst=img)]:                                      # in place
        a = dict(dst=out, W=W, L=L, spp=1, taps=ok, valid_min=1, src_row0=0, src_rows=None, out_row0=0, out_rows=None)
        a.update(kw)
        with pytest.raises(ValueError):
            ctx.convolve_u16(img, a["dst"], a["W"], a["L"], a["spp"], a["taps"], a["valid_min"], a["src_row0"], a["src_rows"], a["out_row0"], a["out_rows"])
    full = _identity(3, 3)
    full[0, 0], full[2, 2] = 14336, -14335                          # sum |t| = 32767 is accepted
    ctx.convolve_u16(img, out, W, L, 1, full, 1)
    ctx.convolve_u16(img, out, W, L, 1, ok, 1, out_row0=10, out_rows=20, src_row0=9, src_rows=22)      # exactly the halo
    ctx.profile_enable(True)
    ctx.profile_reset()
    ctx.convolve_u16(img, out, W, L, 1, ok, 1)
    ctx.convolve_u16(img, out, W, L, 1, ok, 1, out_rows=0)          # no lines: no launch
    ctx.sync()
    prof = ctx.profile()
    ctx.profile_enable(False)
    assert prof["convolve_u16_kernel"][1] == 1
    assert np.array_equal(out.cpu().numpy(), _want(W, L, 1, "design3", 1))
