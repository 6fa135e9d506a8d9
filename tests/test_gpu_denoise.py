"""GPU: oip_sigma_filter_u16 against the integer restatement (_denoise_ref.py).  The arithmetic is exact, so every comparison is
equality.  The image is _denoise_ref.image (a ramp over every table level with noise of four amplitudes and 3 % zeros); at
521 x 257 x 1 it reaches every member count 1 .. (2r+1)^2 (test_denoise_cpu.py asserts that), so every divisor of the two means
is compared.

Which kernel a shape takes (the aligned form needs a line of W * spp samples that is a multiple of 8; the bases torch hands
out are 16-byte aligned), and how it meets the kernel's 512-sample x 16-line tiles (those of convolve.hip):
    (5, 1, 1), (1, 7, 1)  per-sample   smaller than a 7 x 7 window: every neighbour is a replicated border sample
    (96, 64, 1)           aligned      one tile across, four down
    (131, 100, 4)         per-sample   524 samples: two tiles across (the second 12 samples wide), seven down (the last 4 lines)
    (521, 257, 1)         per-sample   two tiles across (the second 9 samples wide), 17 down (the last a single line)
    (1024, 37, 1)         aligned      two full tiles across, three down (the last 5 lines)
    (256, 300, 4)         aligned      1024 samples: the horizontal halo of 4 * r samples crosses the tile edge
    (8, 5000, 1)          aligned      one lane of a wave has work, 313 tiles down
The kernel takes one tile per block and has no grid-stride loop, so no shape is needed for a second trip."""
import functools

import numpy as np
import pytest

import _denoise_ref as ref

pytestmark = pytest.mark.gpu

SHAPES = [(5, 1, 1), (1, 7, 1), (96, 64, 1), (131, 100, 4), (521, 257, 1), (1024, 37, 1), (256, 300, 4), (8, 5000, 1)]
RADII = [1, 2, 3]


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _image(W, L, spp):
    """shared by the tests of a shape, which leave it unchanged"""
    return ref.image(W, L, spp, 1000 * W + L + spp)


@functools.lru_cache(maxsize=None)
def _want(W, L, spp, radius, min_members, valid_min):
    return ref.sigma_filter_parts(_image(W, L, spp), ref.table(spp), radius, min_members, valid_min, spp)


def _filter(ctx, img, W, L, spp, radius, thr, min_members=None, valid_min=1, stats=None):
    import torch
    out = torch.zeros(L, W * spp, dtype=torch.uint16, device="cuda")
    ctx.sigma_filter_u16(_cuda(img), out, W, L, spp, radius, _cuda(thr), min_members, valid_min, stats)
    ctx.sync()
    return out.cpu().numpy()


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("W,L,spp", SHAPES)
def test_equals_restatement(ctx, W, L, spp, radius):
    """valid_min 0 and 1, min_members 1 and the default (2r + 1)"""
    img, thr = _image(W, L, spp), ref.table(spp)
    for vmin in (0, 1):
        for mm in (1, None):
            got = _filter(ctx, img, W, L, spp, radius, thr, mm, vmin)
            assert np.array_equal(got, _want(W, L, spp, radius, mm, vmin)["out"]), (vmin, mm)


@pytest.mark.parametrize("W,L,spp", [(96, 64, 1), (131, 100, 4)])
def test_valid_min_changes_the_result(ctx, W, L, spp):
    """a dark border whose zeros lie within thr[0] = 20 of their neighbours: data at valid_min 0, no data at 1"""
    img = _image(W, L, spp).copy()
    img[:, :20 * spp] = np.minimum(img[:, :20 * spp], 15)
    img[::3, 5 * spp:6 * spp] = 0
    got = [_filter(ctx, img, W, L, spp, 2, ref.table(spp), None, v) for v in (0, 1)]
    for g, v in zip(got, (0, 1)):
        assert np.array_equal(g, ref.sigma_filter(img, ref.table(spp), 2, None, v, spp))
    assert not np.array_equal(got[0], got[1]) and (got[1][img == 0] == 0).all() and (got[0][img == 0] != 0).any()


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("W,L,spp", [(96, 64, 1), (131, 100, 4), (521, 257, 1), (256, 300, 4)])
def test_counters(ctx, W, L, spp, radius):
    """d_stats equals the restatement's four counters; a second call adds to them; without d_stats the image is the same"""
    import torch
    img, thr = _image(W, L, spp), ref.table(spp)
    want = _want(W, L, spp, radius, None, 1)
    stats = torch.zeros(4, dtype=torch.int64, device="cuda")
    got = _filter(ctx, img, W, L, spp, radius, thr, None, 1, stats)
    assert stats.cpu().tolist() == want["stats"] and min(want["stats"]) > 0
    assert np.array_equal(got, want["out"])
    assert np.array_equal(_filter(ctx, img, W, L, spp, radius, thr, None, 1, None), got)
    want1 = _want(W, L, spp, radius, 1, 0)
    _filter(ctx, img, W, L, spp, radius, thr, 1, 0, stats)
    assert stats.cpu().tolist() == [a + b for a, b in zip(want["stats"], want1["stats"])] and want1["stats"][1] == 0


@pytest.mark.parametrize("W,L,spp,radius", [(96, 64, 1, 3), (131, 100, 4, 2), (1024, 37, 1, 1), (521, 257, 1, 3)])
def test_window_calls_give_the_bytes_of_one_call(ctx, W, L, spp, radius):
    """each call sees only the lines it needs (its output lines and `radius` halo lines inside the image), uploaded to a buffer of
    their own, and writes at the start of a buffer of its own: together the bytes, and the counters, of one call.  The first
    window starts at the raster's first line, the last ends at its last, the others have src_row0 > 0 and out_row0 > 0."""
    import torch
    img, thr = _image(W, L, spp), _cuda(ref.table(spp))
    want = _want(W, L, spp, radius, None, 1)
    cuts = [0, L // 3 + 1, 2 * L // 3 - 2, L]
    stats = torch.zeros(4, dtype=torch.int64, device="cuda")
    parts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        s0, s1 = max(0, a - radius), min(L, b + radius)
        out = torch.zeros(b - a, W * spp, dtype=torch.uint16, device="cuda")
        ctx.sigma_filter_u16(_cuda(img[s0:s1]), out, W, L, spp, radius, thr, None, 1, stats, src_row0=s0, src_rows=s1 - s0, out_row0=a, out_rows=b - a)
        parts.append(out)
    ctx.sync()
    assert cuts[1] - radius > 0
    assert np.array_equal(np.concatenate([p.cpu().numpy() for p in parts]), want["out"])
    assert stats.cpu().tolist() == want["stats"]


@pytest.mark.parametrize("W,L,spp", SHAPES)
def test_table_of_zeros_returns_the_input(ctx, W, L, spp):
    """T = 0: only the neighbours equal to the centre are members, and their mean is the centre"""
    img = _image(W, L, spp)
    for radius in RADII:
        for vmin in (0, 1):
            assert np.array_equal(_filter(ctx, img, W, L, spp, radius, np.zeros((spp, 256), np.uint16), 1, vmin), img)


def test_every_channel_has_its_table(ctx):
    """an image whose four channels are equal, tables that differ per channel: the channels differ, and each is what its table
    gives on the one-channel image"""
    W, L = 131, 100
    one = ref.image(W, L, 1, 77)
    img = np.repeat(one, 4, axis=1)
    thr = ref.table(4)
    got = _filter(ctx, img, W, L, 4, 2, thr).reshape(L, W, 4)
    for c in range(4):
        assert np.array_equal(got[:, :, c], ref.sigma_filter(one, thr[c:c + 1], 2))
    assert all(not np.array_equal(got[:, :, c], got[:, :, c + 1]) for c in range(3))
    same = _filter(ctx, img, W, L, 4, 2, np.repeat(thr[:1], 4, axis=0)).reshape(L, W, 4)
    assert all(np.array_equal(same[:, :, 0], same[:, :, c]) for c in range(1, 4))


def test_misaligned_bases_take_the_per_sample_kernel(ctx):
    import torch
    W, L, spp = 96, 64, 1
    img = _image(W, L, spp)
    src = torch.zeros(L * W + 8, dtype=torch.uint16, device="cuda")
    src[1:1 + L * W] = _cuda(img).reshape(-1)
    out = torch.zeros(L * W + 8, dtype=torch.uint16, device="cuda")
    stats = torch.zeros(4, dtype=torch.int64, device="cuda")
    ctx.sigma_filter_u16(src.data_ptr() + 2, out.data_ptr() + 6, W, L, spp, 2, _cuda(ref.table(1)), None, 1, stats)
    ctx.sync()
    got = out.cpu().numpy()
    want = _want(W, L, spp, 2, None, 1)
    assert np.array_equal(got[3:3 + L * W].reshape(L, W), want["out"]) and stats.cpu().tolist() == want["stats"]
    assert not got[:3].any() and not got[3 + L * W:].any()          # nothing outside the destination raster


def test_bad_arguments_and_profiler(ctx):
    """every bad argument is OIP_E_INVALID (ValueError) and launches nothing"""
    import torch
    W, L = 96, 64
    img = _cuda(_image(W, L, 1))
    thr = _cuda(ref.table(1))
    out = torch.zeros(L, W, dtype=torch.uint16, device="cuda")
    ctx.profile_enable(True)
    ctx.profile_reset()
    for kw in [dict(radius=0), dict(radius=4), dict(min_members=0), dict(min_members=26), dict(radius=1, min_members=10), dict(valid_min=-1),
               dict(valid_min=65536), dict(spp=2), dict(spp=3), dict(W=0), dict(L=0), dict(thr=None),
               dict(src_row0=1, src_rows=L - 1),                    # output line 0 needs source line 0
               dict(src_rows=L - 1),                                # the last line is missing
               dict(out_row0=10, out_rows=20, src_row0=10, src_rows=20),        # no halo resident
               dict(out_row0=10, out_rows=20, src_row0=8, src_rows=23),         # the lower halo line is missing
               dict(out_row0=L - 4, out_rows=5),                    # output lines beyond the raster
               dict(dst=img)]:                                      # in place
        a = dict(dst=out, W=W, L=L, spp=1, radius=2, thr=thr, min_members=5, valid_min=1, src_row0=0, src_rows=None, out_row0=0, out_rows=None)
        a.update(kw)
        with pytest.raises(ValueError):
            ctx.sigma_filter_u16(img, a["dst"], a["W"], a["L"], a["spp"], a["radius"], a["thr"], a["min_members"], a["valid_min"], None,
                                 a["src_row0"], a["src_rows"], a["out_row0"], a["out_rows"])
    ctx.sync()
    assert ctx.profile().get("sigma_filter_u16_kernel", (0.0, 0))[1] == 0      # none of them reached a launch
    ctx.sigma_filter_u16(img, out, W, L, 1, 2, thr, 25, 1)          # the largest min_members
    ctx.sigma_filter_u16(img, out, W, L, 1, 2, thr, 5, 1, None, out_row0=10, out_rows=20, src_row0=8, src_rows=24)      # exactly the halo
    ctx.profile_reset()
    ctx.sigma_filter_u16(img, out, W, L, 1, 2, thr)
    ctx.sigma_filter_u16(img, out, W, L, 1, 2, thr, out_rows=0)     # no lines: no launch
    ctx.sync()
    prof = ctx.profile()
    ctx.profile_enable(False)
    assert prof["sigma_filter_u16_kernel"][1] == 1
    assert np.array_equal(out.cpu().numpy(), _want(W, L, 1, 2, None, 1)["out"])
