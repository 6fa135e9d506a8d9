"""GPU: the three kernels of `oip quicklook` -- oip_decimate_box_u16, oip_histogram_u16, oip_apply_lut_u8 -- against the
numpy restatement in _quicklook_ref.py.  Exact integer arithmetic: every comparison is equality of all samples.  Shapes are
the smallest at which each mechanism of the kernels can go wrong (see the docstrings)."""
import numpy as np
import pytest

import _quicklook_ref as ref

pytestmark = pytest.mark.gpu
FACTORS = [2, 4, 8, 16, 32, 64]


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _random(shape, seed, lo=0, hi=65536):
    return np.random.default_rng(seed).integers(lo, hi, shape, dtype=np.uint16)


def _decimate(ctx, d_src, pitch, w, rows, spp, F, offset=0):
    """-> (spp, ceil(rows / F), ceil(w / F)) uint16 on the host; the output starts as 0xFFFF so that a sample the kernel
    leaves out shows (a decimated random image holds that value with probability ~0)"""
    import torch
    ow, oh = -(-w // F), -(-rows // F)
    out = torch.full((spp, oh, ow), -1, dtype=torch.int16, device="cuda").view(torch.uint16)
    ctx.decimate_box_u16(d_src.data_ptr() + 2 * offset, pitch, w, rows, spp, F, out, ow, oh * ow)
    ctx.sync()
    return out.cpu().numpy()


@pytest.fixture(scope="module")
def raster():
    """one random raster shared by the spp = 1 cases: 64 * 70 + 3 lines (the tallest case) of pitch 1024"""
    img = _random((64 * 70 + 3, 1024), 11)
    return img, _cuda(img)


@pytest.mark.parametrize("F", FACTORS)
def test_vector_kernel_partial_lane_group_and_blocks(ctx, raster, F):
    """w = 1000 in lines of pitch 1024: at F >= 16 the last group of lanes is partial (its lanes from column 1000 on hold
    nothing of the image) and every F that does not divide 1000 leaves a partial last block; rows = 70 F + 3: several
    workgroup line ranges (multiples of 64 lines) and a partial bottom block"""
    img, d = raster
    rows = 70 * F + 3
    got = _decimate(ctx, d, 1024, 1000, rows, 1, F)
    assert np.array_equal(got[0], ref.decimate(img[:rows, :1000], F))


@pytest.mark.parametrize("F", FACTORS)
def test_vector_kernel_partial_group_inside_the_image(ctx, raster, F):
    """w = 1003: the lane group at column 1000 holds 3 columns of the image and 5 behind it, which must not be summed"""
    img, d = raster
    rows = 3 * F + 1
    got = _decimate(ctx, d, 1024, 1003, rows, 1, F)
    assert np.array_equal(got[0], ref.decimate(img[:rows, :1003], F))


@pytest.mark.parametrize("F", FACTORS)
def test_lane_groups_across_a_wave_boundary(ctx, F):
    """w = 8 * 64 * 3 + 8: three full waves of lanes and one lane more, whose group (8 lanes at F = 64) starts a fourth wave"""
    w, rows = 8 * 64 * 3 + 8, 2 * F + 1
    img = _random((rows, w), 15)
    got = _decimate(ctx, _cuda(img), w, w, rows, 1, F)
    assert np.array_equal(got[0], ref.decimate(img, F))


@pytest.mark.parametrize("F", FACTORS)
def test_fallback_kernel_odd_pitch(ctx, F):
    """w = pitch = 1001: no 16-byte alignment of the lines, the block-per-lane kernel; rows = 70 F + 3 as above"""
    rows = 70 * F + 3
    img = _random((rows, 1001), 12 + F)
    got = _decimate(ctx, _cuda(img), 1001, 1001, rows, 1, F)
    assert np.array_equal(got[0], ref.decimate(img, F))


@pytest.mark.parametrize("F", FACTORS)
def test_window_two_bytes_off_alignment_equals_aligned_copy(ctx, raster, F):
    """the same 1000 x (3 F + 2) samples as a window that starts at column 1 (fallback kernel) and as an aligned copy (vector
    kernel): equal to each other and to the restatement"""
    img, d = raster
    rows = 3 * F + 2
    win = np.ascontiguousarray(img[:rows, 1:1001])
    off = _decimate(ctx, d, 1024, 1000, rows, 1, F, offset=1)
    aligned = _decimate(ctx, _cuda(win), 1000, 1000, rows, 1, F)
    assert np.array_equal(off, aligned) and np.array_equal(off[0], ref.decimate(win, F))


@pytest.mark.parametrize("F", FACTORS)
def test_degenerate_shapes(ctx, raster, F):
    """one line; one column (pitch 8: vector kernel, pitch 1: fallback)"""
    img, d = raster
    assert np.array_equal(_decimate(ctx, d, 1024, 1000, 1, 1, F)[0], ref.decimate(img[:1, :1000], F))
    col = _random((70, 8), 13)
    assert np.array_equal(_decimate(ctx, _cuda(col), 8, 1, 70, 1, F)[0], ref.decimate(col[:, :1], F))
    one = np.ascontiguousarray(col[:, :1])
    assert np.array_equal(_decimate(ctx, _cuda(one), 1, 1, 70, 1, F)[0], ref.decimate(one, F))


@pytest.mark.parametrize("spp,pitch", [(1, 200), (1, 201), (4, 800), (4, 802)])
def test_largest_sum(ctx, spp, pitch):
    """all samples 65535 at F = 64: S = 65535 * 4096 in a full block, the largest sum the 32-bit registers meet"""
    img = np.full((130, pitch), 65535, np.uint16)
    got = _decimate(ctx, _cuda(img), pitch, 200, 130, spp, 64)
    assert got.shape == (spp, 3, 4) and (got == 65535).all()


@pytest.mark.parametrize("F", FACTORS)
@pytest.mark.parametrize("w,pitch", [(250, 1000), (251, 1008), (251, 1004)])
def test_four_samples_de_interleave(ctx, F, w, pitch):
    """spp = 4: a lane owns 2 pixels.  w = 250: even; w = 251 in lines of 1008 samples: the last lane holds one pixel of the
    image and one behind it; pitch 1004 (not a multiple of 8): the fallback kernel"""
    rows = 2 * F + 3
    img = _random((rows, pitch), 14 + w)
    got = _decimate(ctx, _cuda(img), pitch, w, rows, 4, F)
    assert np.array_equal(got, ref.decimate(img[:, :4 * w].reshape(rows, w, 4), F))


@pytest.mark.parametrize("F", FACTORS)
def test_two_calls_equal_one(ctx, raster, F):
    """lines cut at a multiple of F into two calls, the second writing from output line cut / F on"""
    import torch
    img, d = raster
    w, rows, cut = 1000, 9 * F + 1, 4 * F
    ow, oh = -(-w // F), -(-rows // F)
    out = torch.full((oh, ow), -1, dtype=torch.int16, device="cuda").view(torch.uint16)
    ctx.decimate_box_u16(d, 1024, w, cut, 1, F, out, ow)
    ctx.decimate_box_u16(d.data_ptr() + 2 * cut * 1024, 1024, w, rows - cut, 1, F, out.data_ptr() + 2 * (cut // F) * ow, ow)
    ctx.sync()
    assert np.array_equal(out.cpu().numpy(), _decimate(ctx, d, 1024, w, rows, 1, F)[0])
    assert np.array_equal(out.cpu().numpy(), ref.decimate(img[:rows, :w], F))


def test_decimate_refuses_bad_arguments(ctx, raster):
    import torch
    _, d = raster
    out = torch.zeros(4096, dtype=torch.int16, device="cuda")
    for spp, F, pitch, dst_pitch in [(1, 3, 1024, 64), (1, 1, 1024, 64), (1, 128, 1024, 64), (2, 16, 1024, 64), (1, 16, 999, 64), (1, 16, 1024, 62)]:
        with pytest.raises(ValueError):
            ctx.decimate_box_u16(d, pitch, 1000, 16, spp, F, out, dst_pitch)


# ---- histogram ----------------------------------------------------------------------------------------------------------
def _hist(ctx, calls):
    import torch
    h = torch.zeros(65536, dtype=torch.int64, device="cuda")
    for d, pitch, w, rows in calls:
        ctx.histogram_u16(d, pitch, w, rows, h)
    ctx.sync()
    return h.cpu().numpy().view(np.uint64)


def test_histogram_random_12_bit(ctx):
    img = _random((1237, 1501), 21, 0, 4096)
    assert np.array_equal(_hist(ctx, [(_cuda(img), 1501, 1501, 1237)]), ref.histogram(img))


def test_histogram_all_values(ctx):
    """every one of the 65536 values, both halves of the value range, lines longer than a work item's span"""
    img = np.concatenate([np.arange(65536, dtype=np.uint16), _random(-65536 % 9001, 22)]).reshape(-1, 9001)
    want = ref.histogram(img)
    assert (want > 0).all()
    assert np.array_equal(_hist(ctx, [(_cuda(img), 9001, 9001, img.shape[0])]), want)


@pytest.mark.parametrize("value", [0, 2000, 40000, 65535])
def test_histogram_constant_image(ctx, value):
    """the contention case: 4 M samples on one bin"""
    import torch
    d = torch.full((2000, 2000), value - 65536 if value > 32767 else value, dtype=torch.int16, device="cuda").view(torch.uint16)
    got = _hist(ctx, [(d, 2000, 2000, 2000)])
    assert got[value] == 4000000 and got.sum() == 4000000


def test_histogram_adds_over_calls_and_takes_a_pitch(ctx):
    img = _random((300, 1024), 23, 0, 300)
    d = _cuda(img)
    got = _hist(ctx, [(d, 1024, 1000, 100), (d.data_ptr() + 2 * 100 * 1024, 1024, 1000, 200), (d.data_ptr() + 2 * 7, 1024, 333, 300)])
    assert np.array_equal(got, ref.histogram(img[:, :1000]) + ref.histogram(img[:, 7:340]))


# ---- look-up ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch", [1, 3])
@pytest.mark.parametrize("w,pitch", [(1001, 1001), (333, 512), (1, 1)])
def test_apply_lut(ctx, nch, w, pitch):
    import torch
    rows = 77
    planes = [_random((rows, pitch), 31 + c) for c in range(nch)]
    luts = np.random.default_rng(32).integers(0, 256, (nch, 65536), dtype=np.uint8)
    out = torch.full((rows, w, nch), 7, dtype=torch.uint8, device="cuda")
    d = [_cuda(p) for p in planes]
    ctx.apply_lut_u8(d, pitch, w, rows, _cuda(luts), out)
    ctx.sync()
    want = np.stack([luts[c][planes[c][:, :w]] for c in range(nch)], -1)
    assert np.array_equal(out.cpu().numpy(), want)
