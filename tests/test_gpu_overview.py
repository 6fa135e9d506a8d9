"""GPU: oip_halve_u16, one level of the overview pyramid, against the numpy restatement in _overview_ref.py.  Exact integer
arithmetic: every comparison is equality of all samples.  The data is 12-bit noise with 30 % zeros and 2 % 65535, so blocks
without data and mixed blocks both occur; every output is then in [0, 4095] or >= 16384 (a mean with a 65535 in it), and an
output buffer pre-filled with 5000 shows every sample the kernel left out."""
import numpy as np
import pytest

import _overview_ref as ref

pytestmark = pytest.mark.gpu
WIDTHS = [1, 2, 3, 7, 8, 9, 15, 16, 17, 63, 64, 65, 257]
ROWS = [1, 2, 3, 63, 64, 65, 129]
FILL = 5000


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _noise(shape, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(1, 4096, shape).astype(np.uint16)
    x[rng.random(shape) < 0.30] = 0
    x[rng.random(shape) < 0.02] = 65535
    return x


def _halve(ctx, d_src, src_pitch, w, rows, spp, valid_min, offset=0, dst_pad=0):
    """-> the whole output buffer on the host, (ceil(rows / 2), ceil(w / 2) * spp + dst_pad) uint16, pre-filled with FILL"""
    import torch
    on, oh = -(-w // 2) * spp, -(-rows // 2)
    out = torch.full((oh, on + dst_pad), FILL, dtype=torch.int16, device="cuda").view(torch.uint16)
    ctx.halve_u16(d_src.data_ptr() + 2 * offset, src_pitch, w, rows, spp, valid_min, out, on + dst_pad)
    ctx.sync()
    return out.cpu().numpy()


@pytest.fixture(scope="module")
def raster():
    """one noise raster shared by the cases: 300 lines of 16416 samples (4100 pixels of 4 samples, and 16 more)"""
    img = _noise((300, 16416), 21)
    return img, _cuda(img)


@pytest.mark.parametrize("spp", [1, 4])
@pytest.mark.parametrize("valid_min", [0, 1, 300])
def test_shapes(ctx, raster, spp, valid_min):
    """every w x rows of the lists as a window of the 16416-sample lines (the vector kernel: a partial last lane at most widths,
    one pixel of two at odd widths of spp 4, a last line without a partner at odd heights, 129 lines: a second workgroup line
    range) and as a tight copy (the lane-per-sample kernel wherever w * spp is no multiple of 8)"""
    img, d = raster
    for w in WIDTHS:
        for rows in ROWS:
            win = np.ascontiguousarray(img[:rows, :w * spp])
            want = ref.halve(win, valid_min, spp)
            assert np.array_equal(_halve(ctx, d, 16416, w, rows, spp, valid_min), want), (w, rows, "window")
            assert np.array_equal(_halve(ctx, _cuda(win), w * spp, w, rows, spp, valid_min), want), (w, rows, "tight")


@pytest.mark.parametrize("spp", [1, 4])
def test_several_workgroups_in_x_and_y(ctx, raster, spp):
    """4100 x 300: three (spp 1) or nine (spp 4) workgroups across a line and five line ranges of 64 lines"""
    img, d = raster
    for vm in (0, 1):
        want = ref.halve(img[:, :4100 * spp], vm, spp)
        assert np.array_equal(_halve(ctx, d, 16416, 4100, 300, spp, vm), want)
    tight = np.ascontiguousarray(img[:, :4100])                # 4100 samples a line: no multiple of 8, the lane-per-sample kernel
    assert np.array_equal(_halve(ctx, _cuda(tight), 4100, 4100 // spp, 300, spp, 1), ref.halve(tight, 1, spp))


@pytest.mark.parametrize("spp", [1, 4])
@pytest.mark.parametrize("dst_pad", [8, 5])
def test_window_and_padded_output(ctx, raster, spp, dst_pad):
    """src_pitch > w * spp and dst_pitch larger than the output line (by 8: 8-byte stores; by 5: 2-byte stores): the padding of
    the output keeps what it held"""
    img, d = raster
    w, rows = 1001, 67
    got = _halve(ctx, d, 16416, w, rows, spp, 1, dst_pad=dst_pad)
    on = -(-w // 2) * spp
    assert np.array_equal(got[:, :on], ref.halve(img[:rows, :w * spp], 1, spp))
    assert (got[:, on:] == FILL).all()


@pytest.mark.parametrize("spp", [1, 4])
def test_misaligned_base_and_pitch(ctx, raster, spp):
    """a base shifted by one sample, and a pitch that is no multiple of 8 samples: the lane-per-sample kernel, the same result as
    the vector kernel on an aligned copy"""
    img, d = raster
    w, rows = 500, 131
    win = np.ascontiguousarray(img[:rows, 1:1 + w * spp])
    want = ref.halve(win, 1, spp)
    assert np.array_equal(_halve(ctx, d, 16416, w, rows, spp, 1, offset=1), want)
    assert np.array_equal(_halve(ctx, _cuda(win), w * spp, w, rows, spp, 1), want)
    odd = np.ascontiguousarray(img[:rows, :w * spp + 4])       # pitch = w * spp + 4
    assert np.array_equal(_halve(ctx, _cuda(odd), w * spp + 4, w, rows, spp, 1), ref.halve(odd[:, :w * spp], 1, spp))


@pytest.mark.parametrize("spp", [1, 4])
def test_cut_at_an_even_line_equals_one_call(ctx, raster, spp):
    """130 lines as 64 + 66 into the rows of one output, against one call"""
    import torch
    img, d = raster
    w = 300
    on = -(-w // 2) * spp
    one = _halve(ctx, d, 16416, w, 130, spp, 1)
    out = torch.full((65, on), FILL, dtype=torch.int16, device="cuda").view(torch.uint16)
    ctx.halve_u16(d, 16416, w, 64, spp, 1, out, on)
    ctx.halve_u16(d.data_ptr() + 2 * 64 * 16416, 16416, w, 66, spp, 1, out.data_ptr() + 2 * 32 * on, on)
    ctx.sync()
    assert np.array_equal(out.cpu().numpy(), one) and np.array_equal(one, ref.halve(img[:130, :w * spp], 1, spp))


@pytest.mark.parametrize("spp", [1, 4])
def test_five_chained_levels(ctx, raster, spp):
    """67 x 133 -> 34 x 67 -> 17 x 34 -> 9 x 17 -> 5 x 9 -> 3 x 5, each level from the device's own previous one"""
    import torch
    img, _ = raster
    w, h = 67, 133
    x = np.ascontiguousarray(img[:h, :w * spp])
    cur = _cuda(x)
    for k, want in enumerate(ref.pyramid(x, 5, 1, spp)):
        nw, nh = -(-w // 2), -(-h // 2)
        nxt = torch.full((nh, nw * spp), FILL, dtype=torch.int16, device="cuda").view(torch.uint16)
        ctx.halve_u16(cur, w * spp, w, h, spp, 1, nxt, nw * spp)
        ctx.sync()
        assert np.array_equal(nxt.cpu().numpy(), want), k + 1
        cur, w, h = nxt, nw, nh
    assert (w, h) == (3, 5)


def test_invalid_arguments(ctx, raster):
    import torch
    _, d = raster
    out = torch.zeros((64, 64), dtype=torch.int16, device="cuda").view(torch.uint16)
    ok = dict(src=d, src_pitch=16416, w=16, rows=8, spp=1, valid_min=1, dst=out, dst_pitch=8)
    ctx.halve_u16(**ok)
    ctx.halve_u16(**dict(ok, rows=0))                          # a no-op
    ctx.sync()
    for bad in (dict(spp=2), dict(spp=3), dict(spp=0), dict(w=0), dict(w=-1), dict(rows=-1), dict(rows=1 << 31), dict(valid_min=-1),
                dict(valid_min=65536), dict(src_pitch=15), dict(dst_pitch=7), dict(spp=4, dst_pitch=31), dict(dst=d)):
        with pytest.raises(ValueError):
            ctx.halve_u16(**dict(ok, **bad))
