"""GPU: oip_retile_u16 / oip_untile_u16, the two layout kernels between a raster and its tile-major form, against the numpy
restatement in _cog_ref.py.  Copies: every comparison is equality of all samples.  The data is noise over the whole u16 range
without the value 5000, and every destination is pre-filled with 5000, so a sample a kernel left out shows."""
import numpy as np
import pytest

import _cog_ref as ref

pytestmark = pytest.mark.gpu
FILL = 5000
PITCH = 16416                                 # samples a line of the shared raster: 4100 pixels of 4 samples, and 16 more


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _filled(shape):
    import torch
    return torch.full(shape, FILL, dtype=torch.int16, device="cuda").view(torch.uint16)


@pytest.fixture(scope="module")
def raster():
    rng = np.random.default_rng(77)
    img = rng.integers(0, 65536, (520, PITCH)).astype(np.uint16)
    img[img == FILL] = FILL + 1
    return img, _cuda(img)


def _sizes(T):
    return [1, T - 1, T, T + 1, 2 * T + 3]


def _forms(img, d, w, h, spp):
    """(name, device pointer, pitch, host window): a window of the wide lines on an aligned base (the vector kernels), a tight
    copy (vector where w * spp is a multiple of 8, else a lane per sample), a window one sample to the right (a lane per sample)"""
    win = np.ascontiguousarray(img[:h, :w * spp])
    yield "window", d.data_ptr(), PITCH, win, d
    t = _cuda(win)
    yield "tight", t.data_ptr(), w * spp, win, t
    yield "offset", d.data_ptr() + 2, PITCH, np.ascontiguousarray(img[:h, 1:1 + w * spp]), d


def _retile(ctx, ptr, pitch, w, h, spp, T, cuts=1):
    tx, ty = ref.grid(w, h, T)
    out = _filled((tx * ty, T, T * spp))
    step = -(-ty // cuts)
    for j0 in range(0, ty, step):
        nr = min(step, ty - j0)
        ctx.retile_u16(ptr, pitch, w, h, spp, T, j0, nr, out.data_ptr() + 2 * j0 * tx * T * T * spp)
    ctx.sync()
    return out


def _untile(ctx, tiles, w, h, spp, T, pad=0, cuts=1):
    tx, ty = ref.grid(w, h, T)
    out = _filled((h, w * spp + pad))
    step = -(-ty // cuts)
    for j0 in range(0, ty, step):
        nr = min(step, ty - j0)
        ctx.untile_u16(tiles.data_ptr() + 2 * j0 * tx * T * T * spp, w, h, spp, T, j0, nr, out, w * spp + pad)
    ctx.sync()
    return out.cpu().numpy()


@pytest.mark.parametrize("spp", [1, 4])
@pytest.mark.parametrize("T", [16, 64, 256])
def test_shapes_forms_and_round_trip(ctx, raster, T, spp):
    """w, h in {1, T - 1, T, T + 1, 2 T + 3} and w = 4100 (several workgroups across a line), each raster form: the tile-major
    buffer is the restatement's, padding included and no sample left at the fill value; untile of it is the image again, into a
    tight destination, a pitched one on the vector path (slack 8) and one on the lane-per-sample path (slack 5), slack untouched"""
    img, d = raster
    for w in _sizes(T) + [4100]:
        for h in (_sizes(T) if w != 4100 else [1, T + 1]):
            for name, ptr, pitch, win, _keep in _forms(img, d, w, h, spp):
                want = ref.retile(win, spp, T)
                tiles = _retile(ctx, ptr, pitch, w, h, spp, T)
                assert np.array_equal(tiles.cpu().numpy(), want), (w, h, name)
                if name == "offset":
                    continue
                for pad in (0, 8, 5):
                    back = _untile(ctx, tiles, w, h, spp, T, pad)
                    assert np.array_equal(back[:, :w * spp], win), (w, h, name, pad)
                    assert (back[:, w * spp:] == FILL).all(), (w, h, name, pad)


@pytest.mark.parametrize("spp", [1, 4])
@pytest.mark.parametrize("T", [16, 64])
def test_tile_row_batches_equal_one_call(ctx, raster, T, spp):
    """the grid cut into 1, 2 and ty calls by tile_row0 / tile_rows: the bytes of one call, both ways, on both kinds of kernel"""
    img, d = raster
    w, h = 2 * T + 3, 5 * T + 1
    for name, ptr, pitch, win, _keep in _forms(img, d, w, h, spp):
        want = ref.retile(win, spp, T)
        ty = ref.grid(w, h, T)[1]
        for cuts in (1, 2, ty):
            tiles = _retile(ctx, ptr, pitch, w, h, spp, T, cuts)
            assert np.array_equal(tiles.cpu().numpy(), want), (name, cuts)
            for pad in (0, 5):
                assert np.array_equal(_untile(ctx, tiles, w, h, spp, T, pad, cuts)[:, :w * spp], win), (name, cuts, pad)
    # a batch alone, into a buffer of its own size: tile rows [2, 4)
    tx = ref.grid(w, h, T)[0]
    part = _filled((2 * tx, T, T * spp))
    ctx.retile_u16(d, PITCH, w, h, spp, T, 2, 2, part)
    ctx.sync()
    assert np.array_equal(part.cpu().numpy(), ref.retile(img[:h, :w * spp], spp, T, 2, 2))


@pytest.mark.parametrize("spp", [1, 4])
def test_untile_ignores_the_padding(ctx, raster, spp):
    """the padding of the edge tiles overwritten with garbage: the same image, and the slack of a pitched destination stays"""
    img, d = raster
    T, w, h = 64, 2 * 64 + 3, 64 + 9
    win = np.ascontiguousarray(img[:h, :w * spp])
    tx, ty = ref.grid(w, h, T)
    t = ref.retile(win, spp, T).reshape(ty, tx, T, T, spp).copy()
    t[-1, :, h - (ty - 1) * T:] = 0xDEAD
    t[:, -1, :, w - (tx - 1) * T:] = 0xBEEF
    dirty = _cuda(t.reshape(tx * ty, T, T * spp))
    for pad in (0, 8, 5):
        back = _untile(ctx, dirty, w, h, spp, T, pad)
        assert np.array_equal(back[:, :w * spp], win) and (back[:, w * spp:] == FILL).all(), pad


def test_invalid_arguments(ctx, raster):
    _, d = raster
    out = _filled((64, 16, 16))
    ok = dict(img=d, src_pitch=PITCH, w=40, h=20, spp=1, T=16, tile_row0=0, tile_rows=2, tiles=out)
    ctx.retile_u16(**ok)
    ctx.retile_u16(**dict(ok, tile_rows=0))                    # a no-op
    ctx.sync()
    for bad in (dict(spp=2), dict(spp=0), dict(w=0), dict(h=0), dict(h=1 << 31), dict(T=0), dict(T=8), dict(T=24), dict(T=1040), dict(src_pitch=39),
                dict(tile_row0=-1), dict(tile_row0=1, tile_rows=2), dict(tile_rows=3), dict(tile_rows=-1), dict(tiles=out.data_ptr() + 2),
                dict(tiles=d), dict(img=None), dict(tiles=None)):
        with pytest.raises(ValueError):
            ctx.retile_u16(**dict(ok, **bad))
    img = _filled((20, 40))
    oku = dict(tiles=out, w=40, h=20, spp=1, T=16, tile_row0=0, tile_rows=2, img=img, dst_pitch=40)
    ctx.untile_u16(**oku)
    ctx.sync()
    for bad in (dict(spp=3), dict(w=-1), dict(T=17), dict(dst_pitch=39), dict(tile_row0=2, tile_rows=1), dict(tiles=out.data_ptr() + 8), dict(img=out)):
        with pytest.raises(ValueError):
            ctx.untile_u16(**dict(oku, **bad))
