"""GPU: oip_retile_u16 / oip_untile_u16 at addresses past 2^31 samples, on the probe raster of tests/_bigraster.py (32760 x 65600
= 2 149 056 000 samples, spp 1: one constant on every line but a head and a tail band of seeded noise), T = 256: 128 x 257 tiles,
2 155 872 256 samples of tile-major form.  Tile row 255 (lines 65280 .. 65535) ends just below 2^31 samples of the tile-major
buffer and holds the first 16 lines of the tail band; tile row 256 starts past 2^31, holds the other 64 and below them 192
copies of the last line.  A kernel that computed a tile's or a line's offset in 32 bits would put or find them elsewhere."""
import gc

import numpy as np
import pytest

import _bigraster as br
import _cog_ref as ref

SEED = 47
T = 256


@pytest.mark.gpu
def test_retile_untile_whole_raster(ctx):
    """peak device memory: 3 x 4.3 GB (the raster, the tile-major form, the raster again)"""
    import torch
    geo = br.BIG
    geo.assert_crosses()
    noises = [br.band_noise(geo, k, SEED) for k in (0, 1)]
    src = br.device_raster(geo, noises)
    tx, ty = ref.grid(geo.W, geo.L, T)
    assert (tx, ty) == (128, 257) and 255 * tx * T * T < br.TWO31 <= 256 * tx * T * T
    tiles = torch.full((ty * tx, T, T), 0xABCD - 65536, dtype=torch.int16, device="cuda").view(torch.uint16)
    ctx.retile_u16(src, geo.W, geo.W, geo.L, 1, T, 0, ty, tiles)
    ctx.sync()
    # the tile-major buffer: tile row 0 (the head band), tile rows 255 and 256 (the tail band and the replicated last line)
    # against the restatement on those lines; every tile between is the constant
    top = br.band_input(geo, 0, noises[0], 0, T)
    assert np.array_equal(tiles[:tx].cpu().numpy(), ref.retile(top, 1, T))
    bottom = br.band_input(geo, 1, noises[1], 255 * T, geo.L)
    want = ref.retile(bottom, 1, T)
    assert want.shape == (2 * tx, T, T)
    got = tiles[255 * tx:].cpu().numpy()
    assert np.array_equal(got[:tx], want[:tx]), "tile row 255 (below 2^31)"
    assert np.array_equal(got[tx:], want[tx:]), "tile row 256 (past 2^31)"
    assert np.array_equal(got[tx:, 64:], np.broadcast_to(got[tx:, 63:64], (tx, T - 64, T)))      # (the last line, repeated)
    flat = tiles[tx:255 * tx].view(torch.int16).reshape(-1, T * T)
    for c0 in range(0, flat.shape[0], 4096):
        assert bool((flat[c0:c0 + 4096] == br.CONST).all()), "a tile between the bands is not the constant"
    # and back
    out = torch.full((geo.L, geo.W), 0x1234, dtype=torch.int16, device="cuda").view(torch.uint16)
    ctx.untile_u16(tiles, geo.W, geo.L, 1, T, 0, ty, out, geo.W)
    ctx.sync()
    br.check_rows(out, [(geo.head[0], geo.head[1], noises[0]), (geo.tail[0], geo.tail[1], noises[1])], br.CONST)
    del src, tiles, out, flat
    gc.collect()
    torch.cuda.empty_cache()
