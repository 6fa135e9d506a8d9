"""GPU: oip_halve_u16 at addresses past 2^31 samples, where the lines of a real strip live, on the probe raster of
tests/_bigraster.py (32760 x 65600 = 2 149 056 000 samples: one constant on every line but a head and a tail band of seeded
noise), once at spp 1 and once as 8190 x 65600 pixels of 4 samples.  The (32800, 16380) output: lines [0, 12) are the halved
head band, lines [32760, 32800) the halved tail band -- whose source lines from 65553 on lie wholly past 2^31 samples --, every
other line is the constant (a mean of four equal samples).  A kernel that computed `row * pitch` in 32 bits reads the head of
the raster for the tail band; the CPU twin at the bottom (not `gpu`) shows on _bigraster.SMALL that the check rejects that."""
import gc

import numpy as np
import pytest

import _bigraster as br
import _overview_ref as ref

SEED = 31


def _bands(geo, noises, spp):
    assert geo.head[1] % 2 == 0 and geo.tail[0] % 2 == 0 and geo.L % 2 == 0          # no output line mixes a band and the constant
    return [(a // 2, b // 2, ref.halve(n, 1, spp)) for (a, b), n in zip((geo.head, geo.tail), noises)]


@pytest.mark.gpu
@pytest.mark.parametrize("spp", [1, 4])
def test_halve_whole_raster(ctx, spp):
    """peak device memory: 4.3 GB (the raster) + 1.1 GB (the level)"""
    import torch
    geo = br.BIG
    f = geo.assert_crosses()
    assert f * geo.W >= br.TWO31 and geo.tail[0] < f < geo.L                       # read past 2^31: the tail band's lines from f on
    noises = [br.band_noise(geo, k, SEED) for k in (0, 1)]
    src = br.device_raster(geo, noises)
    out = torch.full((geo.L // 2, geo.W // 2), 0xABCD - 65536, dtype=torch.int16, device="cuda").view(torch.uint16)
    assert out.shape == (32800, 16380)
    ctx.halve_u16(src, geo.W, geo.W // spp, geo.L, spp, 1, out, geo.W // 2)
    ctx.sync()
    bands = _bands(geo, noises, spp)
    assert [(a, b) for a, b, _ in bands] == [(0, 12), (32760, 32800)]
    br.check_rows(out, bands, br.CONST)
    del src, out
    gc.collect()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("spp", [1, 4])
def test_check_rejects_a_wrapped_read(spp):
    """the same check on the host at _bigraster.SMALL (64 x 240, offsets wrap at element 192 * 64 + 8): the restatement of the
    whole raster passes; the raster read through a wrapping offset does not, and differs on most of the lines past the wrap"""
    geo = br.SMALL
    noises = [br.band_noise(geo, k, SEED) for k in (0, 1)]
    x = br.host_raster(geo, noises)
    bands = _bands(geo, noises, spp)
    truth = ref.halve(x, 1, spp)
    br.check_rows(truth, bands, br.CONST)
    wrapped = ref.halve(br.wrapped_read(x, geo.wrap), 1, spp)
    assert br.rejects(wrapped, bands, br.CONST)
    beyond = slice(-(-geo.assert_crosses() // 2), geo.L // 2)
    assert float((wrapped[beyond] != truth[beyond]).mean()) >= 0.5
    bad = truth.copy()
    bad[-1, -1] ^= 1
    assert br.rejects(bad, bands, br.CONST)
