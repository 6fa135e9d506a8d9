"""GPU: oip_sigma_filter_u16 at addresses past 2^31 samples, where the lines of a real strip live, on the probe raster of
tests/_bigraster.py (32760 x 65600 = 2 149 056 000 samples: one constant on every line but a head and a tail band of seeded
noise), at radius 3, once at spp 1 and once as 8190 x 65600 pixels of 4 samples.  Inside each band widened by the halo of 3
lines the output is the restatement's (_denoise_ref.py); on every other line it is the constant, a constant neighbourhood being
a fixed point; d_stats[0] counts the samples with data of the whole raster.  The tail band's lines from 65553 on lie wholly past
2^31 samples, in the source and in the destination: a kernel that computed `line * pitch` in 32 bits reads the head of the
raster for them and writes them over it; the CPU twin at the bottom (not `gpu`) shows on _bigraster.SMALL that the check rejects
both."""
import gc

import numpy as np
import pytest

import _bigraster as br
import _denoise_ref as ref

SEED = 53
RADIUS = 3


def _noises(geo):
    # 1380 .. 1619 around the constant 1500, against thr[5] = 30 + 5 ch: some neighbours are members, some are not; zeros and 65535
    return [br.band_noise(geo, k, SEED, lo=1380, hi=1620, specials=(0, 65535), rate=0.01) for k in (0, 1)]


def _bands(geo, noises, spp):
    out = []
    for k, (lo, hi, oa, ob) in enumerate(br.band_windows(geo, halo=RADIUS)):
        y = ref.sigma_filter(br.band_input(geo, k, noises[k], lo, hi), ref.table(spp), RADIUS, None, 1, spp)
        out.append((oa, ob, y[oa - lo:ob - lo]))
    return out


def _valid(geo, noises):
    return geo.W * (geo.L - sum(n.shape[0] for n in noises)) + sum(int((n >= 1).sum()) for n in noises)


@pytest.mark.gpu
@pytest.mark.parametrize("spp", [1, 4])
def test_whole_raster(ctx, spp):
    """peak device memory: 2 x 4.3 GB (the raster and its image)"""
    import torch
    geo = br.BIG
    f = geo.assert_crosses()
    assert f * geo.W >= br.TWO31 and geo.tail[0] < f < geo.L                       # read and written past 2^31: the tail band's lines from f on
    noises = _noises(geo)
    src = br.device_raster(geo, noises)
    out = torch.full((geo.L, geo.W), 0x5A5A, dtype=torch.int16, device="cuda").view(torch.uint16)
    stats = torch.zeros(4, dtype=torch.int64, device="cuda")
    ctx.sigma_filter_u16(src, out, geo.W // spp, geo.L, spp, RADIUS, torch.from_numpy(ref.table(spp)).cuda(), None, 1, stats)
    ctx.sync()
    bands = _bands(geo, noises, spp)
    assert all((w != br.band_input(geo, k, noises[k], oa, ob)).mean() > 0.2 for k, (oa, ob, w) in enumerate(bands))      # the filter acted in the bands
    br.check_rows(out, bands, br.CONST)
    assert int(stats[0]) == _valid(geo, noises)
    del src, out
    gc.collect()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("spp", [1, 4])
def test_check_rejects_a_wrapped_offset(spp):
    """the same check on the host at _bigraster.SMALL (64 x 240, offsets wrap at element 192 * 64 + 8): the restatement of the
    whole raster passes; the raster read through a wrapping offset does not, nor does the image stored through one"""
    geo = br.SMALL
    noises = _noises(geo)
    x = br.host_raster(geo, noises)
    bands = _bands(geo, noises, spp)
    p = ref.sigma_filter_parts(x, ref.table(spp), RADIUS, None, 1, spp)
    truth = p["out"]
    br.check_rows(truth, bands, br.CONST)
    assert p["stats"][0] == _valid(geo, noises)
    assert br.rejects(ref.sigma_filter(br.wrapped_read(x, geo.wrap), ref.table(spp), RADIUS, None, 1, spp), bands, br.CONST)
    assert br.rejects(br.wrapped_store(truth, geo.wrap, 0x5A5A), bands, br.CONST)
    bad = truth.copy()
    bad[-1, -1] ^= 1
    assert br.rejects(bad, bands, br.CONST)
