"""GPU: oip_mask_cells_u16 at addresses past 2^31 samples, where the lines of a real strip live, on the probe raster of
tests/_bigraster.py (32760 x 65600 = 2 149 056 000 samples: one constant on every line but a head and a tail band of seeded
noise), once at spp 1 with C 8 and once as 8190 x 65600 pixels of 4 samples with C 16.  On the constant lines every cell has the
constant's byte (0 at spp 1; CANDIDATE at spp 4, where four channels of 1500 pass every test); in the cell lines that touch the
head and the tail band -- whose source lines from 65553 on lie wholly past 2^31 samples -- the bytes are the restatement's
(_mask_ref.py).  A kernel that computed `line * pitch` in 32 bits reads the head of the raster for the tail band; the CPU twin at
the bottom (not `gpu`) shows on _bigraster.SMALL that the check rejects that."""
import gc

import numpy as np
import pytest

import _bigraster as br
import _mask_ref as ref

SEED = 53
KW = dict(valid_min=1, sat_level=4095, full=4095, band=ref.DEFAULT_BAND, q8=ref.DEFAULT_Q8)
CASES = [(1, 8, 0.002), (4, 16, 0.0003)]                               # spp, C, the share of zeros and of saturated samples in the bands


def _noises(geo, rate):
    return [br.band_noise(geo, k, SEED, specials=(0, 65535), rate=rate) for k in (0, 1)]


def _bands(geo, noises, spp, C):
    """[(first cell line, end, flags)] of the cell lines that touch a band"""
    out = []
    for k, (a, b) in enumerate((geo.head, geo.tail)):
        lo, hi = a // C * C, min(geo.L, -(-b // C) * C)
        want, _ = ref.cells(br.band_input(geo, k, noises[k], lo, hi), spp, C, **KW)
        out.append((lo // C, -(-hi // C), want))
    return out


def _const_byte(spp):
    f, _ = ref.cells(np.full((16, 64), br.CONST, np.uint16), spp, 16, **KW)
    assert (f == f[0, 0]).all()
    return int(f[0, 0])


@pytest.mark.gpu
@pytest.mark.parametrize("spp,C,rate", CASES)
def test_flags_whole_raster(ctx, spp, C, rate):
    """peak device memory: 4.3 GB (the raster) + 34 MB (the flags)"""
    import torch
    geo = br.BIG
    f = geo.assert_crosses()
    assert f * geo.W >= br.TWO31 and geo.tail[0] < f < geo.L                       # read past 2^31: the tail band's lines from f on
    noises = _noises(geo, rate)
    src = br.device_raster(geo, noises)
    gw, gh = ref.grid(geo.W // spp, geo.L, C)
    out = torch.full((gh, gw), 0xEE, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
    ctx.mask_cells_u16(src, geo.W, geo.W // spp, geo.L, spp, C, out, gw, cnt, KW["valid_min"], KW["sat_level"], KW["full"], KW["band"], *KW["q8"])
    ctx.sync()
    bands = _bands(geo, noises, spp, C)
    assert [(a, b) for a, b, _ in bands] == ([(0, 3), (8190, 8200)] if C == 8 else [(0, 2), (4095, 4100)])
    kinds = np.concatenate([w.reshape(-1) for _, _, w in bands])
    assert (kinds & ref.NODATA).any() and (kinds & ref.SATURATED).any() and (kinds == (ref.CANDIDATE if spp == 4 else 0)).any()
    const = _const_byte(spp)
    assert const == (ref.CANDIDATE if spp == 4 else 0)
    br.check_rows(out.cpu().numpy(), bands, const)
    counts = cnt.cpu().numpy()
    assert counts[0] == gw * gh
    assert counts[1] == int((kinds & ref.NODATA != 0).sum()) and counts[2] == int((kinds & ref.SATURATED != 0).sum())
    del src, out
    gc.collect()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("spp,C,rate", [(1, 8, 0.01), (4, 16, 0.002)])
def test_check_rejects_a_wrapped_read(spp, C, rate):
    """the same check on the host at _bigraster.SMALL (64 x 240, offsets wrap at element 192 * 64 + 8): the restatement of the
    whole raster passes; the raster read through a wrapping offset does not"""
    geo = br.SMALL
    noises = _noises(geo, rate)
    x = br.host_raster(geo, noises)
    bands = _bands(geo, noises, spp, C)
    const = _const_byte(spp)
    truth, counts = ref.cells(x, spp, C, **KW)
    wrapped, _ = ref.cells(br.wrapped_read(x, geo.wrap), spp, C, **KW)
    br.check_rows(truth, bands, const)
    assert counts[0] == truth.size
    assert br.rejects(wrapped, bands, const)
    bad = truth.copy()
    bad[-1, -1] ^= 1
    assert br.rejects(bad, bands, const)
