"""GPU: oip_noise_blocks_u16 at addresses past 2^31 samples, where the lines of a real strip live, on the probe raster of
tests/_bigraster.py (32760 x 65600 = 2 149 056 000 samples: one constant on every line but a head and a tail band of seeded
noise), once at spp 1 with B 8 and once as 8190 x 65600 pixels of 4 samples with B 16.  On the constant lines every key is
(1500 >> shift) << 8 (sigma 0); in the lines of blocks that touch the head and the tail band -- whose source lines from 65553
on lie wholly past 2^31 samples -- the keys are the restatement's (_noise_ref.py).  A kernel that computed `line * pitch` in
32 bits reads the head of the raster for the tail band; the CPU twin at the bottom (not `gpu`) shows on _bigraster.SMALL that
the check rejects that."""
import gc

import numpy as np
import pytest

import _bigraster as br
import _noise_ref as ref

SEED = 47
SHIFT = 4


def _noises(geo):
    # 1400 .. 1459 around the constant: real keys of sigma 17 DN (q about 69); 0.2 % zeros: one block in nine holds no data
    return [br.band_noise(geo, k, SEED, lo=1400, hi=1460, specials=(0,), rate=0.002) for k in (0, 1)]


def _bands(geo, noises, spp, B):
    """per channel: [(first key line, end, keys)] of the lines of blocks that touch a band"""
    out = [[] for _ in range(spp)]
    for k, (a, b) in enumerate((geo.head, geo.tail)):
        lo, hi = a // B * B, min(geo.L // B * B, -(-b // B) * B)
        want = ref.keys(br.band_input(geo, k, noises[k], lo, hi), spp, B, SHIFT)
        for c in range(spp):
            out[c].append((lo // B, hi // B, want[c]))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("spp,B", [(1, 8), (4, 16)])
def test_keys_whole_raster(ctx, spp, B):
    """peak device memory: 4.3 GB (the raster) + 67 MB (the keys)"""
    import torch
    geo = br.BIG
    f = geo.assert_crosses()
    assert f * geo.W >= br.TWO31 and geo.tail[0] < f < geo.L                       # read past 2^31: the tail band's lines from f on
    noises = _noises(geo)
    src = br.device_raster(geo, noises)
    nbx, nby = geo.W // spp // B, geo.L // B
    out = torch.full((spp, nby, nbx), 0xABCD - 65536, dtype=torch.int16, device="cuda").view(torch.uint16)
    ctx.noise_blocks_u16(src, geo.W, geo.W // spp, geo.L, spp, B, SHIFT, out, nbx, nby * nbx)
    ctx.sync()
    bands = _bands(geo, noises, spp, B)
    assert [(a, b) for a, b, _ in bands[0]] == ([(0, 3), (8190, 8200)] if B == 8 else [(0, 2), (4095, 4100)])
    for c in range(spp):
        kinds = np.concatenate([w.reshape(-1) for _, _, w in bands[c]])
        assert (kinds == ref.NODATA).any() and ((kinds & 0xFF) < 254).any()
        br.check_rows(out[c], bands[c], (br.CONST >> SHIFT) << 8)
    del src, out
    gc.collect()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("spp,B", [(1, 8), (4, 16)])
def test_check_rejects_a_wrapped_read(spp, B):
    """the same check on the host at _bigraster.SMALL (64 x 240, offsets wrap at element 192 * 64 + 8): the restatement of the
    whole raster passes; the raster read through a wrapping offset does not"""
    geo = br.SMALL
    noises = _noises(geo)
    x = br.host_raster(geo, noises)
    bands = _bands(geo, noises, spp, B)
    truth = ref.keys(x, spp, B, SHIFT)
    wrapped = ref.keys(br.wrapped_read(x, geo.wrap), spp, B, SHIFT)
    for c in range(spp):
        br.check_rows(truth[c], bands[c], (br.CONST >> SHIFT) << 8)
        assert br.rejects(wrapped[c], bands[c], (br.CONST >> SHIFT) << 8)
        bad = truth[c].copy()
        bad[-1, -1] ^= 1
        assert br.rejects(bad, bands[c], (br.CONST >> SHIFT) << 8)
