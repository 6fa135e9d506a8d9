"""GPU: oip_rescale_u16 at addresses past 2^31 samples, on the probe raster of tests/_bigraster.py (one constant on every line but
a head and a tail band of seeded noise).
Reads: the probe raster (32760 x 65600 = 2 149 056 000 samples) goes to a quarter of its columns (24 taps a row) at unchanged
lines; the band lines are the restatement's (_rescale_ref.py), every constant line gives the constant.  The tail band's lines
from 65553 on lie wholly past 2^31 samples of the SOURCE.
Writes: a raster of 8190 x 16400 built the same way goes x 4 on both axes to 32760 x 65600; the output lines in reach of a band
are the restatement's, every other line holds the constant.  The output lines from 65553 on lie wholly past 2^31 samples of the
OUTPUT, and they are in reach of the tail band.
A kernel that computed `line * samples per line` in 32 bits would read, or write, the head of the raster for those lines; the CPU
twins at the bottom (not `gpu`) show on _bigraster.SMALL that the checks reject that."""
import gc

import numpy as np
import pytest

import _bigraster as br
import _rescale_ref as ref

SEED = 83
FILL = 5000
# the source of the write test and its host model: a quarter of BIG / SMALL on both axes, bands at the head and the tail
BIG_SRC = br.Geometry(8190, 16400, 6, 16380)
SMALL_SRC = br.Geometry(16, 60, 6, 40, wrap=br.SMALL.wrap)


def _noises(geo):
    return [br.band_noise(geo, k, SEED, specials=(0, 65535), rate=0.01) for k in (0, 1)]


class ReadCase:
    """geo.W -> geo.W / 4 columns, lines unchanged"""

    def __init__(self, geo):
        self.geo, self.Wo = geo, geo.W // 4
        self.fx, self.tx = ref.taps("lanczos", geo.W, self.Wo)
        self.fy, self.ty = ref.taps("lanczos", geo.L, geo.L)
        assert self.tx.shape[1] == 24 and self.ty.shape[1] == 6
        self.noises = _noises(geo)

    def restate(self, lo, x):
        n = x.shape[0]
        fy, ty = ref.taps("lanczos", n, n)
        return ref.rescale(x, 1, self.Wo, n, self.fx, self.tx, fy, ty)

    def bands(self):
        return br.expected_bands(self.geo, [(self.noises, br.CONST)], 3, self.restate)


class WriteCase:
    """src.W x src.L -> 4 src.W x 4 src.L"""

    def __init__(self, src, out):
        assert out.W == 4 * src.W and out.L == 4 * src.L
        self.src, self.out = src, out
        self.fx, self.tx = ref.taps("lanczos", src.W, out.W)
        self.fy, self.ty = ref.taps("lanczos", src.L, out.L)
        self.Ky = self.ty.shape[1]
        self.noises = _noises(src)

    def bands(self):
        """[(oa, ob, want)]: the output lines whose rows of taps touch a band, from the source lines those rows read"""
        out = []
        for k, (a, b) in enumerate((self.src.head, self.src.tail)):
            ys = np.nonzero((self.fy + self.Ky - 1 >= a) & (self.fy <= b - 1))[0]
            oa, ob = int(ys[0]), int(ys[-1]) + 1
            s0, sn = ref.src_range(self.src.L, self.out.L, self.Ky, oa, ob - oa)
            win = br.band_input(self.src, k, self.noises[k], s0, s0 + sn)
            out.append((oa, ob, ref.rescale(win, 1, self.out.W, ob - oa, self.fx, self.tx, self.fy[oa:ob] - s0, self.ty[oa:ob])))
        return out


def _device(ctx, case_tables):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in case_tables]


@pytest.mark.gpu
def test_reads_past_2g(ctx):
    """peak device memory: 4.3 GB (the source) + 1.1 GB (the output)"""
    import torch
    geo = br.BIG
    f = geo.assert_crosses()
    assert f * geo.W >= br.TWO31
    c = ReadCase(geo)
    bands = c.bands()
    src = br.device_raster(geo, c.noises)
    out = torch.full((geo.L, c.Wo), FILL, dtype=torch.int16, device="cuda").view(torch.uint16)
    fx, tx, fy, ty = _device(ctx, (c.fx, c.tx, c.fy, c.ty))
    ctx.rescale_u16(src, 0, geo.L, geo.W, geo.L, 1, out, 0, geo.L, c.Wo, geo.L, fx, tx, 24, fy, ty, 6, 0)
    ctx.sync()
    br.check_rows(out, bands, br.CONST)
    del src, out
    gc.collect()
    torch.cuda.empty_cache()


@pytest.mark.gpu
def test_writes_past_2g(ctx):
    """peak device memory: 0.27 GB (the source) + 4.3 GB (the output)"""
    import torch
    geo = br.BIG
    f = geo.assert_crosses()
    c = WriteCase(BIG_SRC, geo)
    bands = c.bands()
    assert bands[1][0] < f < bands[1][1] == geo.L                      # the tail band reaches the lines past 2^31 output samples
    src = br.device_raster(BIG_SRC, c.noises)
    out = torch.full((geo.L, geo.W), FILL, dtype=torch.int16, device="cuda").view(torch.uint16)
    fx, tx, fy, ty = _device(ctx, (c.fx, c.tx, c.fy, c.ty))
    ctx.rescale_u16(src, 0, BIG_SRC.L, BIG_SRC.W, BIG_SRC.L, 1, out, 0, geo.L, geo.W, geo.L, fx, tx, 6, fy, ty, c.Ky, 0)
    ctx.sync()
    br.check_rows(out, bands, br.CONST)
    del src, out
    gc.collect()
    torch.cuda.empty_cache()


def test_checks_reject_a_wrapped_read_and_a_wrapped_store():
    """the same checks on the host at _bigraster.SMALL (64 x 240, offsets wrap at element 192 * 64 + 8): the restatement of the
    whole raster passes; what a wrapping load or store offset would have produced does not"""
    geo = br.SMALL
    geo.assert_crosses()
    c = ReadCase(geo)
    x = br.host_raster(geo, c.noises)
    bands = c.bands()
    truth = ref.rescale(x, 1, c.Wo, geo.L, c.fx, c.tx, c.fy, c.ty)
    br.check_rows(truth, bands, br.CONST)
    assert br.rejects(ref.rescale(br.wrapped_read(x, geo.wrap), 1, c.Wo, geo.L, c.fx, c.tx, c.fy, c.ty), bands, br.CONST)
    bad = truth.copy()
    bad[-1, -1] ^= 1
    assert br.rejects(bad, bands, br.CONST)

    w = WriteCase(SMALL_SRC, geo)
    xs = br.host_raster(SMALL_SRC, w.noises)
    bands = w.bands()
    assert bands[1][0] < geo.first_line_beyond < bands[1][1] == geo.L
    truth = ref.rescale(xs, 1, geo.W, geo.L, w.fx, w.tx, w.fy, w.ty)
    br.check_rows(truth, bands, br.CONST)
    assert br.rejects(br.wrapped_store(truth, geo.wrap, FILL), bands, br.CONST)
    bad = truth.copy()
    bad[100, 7] ^= 1
    assert br.rejects(bad, bands, br.CONST)
