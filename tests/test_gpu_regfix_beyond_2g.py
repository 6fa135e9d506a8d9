"""GPU: oip_warp_grid_bicubic_u16 at addresses past 2^31 samples, on the probe raster of tests/_bigraster.py (BIG: 32760 x 65600
= 2 149 056 000 samples, one constant on every line but a head and a tail band of seeded noise), through its Probe and
check_rows.  The lattice has a node line every 8 lines; the field is random on the node lines inside the two bands (|dx| <= 7 px,
|dy| <= 2 px) and the same on every node line between them, so far from the bands the output is one row vector -- the image of
the constant, which differs from it only where a window leaves the raster at the left or right.  A kernel that computed
`line * pitch` in 32 bits would read the head band for the tail's lines; the CPU twin at the bottom (not `gpu`) shows on
_bigraster.SMALL that the comparison rejects that."""
import gc

import numpy as np
import pytest

import _bigraster as br
import _regfix_ref as ref

SEED = 61
SY = 8
HALO = 12          # the field varies within 8 lines of a band, and a window reaches ceil(|dy|) + 3 = 5 lines further: both inside 12 / 24


def _field(geo, nx):
    """nodes at (i sx, 8 j) covering the raster; NX, NY (ny, nx) int32 Q10"""
    sx = -(-(geo.W - 1) // (nx - 1))
    ny = -(-(geo.L - 1) // SY) + 1
    rng = np.random.default_rng(SEED)
    NX = np.tile(rng.integers(-7168, 7169, (1, nx)), (ny, 1))
    NY = np.tile(rng.integers(-2048, 2049, (1, nx)), (ny, 1))
    for a, b in (geo.head, geo.tail):
        j = np.arange(ny)
        sel = (j * SY >= a) & (j * SY <= b)
        NX[sel] = rng.integers(-7168, 7169, (int(sel.sum()), nx))
        NY[sel] = rng.integers(-2048, 2049, (int(sel.sum()), nx))
    assert (ny - 1) * SY >= geo.L - 1 and (nx - 1) * sx >= geo.W - 1 and np.abs(NX).max() > 6000
    return NX.astype(np.int32), NY.astype(np.int32), sx


def _probe(geo, nx):
    NX, NY, sx = _field(geo, nx)

    def warp(lo, x):
        """the restatement on input lines [lo, lo + lines): the lines out of reach of the window's own edges, zeros elsewhere
        (expected_bands compares the former only)"""
        lines = x.shape[0]
        a = lo if lo == 0 else lo + HALO
        b = lo + lines if lo + lines == geo.L else lo + lines - HALO
        out = np.zeros_like(x)
        out[a - lo:b - lo] = ref.warp(x, NX, NY, 0, 0, sx, SY, row0=lo, L=geo.L, out_row0=a, out_rows=b - a)
        return out
    return br.Probe("warp_grid", geo, [br._inp(geo, SEED, specials=(0, 65535))], HALO, warp, NX=NX, NY=NY, sx=sx)


@pytest.mark.gpu
def test_warp_whole_raster_and_last_shard(ctx, oracle_mod):
    """the whole raster in one call, then lines 65500 .. 65599 again as a shard whose source is a small buffer of the lines
    oip_warp_grid_src_range names: the same bytes.  Peak device memory: 2 x 4.3 GB"""
    import torch
    import opticalimageprocessor_amd as oip
    geo = br.BIG
    f = geo.assert_crosses()
    W, L = geo.W, geo.L
    assert (L - 1) * W >= br.TWO31 and f < geo.tail[1] - HALO
    p = _probe(geo, 9)
    NX, NY, sx = p.extra["NX"], p.extra["NY"], p.extra["sx"]
    bands, row = p.bands(), p.const_row()
    assert (row != br.CONST).any() and (row == br.CONST).sum() > W - 64          # the constant, but for the columns at the two edges
    src = br.device_raster(geo, *p.inputs[0])
    out = torch.full((L, W), 0x5A5A, dtype=torch.int16, device="cuda").view(torch.uint16)
    ctx.warp_grid_bicubic_u16(src, out, W, L, 1, NX, NY, 0, 0, sx, SY)
    ctx.sync()
    br.check_rows(out, bands, row)
    o0, n = 65500, 100
    assert o0 * W < br.TWO31 < (o0 + n - 1) * W
    a, b = oip.warp_grid_src_range(o0, n, L, NY, 0, SY)
    assert 65480 <= a <= o0 - 1 and b == L
    halo = src[a:b].clone()
    part = torch.full((n, W), 0x5A5A, dtype=torch.int16, device="cuda").view(torch.uint16)
    ctx.warp_grid_bicubic_u16(halo, part, W, L, 1, NX, NY, 0, 0, sx, SY, src_row0=a, src_rows=b - a, out_row0=o0, out_rows=n)
    ctx.sync()
    assert bool((part.view(torch.int16) == out[o0:o0 + n].view(torch.int16)).all())
    del src, out, halo, part
    gc.collect()
    torch.cuda.empty_cache()


def test_check_rejects_a_wrapped_read(oracle_mod):
    """the same comparison on the host at _bigraster.SMALL (64 x 240, offsets wrap at element 192 * 64 + 8): the restatement on
    the whole raster passes it, the restatement on the raster read through a wrapping offset does not"""
    geo = br.SMALL
    geo.assert_crosses()
    p = _probe(geo, 8)
    NX, NY, sx = p.extra["NX"], p.extra["NY"], p.extra["sx"]
    bands, row = p.bands(), p.const_row()
    x, = p.host_inputs()
    br.check_rows(ref.warp(x, NX, NY, 0, 0, sx, SY), bands, row)
    y = br.wrapped_read(x, geo.wrap)
    assert br.rejects(ref.warp(y, NX, NY, 0, 0, sx, SY), bands, row)
    # ... and so would a field applied with the wrong sign, or not at all
    assert br.rejects(ref.warp(x, -NX, -NY, 0, 0, sx, SY), bands, row) and br.rejects(x, bands, row)
