"""GPU: oip_block_moments_u16 and oip_wallis_apply_u16 at addresses past 2^31 samples, where the lines of a real strip live, on the
probe raster of tests/_bigraster.py (32760 x 65600 = 2 149 056 000 samples: one constant on every line but a head and a tail band
of seeded noise).  Moments: 8190 pixels of 4 samples, B 128 (a block is one whole wave); the block lines that touch a band are the
restatement's (_wallis_ref.py), every other block line holds the moments of the constant.  Apply: one sample per pixel, B 32, in
place, node tables that vary across the line only but for the two node lines at either end, which differ from one another:
every constant line out of their reach has the same image, and the lines in their reach -- the bands among them, where a
workgroup walks many rounds of lines and passes from one node line to the next -- are the restatement's.  The tail band's lines
from 65553 on lie wholly past 2^31 samples: a kernel that computed `line * pitch` in
32 bits reads (and writes) the head of the raster for them; the CPU twins at the bottom (not `gpu`) show on _bigraster.SMALL that
the checks reject that."""
import gc

import numpy as np
import pytest

import _bigraster as br
import _wallis_ref as ref

SEED = 61
MOMENTS = (4, 128)                                                      # spp, B
APPLY = (1, 32)


def _noises(geo):
    return [br.band_noise(geo, k, SEED, specials=(0, 65535), rate=0.002) for k in (0, 1)]


def _moment_bands(geo, noises, spp, B):
    """[(first block line, end, moments (3, spp, n, gw))] of the block lines that touch a band, and the planes of a constant line"""
    out = []
    for k, (a, b) in enumerate((geo.head, geo.tail)):
        lo, hi = a // B * B, min(geo.L, -(-b // B) * B)
        out.append((lo // B, -(-hi // B), ref.moments(br.band_input(geo, k, noises[k], lo, hi), spp, B)))
    const = ref.moments(np.full((B, geo.W), br.CONST, np.uint16), spp, B)[:, :, 0]
    return out, const


def _check_moments(acc, bands, const):
    """acc (3, spp, gh, gw): the block lines of the bands equal the restatement, every other one the constant's"""
    pos = 0
    for a, b, want in bands + [(acc.shape[2], acc.shape[2], None)]:
        assert (acc[:, :, pos:a] == const[:, :, None, :]).all(), "a block line in [%d, %d) is not the constant's" % (pos, a)
        if want is not None:
            assert np.array_equal(acc[:, :, a:b], want), "block lines [%d, %d) differ from the restatement" % (a, b)
        pos = b


VARIED = 2                                                              # node lines at either end of the grid that differ from line to line


def _nodes(geo, B, seed=5):
    """node tables that vary across the line only, except in the first and last VARIED node lines, which differ from one another:
    the lines of the two bands are interpolated between different node lines, every constant line far enough from them is not"""
    gw, gh = ref.grid(geo.W, geo.L, B)
    assert gh >= 4 * VARIED
    G, O = ref.mild_nodes(1, gw, 1, seed)
    G, O = np.repeat(G, gh, axis=0), np.repeat(O, gh, axis=0)
    Gv, Ov = ref.mild_nodes(2 * VARIED, gw, 1, seed + 1)
    G[:VARIED], O[:VARIED], G[-VARIED:], O[-VARIED:] = Gv[:VARIED], Ov[:VARIED], Gv[VARIED:], Ov[VARIED:]
    return G, O


def _apply_bands(geo, noises, G, O, B):
    """[(first line, end, want)]: the lines that a varied node line reaches (it reaches B + B / 2 lines past its own) and that hold
    a band; and the image of a constant line everywhere else"""
    gh = G.shape[0]
    reach = (VARIED * B + B, (gh - VARIED) * B - B)                    # lines below / from which a varied node line counts
    assert geo.head[1] <= reach[0] < reach[1] <= geo.tail[0]
    out = []
    for k, (a, b) in enumerate(((0, reach[0]), (reach[1], geo.L))):
        want, _ = ref.apply(br.band_input(geo, k, noises[k], a, b), 1, G, O, B, 1, 65535, 4095, row0=a, L=geo.L)
        out.append((a, b, want))
    mid = gh // 2
    const, _ = ref.apply(np.full((1, geo.W), br.CONST, np.uint16), 1, G[mid:mid + 1], O[mid:mid + 1], B, 1, 65535, 4095, row0=0, L=1)
    return out, const[0]


@pytest.mark.gpu
def test_moments_whole_raster(ctx):
    """peak device memory: 4.3 GB (the raster) + 3 MB (the planes)"""
    import torch
    geo = br.BIG
    f = geo.assert_crosses()
    assert f * geo.W >= br.TWO31 and geo.tail[0] < f < geo.L
    spp, B = MOMENTS
    noises = _noises(geo)
    src = br.device_raster(geo, noises)
    gw, gh = ref.grid(geo.W // spp, geo.L, B)
    acc = torch.full((3 * spp, gh, gw), -1, dtype=torch.int64, device="cuda")
    ctx.block_moments_u16(src, geo.W, geo.W // spp, geo.L, spp, B, acc, gw, gh * gw)
    ctx.sync()
    bands, const = _moment_bands(geo, noises, spp, B)
    assert [(a, b) for a, b, _ in bands] == [(0, 1), (511, 513)]
    _check_moments(acc.cpu().numpy().astype(np.uint64).reshape(3, spp, gh, gw), bands, const)
    del src, acc
    gc.collect()
    torch.cuda.empty_cache()


@pytest.mark.gpu
def test_apply_whole_raster_in_place(ctx):
    """peak device memory: 4.3 GB (the raster, transformed in place) + 17 MB (the node tables)"""
    import torch
    geo = br.BIG
    geo.assert_crosses()
    _, B = APPLY
    noises = _noises(geo)
    G, O = _nodes(geo, B)
    bands, const = _apply_bands(geo, noises, G, O, B)
    assert (const != br.CONST).any()
    src = br.device_raster(geo, noises)
    gh, gw, _ = G.shape
    st = torch.zeros(3, dtype=torch.int64, device="cuda")
    ctx.wallis_apply_u16(src, src, 0, geo.L, geo.W, geo.L, 1, B, torch.from_numpy(G).cuda(), torch.from_numpy(O).cuda(), gw, gh, 1, 65535, 4095, st)
    ctx.sync()
    br.check_rows(src, bands, const)
    specials = sum(int(((n == 0) | (n == 65535)).sum()) for n in noises)
    assert int(st[0]) == geo.W * geo.L - int(sum((n == 0).sum() for n in noises)) and specials > 0
    del src
    gc.collect()
    torch.cuda.empty_cache()


def test_checks_reject_a_wrapped_read():
    """the same checks on the host at _bigraster.SMALL (64 x 240, offsets wrap at element 192 * 64 + 8): the restatement of the
    whole raster passes; the raster read through a wrapping offset does not"""
    geo = br.SMALL
    noises = _noises(geo)
    x = br.host_raster(geo, noises)
    for spp, B in (MOMENTS, (1, 32)):
        bands, const = _moment_bands(geo, noises, spp, B)
        _check_moments(ref.moments(x, spp, B), bands, const)
        with pytest.raises(AssertionError):
            _check_moments(ref.moments(br.wrapped_read(x, geo.wrap), spp, B), bands, const)
    _, B = APPLY
    G, O = _nodes(geo, B)
    bands, const = _apply_bands(geo, noises, G, O, B)
    truth, _ = ref.apply(x, 1, G, O, B, 1, 65535, 4095)
    br.check_rows(truth, bands, const)
    wrapped, _ = ref.apply(br.wrapped_read(x, geo.wrap), 1, G, O, B, 1, 65535, 4095)
    assert br.rejects(wrapped, bands, const)
    bad = truth.copy()
    bad[-1, -1] ^= 1
    assert br.rejects(bad, bands, const)
