"""GPU: oip_pansharpen_sfim_u16 where the product passes 2^31 samples.  The MSS raster is 2048 x 16400, the product 8192 pixels x 4
samples x 65600 lines = 2 149 580 800 samples (4.3 GB): a line is 2^15 samples, so line 65536 begins at sample 2^31 exactly and
lines 65536 .. 65599 lie beyond it.  The pattern is that of tests/_bigraster.py -- every line constant but a head and a tail band
of seeded noise -- and its check_rows compares: the bands with the restatement on windows, every other line with the one row the
constants give.  PAN and MSS have other shapes than the product (a quarter of its samples per line; a quarter of its lines), so
the rasters are built here and not by _bigraster.Probe.

Constants: PAN 1500 and MSS bands 1000, 1500, 2000, 2500.  There Lm = 1500, UL = 12000, g = 0.125 exactly (the limit of
--max-gain 1, which is not a cut) and the product's pixel is the MSS pixel.  A kernel that computed `line * pitch` of the product
in 32 bits would store the tail band's lines over the head band; the CPU twin at the bottom (not `gpu`) shows on a small geometry
that the comparison rejects that."""
import gc

import numpy as np
import pytest

import _bigraster as br
import _pansharpen_ref as ref

SEED = 83
W_MSS, H_MSS = 2048, 16400
MSS_CONST = (1000, 1500, 2000, 2500)
HEAD, TAIL0 = 24, 16376                      # MSS lines [0, 24) and [16376, 16400) carry noise, and the PAN lines under them
HALO = 3                                     # MSS lines: an output line reads MSS lines cell - 2 .. cell + 2
GAIN = 1                                     # --max-gain 1: in the noise about half the gains are cut, so both counters count


def _geo(w, h, head, tail0, wrap=br.TWO31):
    """the product as a _bigraster geometry: 16 w samples per line, 4 h lines, the bands widened by the operator's reach"""
    return br.Geometry(16 * w, 4 * h, 4 * (head + HALO), 4 * (tail0 - HALO), wrap)


def _noise(w, h, head, tail0):
    """per band (0 head, 1 tail): MSS lines (n, w, 4) and PAN lines (4 n, 4 w) of 12-bit noise with zeros among the PAN's, and
    where the band is wide enough a patch of 8 x 10 MSS cells without data (UL == 0 inside it)"""
    out = []
    for k, n in enumerate((head, h - tail0)):
        rng = np.random.default_rng(SEED * 2 + k)
        M = rng.integers(300, 3801, (n, w, 4)).astype(np.uint16)
        P = rng.integers(300, 3801, (4 * n, 4 * w)).astype(np.uint16)
        P[rng.random(P.shape) < 0.02] = 0
        if n >= 12 and w >= 64:
            P[8:40, 96:136] = 0
        out.append((M, P))
    return out


def _host_window(w, h, head, tail0, noise, k, m0, m1):
    """MSS lines [m0, m1) and the PAN lines under them as the host sees them (band k's noise, constants elsewhere)"""
    a, b = (tail0, h) if k else (0, head)
    M = np.empty((m1 - m0, w, 4), np.uint16)
    M[:] = np.array(MSS_CONST, np.uint16)
    P = np.full((4 * (m1 - m0), 4 * w), br.CONST, np.uint16)
    M[a - m0:b - m0] = noise[k][0]
    P[4 * (a - m0):4 * (b - m0)] = noise[k][1]
    return M, P


def _bands(w, h, head, tail0, noise):
    """[(oa, ob, want)] for check_rows: the restatement on each band with 2 HALO constant MSS lines around it, compared on the band
    widened by HALO -- beyond that every line is the constants' -- and the two counters of the whole product"""
    out, zero, cut = [], 0, 0
    for k, (a, b) in enumerate(((0, head), (tail0, h))):
        m0, m1 = max(0, a - 2 * HALO), min(h, b + 2 * HALO)
        oa, ob = 4 * max(0, a - HALO), 4 * min(h, b + HALO)
        M, P = _host_window(w, h, head, tail0, noise, k, m0, m1)
        want, (z, c) = ref.fuse_window(P[oa - 4 * m0:ob - 4 * m0], M, ref.box4(P), oa, h, m0, GAIN)
        out.append((oa, ob, want.reshape(ob - oa, 16 * w)))
        zero, cut = zero + z, cut + c
    return out, (zero, cut)


def _const_row(w):
    """the product's line far from the bands, from the restatement on constants, asked at two places"""
    M = np.empty((9, w, 4), np.uint16)
    M[:] = np.array(MSS_CONST, np.uint16)
    P = np.full((36, 4 * w), br.CONST, np.uint16)
    rows = [ref.fuse_window(P[16:17], M, ref.box4(P), 4 * m + 16, 100 * 1000, m, GAIN)[0].reshape(-1) for m in (500, 507)]
    assert np.array_equal(rows[0], rows[1]) and np.array_equal(rows[0], np.tile(np.array(MSS_CONST, np.uint16), 4 * w))
    return rows[0]


@pytest.mark.gpu
def test_whole_product_and_last_shard(ctx):
    """the whole product in one call, then its last 100 lines again, written where they belong -- 2 146 304 000 samples into the
    product's buffer, the call's own base -- from PAN lines handed over as a small buffer of their own: the same bytes.  Peak
    device memory: 4.3 GB + 1.1 GB + 0.4 GB"""
    import torch
    w, h = W_MSS, H_MSS
    geo = _geo(w, h, HEAD, TAIL0)
    f = geo.assert_crosses()
    assert geo.W * geo.L == 2149580800 and f == 65536 and geo.tail[0] < f
    noise = _noise(w, h, HEAD, TAIL0)
    bands, counts = _bands(w, h, HEAD, TAIL0, noise)
    pan = torch.full((4 * h, 4 * w), br.CONST, dtype=torch.int16, device="cuda").view(torch.uint16)
    mss = torch.from_numpy(np.array(MSS_CONST, np.int16)).cuda().repeat(h * w).view(torch.uint16).view(h, w, 4)
    for (a, b), (M, P) in zip(((0, HEAD), (TAIL0, h)), noise):
        mss[a:b] = torch.from_numpy(M).cuda()
        pan[4 * a:4 * b] = torch.from_numpy(P).cuda()
    low = torch.zeros(h, w, dtype=torch.uint16, device="cuda")
    ctx.decimate_box_u16(pan, 4 * w, 4 * w, 4 * h, 1, 4, low, w)
    out = torch.full((geo.L, geo.W), 0x5A5A, dtype=torch.int16, device="cuda").view(torch.uint16)
    st = torch.zeros(2, dtype=torch.int64, device="cuda")
    ctx.pansharpen_sfim_u16(pan, mss, low, w, h, out, GAIN, st)
    ctx.sync()
    br.check_rows(out, bands, _const_row(w))
    assert tuple(int(v) for v in st.cpu().numpy()) == counts and counts[0] > 1000 and counts[1] > 1000
    o0, n = 65500, 100
    assert o0 * geo.W < br.TWO31 < (o0 + n - 1) * geo.W
    whole = out[o0:].clone()
    out[o0:] = torch.full((n, geo.W), 0x5A5A, dtype=torch.int16, device="cuda").view(torch.uint16)
    shard_pan = pan[o0:].clone()
    ctx.pansharpen_sfim_u16(shard_pan, mss, low, w, h, out[o0:], GAIN, None, out_row0=o0, out_rows=n)
    ctx.sync()
    assert bool((out[o0:].view(torch.int16) == whole.view(torch.int16)).all())
    br.check_rows(out, bands, _const_row(w))                  # ... and nothing else was touched
    del pan, mss, low, out, whole, shard_pan
    gc.collect()
    torch.cuda.empty_cache()


def test_check_rejects_a_wrapped_store():
    """the same comparison on the host at 4 x 60 MSS pixels (the product: 64 samples x 240 lines, store offsets wrapping at sample
    192 * 64 + 8, 47 lines beyond it as in the big one): the restatement passes it, the restatement stored through a wrapping
    offset does not, and neither does the plain up-sampling"""
    w, h, head, tail0 = 4, 60, 3, 43
    geo = _geo(w, h, head, tail0, wrap=192 * 64 + 8)
    geo.assert_crosses()
    noise = _noise(w, h, head, tail0)
    bands, counts = _bands(w, h, head, tail0, noise)
    M = np.empty((h, w, 4), np.uint16)
    M[:] = np.array(MSS_CONST, np.uint16)
    P = np.full((4 * h, 4 * w), br.CONST, np.uint16)
    for (a, b), (Mn, Pn) in zip(((0, head), (tail0, h)), noise):
        M[a:b], P[4 * a:4 * b] = Mn, Pn
    out, got = ref.fuse(P, M, G=GAIN)
    out = out.reshape(4 * h, 16 * w)
    row = _const_row(w)
    br.check_rows(out, bands, row)
    assert got == counts
    assert br.rejects(br.wrapped_store(out, geo.wrap, 0x5A5A), bands, row)
    assert br.rejects(ref.plain(M).reshape(4 * h, 16 * w), bands, row)
