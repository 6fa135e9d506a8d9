"""GPU: every raster kernel at addresses past 2^31 elements (past byte 2^32), where the lines of a real strip live.

A 30000 x 100000 uint16 strip holds 3.0e9 samples; no other test hands a kernel an offset that a 32-bit register cannot hold.
A kernel that computed `row * pitch` in 32 bits would pass every one of them and corrupt the last third of each product.  Two
ways past the boundary, both with small references (tests/_bigraster.py):

  A. entry points that take a pitch or a plane stride: an image of about 1000 x 40 in lines 2^26 elements apart (rows 32 .. 39
     start at >= 2^31), or planes 2^30 elements apart.  The allocation (torch.empty) is mostly never touched; the existing CPU
     restatement computes all of the image; where the entry point writes, the gaps hold a sentinel that must survive.
  B. entry points whose pitch is the width: the probe raster, 32760 x 65600 = 2 149 056 000 samples (line 65552 straddles
     2^31, lines 65553 .. 65599 lie beyond it) -- one constant on every line but a head and a tail band of seeded noise.  The
     bands, widened by the operation's footprint, must equal the CPU restatement; every other line must equal the image of
     the constant, compared on the device in chunks of 8192 lines.  A load that wraps gives a wrong tail band, a store that
     wraps damages the head band or the constant region (test_bigraster_cpu.py shows both on the host).

Every comparison is equality.  Each test asserts from its shapes which of its addresses lie past 2^31 (a read and a write; for a
reduction, or a case of kind A whose huge pitch is the source's alone, a read), frees what it allocated before it returns, and
states its peak device memory (all under 20 GB)."""
import gc

import numpy as np
import pytest

import _bigraster as br

pytestmark = pytest.mark.gpu

GEO = br.BIG
W, L = GEO.W, GEO.L
TWO31 = br.TWO31
SENT = 0xABCD                     # what destinations hold before a call
P26 = 1 << 26                     # the pitch of kind A: rows 32 .. 39 of 40 start at >= 2^31 elements
ROWS_A = 40
S30 = 1 << 30                     # the plane stride of kind A: planes 2 and 3 start at >= 2^31 elements


def _torch():
    import torch
    return torch


def _cuda(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


def _i16(t):
    return t.view(_torch().int16)


def _empty(n):
    """n uint16 on the device, not touched"""
    torch = _torch()
    return torch.empty(n, dtype=torch.int16, device="cuda").view(torch.uint16)


def _full(shape, value=SENT):
    torch = _torch()
    return torch.full(shape, value - 65536 if value > 32767 else value, dtype=torch.int16, device="cuda").view(torch.uint16)


def _free():
    gc.collect()
    _torch().cuda.empty_cache()


def _rand12(lines, width, seed, lo=16, hi=3900):
    """(lines, width) uint16 of seeded noise made on the device in blocks of 8192 lines (the int32 draw stays at 1 GB)"""
    torch = _torch()
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = _empty(lines * width).view(lines, width)
    for r in range(0, lines, 8192):
        n = min(8192, lines - r)
        _i16(out)[r:r + n] = torch.randint(lo, hi, (n, width), device="cuda", generator=g, dtype=torch.int32).to(torch.int16)
    return out


def _equal(a, b, chunk=8192):
    """torch.equal of two (lines, n) uint16 views, in blocks of lines: no copy of a strided view larger than a block"""
    torch = _torch()
    assert a.shape == b.shape, (a.shape, b.shape)
    return all(torch.equal(_i16(a[r:r + chunk]), _i16(b[r:r + chunk])) for r in range(0, a.shape[0], chunk))


def _holds(flat, value, written, chunk=1 << 28):
    """every element of the flat uint16 buffer outside the [a, b) ranges of `written` still holds `value`"""
    v = value - 65536 if value > 32767 else value
    pos = 0
    for a, b in sorted(written) + [(flat.numel(), flat.numel())]:
        assert pos <= a
        for c in range(pos, a, chunk):
            if bool((_i16(flat[c:min(a, c + chunk)]) != v).any()):
                return False
        pos = b
    return True


def _kernels(ctx, call):
    """run `call` with the context's profiler on -> the names its launches were profiled under"""
    ctx.sync()
    ctx.profile_enable(True)
    try:
        ctx.profile_reset()
        call()
        ctx.sync()
        return set(ctx.profile())
    finally:
        ctx.profile_reset()
        ctx.profile_enable(False)


def _past(*offsets):
    """the test's own proof that it is where it claims to be: each element offset is >= 2^31"""
    for o in offsets:
        assert o >= TWO31, o


@pytest.fixture(scope="module")
def probes(oracle_mod):
    GEO.assert_crosses()
    return br.probes(GEO, oracle_mod, folds=(100, 99))


def _rasters(p):
    return [br.device_raster(GEO, noises, c) for noises, c in p.inputs]


# =============================================================================================================== kind B
def test_rrc_whole_raster(ctx, probes):
    """oip_rrc_u16 with a LUT that differs per column: out of place into a sentinel, in place, and in place through a view
    that starts 8 elements into its allocation (the line-aligned kernel), whose neighbours must stay.
    Peak: src + dst + the offset copy = 3 x 4.3 GB = 12.9 GB."""
    p = probes["rrc"]
    bands, row = p.bands(), p.const_row()
    _past((L - 1) * W)                                             # last line: read and written there
    d_kb = ctx.upload_kb(p.extra["kb"])
    src, = _rasters(p)
    dst = _full((L, W))
    ctx.rrc_u16(src, dst, W, L, d_kb); ctx.sync()
    br.check_rows(dst, bands, row)
    del dst
    base = _full((L * W + 4096,))
    view = base[8:8 + L * W]
    view.view(L, W).copy_(src)
    ctx.rrc_u16(src, src, W, L, d_kb)
    ctx.rrc_u16(view, view, W, L, d_kb); ctx.sync()
    br.check_rows(src, bands, row)
    br.check_rows(view.view(L, W), bands, row)
    assert _holds(base, SENT, [(8, 8 + L * W)])
    del src, base, view
    _free()


def test_rrc_narrow_raster_grid_cap(ctx, oracle_mod):
    """oip_rrc_u16 on 64 x 33 554 480: as many samples, in half a million times as many lines.  The flat kernel's launch then
    has more line groups than 65535 x 16 and takes the branch that caps grid.y and recomputes the groups per block, which no
    other shape in the suite reaches; lines from 2^25 on start past 2^31.  Peak: 2 x 4.3 GB."""
    geo = br.Geometry(64, (1 << 25) + 48, 24, (1 << 25) - 32)
    assert geo.assert_crosses() == 1 << 25
    assert geo.L // 8 > 65535 * 16                                  # 8 lines of 8 chunks make a group of 64 chunks
    _past((geo.L - 1) * geo.W)
    kb = br.lut(geo.W, 64)
    noises = [br.band_noise(geo, k, 64, specials=(0, 65535, 4095)) for k in (0, 1)]
    bands = [(a, b, oracle_mod.rrc(n, kb)) for (a, b), n in zip((geo.head, geo.tail), noises)]
    row = oracle_mod.rrc(np.full((1, geo.W), br.CONST, np.uint16), kb)[0]
    src = br.device_raster(geo, noises)
    dst = _full((geo.L, geo.W))
    ctx.rrc_u16(src, dst, geo.W, geo.L, ctx.upload_kb(kb)); ctx.sync()
    br.check_rows(dst, bands, row, chunk=1 << 22)
    del src, dst
    _free()


def test_mss_split_rrc_whole_raster(ctx, probes):
    """oip_mss_split_rrc_u16 of a 4 x 8190 BIL line: band b is columns [8190 b, 8190 (b + 1)) through its own LUT, so the four
    planes side by side are the RRC of the raster under the band-major LUT.  Plane 3's lines from 65409 on are written past
    2^31.  Peak: 2 x 4.3 GB."""
    p = probes["mss_split_rrc"]
    bands, row = p.bands(), p.const_row()
    bw = W // 4
    _past((L - 1) * W, 3 * L * bw + (L - 1) * bw)
    bil, = _rasters(p)
    planes = _full((4, L, bw))
    ctx.mss_split_rrc_u16(bil, planes, L * bw, W, L, ctx.upload_kb(p.extra["kb"])); ctx.sync()
    for b in range(4):
        cols = slice(b * bw, (b + 1) * bw)
        br.check_rows(planes[b], [(a, e, w[:, cols]) for a, e, w in bands], row[cols])
    del bil, planes
    _free()


@pytest.mark.parametrize("fold", [100, 99])
def test_stitch_rows_whole_raster(ctx, probes, fold):
    """oip_stitch_rows_u16: fold 100 (output line 65320, the vector kernel) and fold 99 (65322: the scalar kernel); the two
    inputs differ in their constant and in their noise.  Peak: 2 x 4.3 + 8.6 = 17.2 GB."""
    p = probes["stitch_rows_f%d" % fold]
    Wo = 2 * (W - fold)
    _past((L - 1) * W, (L - 1) * Wo)
    left, right = _rasters(p)
    out = _full((L, Wo))
    ctx.stitch_rows_u16(left, right, out, W, L, fold); ctx.sync()
    br.check_rows(out, p.bands(), p.const_row())
    del left, right, out
    _free()


def test_permute_whole_raster(ctx, probes):
    """oip_permute_u16x4 in place on 8190 x 65600 pixels of 4 samples (a flat index).  Peak: 4.3 GB."""
    p = probes["permute"]
    _past((L - 1) * W)
    img, = _rasters(p)
    ctx.permute_u16x4(img, L * W // 4, p.extra["order"]); ctx.sync()
    br.check_rows(img, p.bands(), p.const_row())
    del img
    _free()


def test_merge_subimages_whole_raster(ctx):
    """oip_merge_subimages_be16 with 8 x 5 tiles of 8200 x 6552: 8 * 5 * 8200 * 6552 = W * L samples.  The tiles are made on the
    device from the probe raster (cut, byte-swapped), so the output must be the probe raster itself.  The last tile's lines from
    8168 on are read past 2^31, output lines from 65553 on are written there.  Peak while the tiles are made: raster + cut + swapped = 12.9 GB."""
    torch = _torch()
    vp, hp, sl, sc = 8, 5, 8200, 6552
    assert vp * sl == L and hp * sc == W
    _past((L - 1) * W, (vp * hp * sl - 1) * sc)                     # the last line of the last tile / of the output
    noises = [br.band_noise(GEO, k, 50) for k in (0, 1)]
    x = br.device_raster(GEO, noises)
    cut = _i16(x).view(vp, sl, hp, sc).permute(0, 2, 1, 3).contiguous()
    del x
    tiles = cut.view(torch.uint8).view(-1, 2).flip(1).contiguous().view(torch.int16)
    del cut
    out = _full((L, W))
    ctx.merge_subimages_be16(tiles, out, vp, hp, sl, sc); ctx.sync()
    br.check_rows(out, [(GEO.head[0], GEO.head[1], noises[0]), (GEO.tail[0], GEO.tail[1], noises[1])], br.CONST)
    del tiles, out
    _free()


@pytest.mark.parametrize("spp", [1, 4])
def test_seam_moments_whole_raster(ctx, spp):
    """oip_seam_moments_u16 and oip_seam_moments_blocks_u16 (blocks of 40 lines: the last one, 65560 .. 65599, lies past 2^31)
    with valid range 1 .. 65534 against br.expected_block_moments: _seam_ref.moments on the lines of the bands plus the closed
    form for the constant lines -- the left raster's constant is 1500, the right one's 1700 (test_bigraster_cpu.py holds that
    expectation to _seam_lines_ref.block_moments and shows that a wrapped read misses it).  A reduction: only reads cross.
    Peak: 2 x 4.3 GB."""
    torch = _torch()
    fold, B = 100 // spp, 40
    nb = L // B
    assert (nb - 1) * B >= GEO.first_line_beyond
    _past((nb - 1) * B * W, (L - 1) * W)
    ins = br.seam_inputs(GEO, spp)
    want = br.expected_block_moments(GEO, ins, fold, spp, B, 1, 65534)
    left, right = (br.device_raster(GEO, n, c) for n, c in ins)
    acc = torch.zeros(6, spp, dtype=torch.int64, device="cuda")
    accb = torch.zeros(nb, 6, spp, dtype=torch.int64, device="cuda")
    ctx.seam_moments_u16(left, right, W, L, fold * spp, spp, acc, 1, 65534)
    ctx.seam_moments_blocks_u16(left, right, W, L, fold * spp, spp, B, accb, 1, 65534); ctx.sync()
    assert np.array_equal(accb.cpu().numpy().view(np.uint64), want)
    assert np.array_equal(acc.cpu().numpy().view(np.uint64), want.sum(0, dtype=np.uint64))
    del left, right
    _free()


@pytest.mark.parametrize("lines", [False, True])
@pytest.mark.parametrize("spp,h,tag", [(1, 16, ""), (4, 0, ""), (1, 0, ""), (4, 16, ""), (1, 16, "_scalar")])
def test_stitch_balanced_whole_raster(ctx, probes, spp, h, tag, lines):
    """oip_stitch_balanced_u16 and, with a (G, O) per line in tables of 65600 entries (their own pair on every line of the
    bands), oip_stitch_balanced_lines_u16.  fs = 100 samples, output line 65320: the vector form; "_scalar": fs = 99, output
    line 65322, not a multiple of 8: the per-sample form of either.
    Peak: 2 x 4.3 + 8.6 = 17.2 GB."""
    p = probes["stitch_balanced_%sspp%d_h%d%s" % ("lines_" if lines else "", spp, h, tag)]
    e = p.extra
    Wo = 2 * (W - e["fold"] * spp)
    assert (Wo % 8 != 0) == bool(tag)
    _past((L - 1) * W, (L - 1) * Wo)
    left, right = _rasters(p)
    out = _full((L, Wo))
    if lines:
        assert e["LG"].shape == (L, spp)
        ctx.stitch_balanced_lines_u16(left, right, out, W, L, e["fold"] * spp, spp, _cuda(e["LG"]), _cuda(e["LO"]), h, 1)
    else:
        ctx.stitch_balanced_u16(left, right, out, W, L, e["fold"] * spp, spp, _cuda(e["G"]), _cuda(e["O"]), h, 1)
    ctx.sync()
    br.check_rows(out, p.bands(), p.const_row())
    del left, right, out
    _free()


@pytest.mark.parametrize("k,spp", [(9, 1), (3, 1), (9, 4), (3, 4)])
def test_convolve_whole_raster_and_last_shard(ctx, probes, k, spp):
    """oip_convolve_u16, and its lines 65500 .. 65599 again as a shard whose source (the halo included) is a small buffer of its
    own: the same bytes as the whole call.  Peak: 2 x 4.3 GB."""
    p = probes["convolve_%dx%d_spp%d" % (k, k, spp)]
    taps = p.extra["taps"]
    _past((L - 1) * W)
    src, = _rasters(p)
    out = _full((L, W))
    ctx.convolve_u16(src, out, W // spp, L, spp, taps, 1); ctx.sync()
    br.check_rows(out, p.bands(), p.const_row())
    o0, n, s0 = 65500, 100, 65500 - k // 2
    assert o0 * W < TWO31 < (o0 + n - 1) * W
    halo = src[s0:].clone()
    part = _full((n, W))
    ctx.convolve_u16(halo, part, W // spp, L, spp, taps, 1, src_row0=s0, src_rows=L - s0, out_row0=o0, out_rows=n); ctx.sync()
    assert _equal(part, out[o0:o0 + n])
    del src, out, halo, part
    _free()


@pytest.mark.parametrize("spp", [1, 4])
def test_despike_whole_raster(ctx, probes, spp):
    """oip_despike_u16: spp 1 with a column table and four groups, spp 4 without; the noise carries impulses, no data and
    65535.  The replacements counted per column are those of the two bands (a constant line replaces nothing).  Then the last
    lines as a shard, as for the convolution.  Peak: 2 x 4.3 GB."""
    torch = _torch()
    p = probes["despike_spp%d" % spp]
    e = p.extra
    _past((L - 1) * W)
    want_cnt = np.zeros(W, np.uint64)
    for k, (lo, hi, _, _) in enumerate(br.band_windows(GEO, p.halo)):
        want_cnt += e["counts"](br.band_input(GEO, k, p.inputs[0][0][k], lo, hi, p.inputs[0][1]))
    assert want_cnt.sum() > 1000
    src, = _rasters(p)
    out = _full((L, W))
    cnt = torch.zeros(W, dtype=torch.int64, device="cuda")
    tab = _cuda(e["coltab"]) if e["coltab"] is not None else None
    ctx.despike_u16(src, out, W // spp, L, spp, *e["thr"], e["groups"], tab, cnt); ctx.sync()
    br.check_rows(out, p.bands(), p.const_row())
    assert np.array_equal(cnt.cpu().numpy().view(np.uint64), want_cnt)
    # lines 65500 .. 65599 again as a shard whose source, one halo line included, is a small buffer: the bytes of the whole call
    o0, n, s0 = 65500, 100, 65499
    assert o0 * W < TWO31 < (o0 + n - 1) * W
    halo = src[s0:].clone()
    part = _full((n, W))
    ctx.despike_u16(halo, part, W // spp, L, spp, *e["thr"], e["groups"], tab, None, src_row0=s0, src_rows=L - s0, out_row0=o0, out_rows=n)
    ctx.sync()
    assert _equal(part, out[o0:o0 + n])
    del src, out, halo, part
    _free()


# ---- resampling -----------------------------------------------------------------------------------------------------------
# multiples of 1/128: x + dx and y + dy are exact in fp32 for every column below 32768, so a slab's own column index gives the
# phases of the whole image (test_bigraster_cpu.py shows the slab argument on the oracle)
SHIFTS = [(3.3828125, -1.6171875), (-2.2578125, 2.3984375)]


@pytest.mark.parametrize("dx,dy", SHIFTS)
def test_remap_shift_whole_raster_on_slabs_and_last_shard(ctx, oracle_mod, dx, dy):
    """oip_remap_shift_bicubic_u16 on random 12-bit data with the default sections (30000 lines: the third one starts at about
    line 60000 and ends past 2^31) against oracle.prestitch on three 96-column slabs over all 65600 lines, exact on the columns
    whose taps stay inside the slab and through the image's own edges; then lines 65500 .. 65599 as a shard from a small source
    buffer: the bytes of the whole call.  Peak: 2 x 4.3 + the halo (2.0 GB at dy > 0) = 10.6 GB."""
    import opticalimageprocessor_amd as oip
    _past((L - 1) * W)
    src = _rand12(L, W, 101)
    _i16(src)[::97] = -1                                            # saturated lines: the clamp at bicubic overshoot
    dst = _full((L, W))
    ctx.remap_shift_bicubic_u16(src, dst, W, L, dx, dy); ctx.sync()
    for c0, c1 in br.slabs(W):
        a, b = br.slab_columns(c0, c1, W, dx)
        want, _ = oracle_mod.prestitch(src[:, c0:c1].cpu().numpy(), dx, dy)
        got = dst[:, a:b].cpu().numpy()
        assert np.count_nonzero(want[GEO.first_line_beyond:L - 8]) > 0
        assert np.array_equal(got, want[:, a - c0:b - c0]), (c0, c1, np.argwhere(got != want[:, a - c0:b - c0])[:4])
    o0, n = 65500, 100
    f, l = oip.remap_shift_src_range(o0, n, L, dy)
    assert 0 <= f < l <= L          # dy > 0: the short last section reads the stale tail of the section before it, 30000 lines
    halo = src[f:l].clone()
    part = _full((n, W))
    ctx.remap_shift_bicubic_u16(halo, part, W, L, dx, dy, src_row0=f, src_rows=l - f, out_row0=o0, out_rows=n); ctx.sync()
    assert _equal(part, dst[o0:o0 + n])
    del src, dst, halo, part
    _free()


@pytest.mark.parametrize("f16", [False, True])
def test_remap_window_forms_whole_raster(ctx, f16):
    """oip_remap_shift_bicubic_u16_window, oip_remap_shift_rrc_bicubic_u16_window and the fp16-accumulate form of both against
    the chain of test_remap_window_equals_remap_then_stitch: oip_rrc_u16, then the plain call (fp32 above: exact against the
    oracle; the f16 form has no oracle and is compared with its own plain call).  The stitch step of that chain is a copy of
    columns >= fold to another pitch; here the comparison does it: the window is columns >= 104 written from column 112 on into
    a raster of pitch W + 8, compared with those columns of the plain result.  Four rasters fit that way: a destination of pitch
    2 (W - fold) next to its stitched reference would take 21.5 GB.  What the window leaves out must keep the sentinel.
    Peak: 4 x 4.3 = 17.2 GB."""
    dx, dy = SHIFTS[0]
    c0, off, P = 104, 112, W + 8
    n = W - c0
    assert off + n == P and P != W
    _past((L - 1) * W, (L - 1) * P + off)
    rng = np.random.default_rng(5)
    kb = np.stack([1.0 + rng.integers(-3, 4, W) / 64.0, rng.integers(-8, 9, W) / 4.0], 1)     # 12-bit data stays 12-bit data
    d_kb = ctx.upload_kb(kb)
    raw = _rand12(L, W, 102)
    corrected = _full((L, W))
    ctx.rrc_u16(raw, corrected, W, L, d_kb)
    plain = _full((L, W))
    ctx.remap_shift_bicubic_u16(corrected, plain, W, L, dx, dy, f16acc=f16)
    got = _full((L, P))
    ctx.remap_shift_bicubic_u16_window(corrected, got, P, c0, off, W, L, dx, dy, f16acc=f16); ctx.sync()
    assert not _equal(corrected[:64], raw[:64])
    assert _equal(got[:, off:], plain[:, c0:])
    assert not bool((_i16(got[:, :off]) != SENT - 65536).any())
    del corrected
    _i16(got).fill_(SENT - 65536)
    ctx.remap_shift_rrc_bicubic_u16_window(raw, d_kb, got, P, c0, off, W, L, dx, dy, f16acc=f16); ctx.sync()
    assert _equal(got[:, off:], plain[:, c0:])
    assert not bool((_i16(got[:, :off]) != SENT - 65536).any())
    del raw, plain, got
    _free()


# ---- correlation ----------------------------------------------------------------------------------------------------------
def test_stt_correlate_sections_past_2g(ctx):
    """oip_stt_correlate on two 32760 x 100000 rasters, five sections of the product's 16000 lines x 200 columns.  The rule of
    oip_c.h / stitcher.h:151-167: gap = (L - sections * lps) / (sections + 1), section s starts at gap + s (gap + lps).  Section 4
    starts at line 80665, 2.6e9 elements in; section 3 ends past 2^31.  Only the windows are filled (noise, every section its
    own).  Each such section must equal, to the bit, the call on a contiguous copy of its lines.  Peak: 2 x 6.6 GB = 13.1 GB."""
    Ls, S, lps, ov, edge = 100000, 5, 16000, 200, 4
    gap = (Ls - S * lps) // (S + 1)
    start = [gap + s * (gap + lps) for s in range(S)]
    past = [s for s in range(S) if start[s] * W >= TWO31]
    assert past == [4] and (start[3] + lps) * W > TWO31 and start[4] + lps <= Ls
    _past(start[4] * W + W - ov)
    p1, p2 = _empty(Ls * W).view(Ls, W), _empty(Ls * W).view(Ls, W)
    for s in range(S):
        p1[start[s]:start[s] + lps, W - ov:] = _rand12(lps, ov, 200 + s, 64, 4096)
        p2[start[s]:start[s] + lps, :ov] = _rand12(lps, ov, 300 + s, 64, 4096)
    whole = ctx.stt_correlate(p1, p2, W, Ls, 0, Ls, S, lps, ov, edge)
    assert np.isfinite(whole).all()
    for s in (3, 4):
        a = p1[start[s]:start[s] + lps].clone()
        b = p2[start[s]:start[s] + lps].clone()
        alone = ctx.stt_correlate(a, b, W, lps, 0, lps, 1, lps, ov, edge)
        assert np.array_equal(alone[0], whole[s]), (s, alone[0], whole[s])
        del a, b
    assert not np.array_equal(whole[4], whole[0])                  # the sections do differ: a wrapped window would show
    del p1, p2
    _free()


def test_interband_correlate_sections_past_2g(ctx):
    """oip_interband_correlate at the production geometry, which is what takes the production plan route (16000 x 3000 windows:
    W = 30000 in 10 slices -- 32760 has no slice count that gives 3000 columns): Lp = 100000, five sections.  preproc.h:245-257:
    gap = (Lp - sections * corr) / (sections + 1), section s starts at gap + s (corr + gap); the bands at a quarter of it.
    Section 4 starts at line 80665 = 2.4e9 elements; the band planes are small and 2^30 elements apart, so bands 2 and 3 are read
    past 2^31 in every section.  Section 4 must equal, to the bit, the call on contiguous copies of its PAN and band lines.
    Peak: PAN 6.0 + planes 6.8 + copies 1.2 + transforms = about 15 GB."""
    torch = _torch()
    Wp, Lp, S, corr, slices = 30000, 100000, 5, 16000, 10
    Wb, Lm, brows = Wp // 4, Lp // 4, corr // 4
    gap = (Lp - S * corr) // (S + 1)
    start = [gap + s * (corr + gap) for s in range(S)]
    bstart = [gap // 4 + s * (brows + gap // 4) for s in range(S)]
    assert start[4] * Wp >= TWO31 and start[3] * Wp < TWO31 and start[4] + corr <= Lp and bstart[4] + brows <= Lm
    _past(start[4] * Wp, 2 * S30)
    pan = _empty(Lp * Wp).view(Lp, Wp)
    planes = _empty(3 * S30 + Lm * Wb)
    band = [planes[b * S30:b * S30 + Lm * Wb].view(Lm, Wb) for b in range(4)]
    for s in range(S):
        pan[start[s]:start[s] + corr] = _rand12(corr, Wp, 400 + s, 64, 4096)
        for b in range(4):
            band[b][bstart[s]:bstart[s] + brows] = _rand12(brows, Wb, 500 + 4 * s + b, 64, 4096)
    whole = ctx.interband_correlate(pan, Lp, 0, Lp, planes, S30, 0, Lm, Wp, slices, S, corr)
    assert np.isfinite(whole[..., :3]).all()
    s = 4
    pc = pan[start[s]:start[s] + corr].clone()
    bc = torch.stack([_i16(band[b][bstart[s]:bstart[s] + brows]) for b in range(4)])
    alone = ctx.interband_correlate(pc, corr, 0, corr, bc, brows * Wb, 0, brows, Wp, slices, 1, corr)
    assert np.array_equal(alone[:, :, :3], whole[:, s * slices:(s + 1) * slices, :3])
    assert not np.array_equal(whole[:, :slices, :3], whole[:, s * slices:(s + 1) * slices, :3])
    del pan, planes, band, pc, bc
    _free()


# ---- LZW ------------------------------------------------------------------------------------------------------------------
def _predict(block, spp):
    d = block.astype(np.uint16).copy()
    d[:, spp:] = (block[:, spp:].astype(np.int32) - block[:, :-spp].astype(np.int32)).astype(np.uint16)
    return d.astype("<u2").tobytes()


def test_lzw_strips_of_the_probe_raster(ctx):
    """oip_tiff_lzw_strips_u16 / oip_tiff_lzw_decode_u16: width 8190, 4 samples, one row per strip: 65600 strips whose input
    index passes 2^31.  The strips of the first line, of line 65552 (it straddles 2^31), of the first line wholly beyond and of
    the last line (br.lzw_lines) against _tiff.lzw_encode byte for byte; the whole payload decoded on the device is the image.
    Peak: image 4.3 + payload buffer 6.5 (oip_tiff_lzw_worst_bytes: 65600 strips of 1.5 x 65520 + 129 bytes) + decoded 4.3 +
    the coder's scratch (under 0.1) = 15.2 GB."""
    import _tiff
    torch = _torch()
    width, spp = W // 4, 4
    _past((L - 1) * W)
    noises = [br.band_noise(GEO, k, 90) for k in (0, 1)]
    img = br.device_raster(GEO, noises)
    cap = ctx.tiff_lzw_worst_bytes(L, width, spp, 1)
    assert cap == L * (65520 * 3 // 2 + 65520 // 1024 + 66) and 2 * (2 * L * W) + cap < 15.1e9
    pay = torch.empty(cap, dtype=torch.uint8, device="cuda")
    off, ln, total = ctx.tiff_lzw_strips(_i16(img), L, width, spp, 1, pay)
    assert len(off) == L and off[0] == 0 and total == off[-1] + ln[-1] and total <= cap
    assert (off % 2 == 0).all() and (off[1:] >= off[:-1] + ln[:-1]).all() and (off[1:] <= off[:-1] + ln[:-1] + 1).all()
    assert br.lzw_lines(GEO) == (0, 65552, 65553, L - 1)
    for r in br.lzw_lines(GEO):
        a = GEO.tail[0] if r >= GEO.tail[0] else 0
        line = (noises[1] if r >= GEO.tail[0] else noises[0])[r - a:r - a + 1]
        got = pay[int(off[r]):int(off[r] + ln[r])].cpu().numpy().tobytes()
        assert got == _tiff.lzw_encode(_predict(line, spp)), r
    const = _tiff.lzw_encode(_predict(np.full((1, W), br.CONST, np.uint16), spp))
    assert pay[int(off[30000]):int(off[30000] + ln[30000])].cpu().numpy().tobytes() == const
    back = _full((L, W))
    ctx.tiff_lzw_decode(pay, off, ln, L, width, spp, 1, 2, _i16(back))
    assert _equal(back, img)
    del img, pay, back
    _free()


def test_lzw_payload_past_4g_bytes(ctx):
    """the same geometry filled with 16-bit noise, which LZW cannot compress: 5.5 GB of payload, so the offsets of the strips
    from about line 51000 on -- and what the pack kernel writes and the decoder reads there -- lie past byte 2^32.  The last
    line's strip against _tiff.lzw_encode, the payload decoded on the device against the image.  Measured on the MI355X:
    encode 0.29 s, decode 0.30 s.  Peak: image 4.3 + payload buffer 6.5 + decoded 4.3 + scratch (under 0.1) = 15.2 GB."""
    import _tiff
    torch = _torch()
    width, spp = W // 4, 4
    img = _rand12(L, W, 104, -32768, 32768)
    pay = torch.empty(ctx.tiff_lzw_worst_bytes(L, width, spp, 1), dtype=torch.uint8, device="cuda")
    off, ln, total = ctx.tiff_lzw_strips(_i16(img), L, width, spp, 1, pay)
    assert len(off) == L and total == off[-1] + ln[-1] and total <= pay.numel()
    _past(int(off[-1]) // 2)                                        # byte offset >= 2^32
    assert int(off[GEO.first_line_beyond]) >= 1 << 32
    r = L - 1
    got = pay[int(off[r]):int(off[r] + ln[r])].cpu().numpy().tobytes()
    assert got == _tiff.lzw_encode(_predict(img[r:r + 1].cpu().numpy(), spp))
    back = _full((L, W))
    ctx.tiff_lzw_decode(pay, off, ln, L, width, spp, 1, 2, _i16(back))
    assert _equal(back, img)
    del img, pay, back
    _free()


# =============================================================================================================== kind A
def _image_a(w, seed, lo=0, hi=65536):
    return np.random.default_rng(0xA + seed).integers(lo, hi, (ROWS_A, w), dtype=np.uint16)


def _pitched(img, pitch=P26, offset=0, buf=None):
    """the image in lines `pitch` elements apart, the first at element `offset` of an untouched allocation"""
    rows, w = img.shape
    if buf is None:
        buf = _empty((rows - 1) * pitch + offset + w + 4096)
    d = _cuda(img)
    for r in range(rows):
        buf[offset + r * pitch:offset + r * pitch + w] = d[r]
    return buf


@pytest.mark.parametrize("w,soff,doff", [(1000, 0, 0), (1003, 0, 0), (1003, 1, 3), (1000, 0, 8)])
def test_rrc_window_huge_pitches(ctx, oracle_mod, w, soff, doff):
    """oip_rrc_u16_window with src_pitch 2^26, then with dst_pitch 2^26 as well, into a buffer full of a sentinel that must
    survive between the lines.  The wrapper takes rrc_u16_window_kernel when both pitches are multiples of 8, both bases 16-byte
    aligned and the last 8-column group fits the source line: (1000, 0, 0), (1003, 0, 0) -- a partial last group -- and
    (1000, 0, 8), a destination 16 bytes into its buffer.  A source 1 and a destination 3 elements off alignment take
    rrc_u16_window_scalar_kernel.  Peak: 5.2 GB + 5.2 GB."""
    img = _image_a(w, w + soff)
    kb = br.lut(w, w)
    want = oracle_mod.rrc(img, kb)
    d_kb = ctx.upload_kb(kb)
    _past((ROWS_A - 1) * P26)
    src = _pitched(img, offset=soff)
    vector = (src.data_ptr() + 2 * soff) % 16 == 0 and doff % 8 == 0
    assert vector == (soff == 0)
    small = _full((ROWS_A * 1024 + 64,))
    ctx.rrc_u16_window(src[soff:], P26, small[doff:], 1024, w, ROWS_A, d_kb); ctx.sync()
    canvas = np.full(ROWS_A * 1024 + 64, SENT, np.uint16)
    for r in range(ROWS_A):
        canvas[doff + r * 1024:doff + r * 1024 + w] = want[r]
    assert np.array_equal(small.cpu().numpy(), canvas)
    big = _full(((ROWS_A - 1) * P26 + 1024 + 64,))
    assert big.data_ptr() % 16 == 0
    ctx.rrc_u16_window(src[soff:], P26, big[doff:], P26, w, ROWS_A, d_kb); ctx.sync()
    rows = np.stack([big[doff + r * P26:doff + r * P26 + w].cpu().numpy() for r in range(ROWS_A)])
    assert np.array_equal(rows, want)
    assert _holds(big, SENT, [(doff + r * P26, doff + r * P26 + w) for r in range(ROWS_A)])
    del src, big
    _free()


@pytest.mark.parametrize("w,offset,kernel", [(1000, 0, "colstats_u16_kernel"), (1003, 0, "colstats_u16_kernel"),
                                             (1003, 2, "colstats_u16_column_kernel"), (1000, 1, "colstats_u16_column_kernel")])
def test_colstats_huge_pitch(ctx, w, offset, kernel):
    """oip_colstats_u16 with pitch 2^26.  The wrapper chooses by pitch and alignment, not by width: a 16-byte aligned window takes
    colstats_u16_kernel (w 1000, and 1003 with a partial last group), a window 2 or 1 elements off takes
    colstats_u16_column_kernel; the profiler says which one ran.  Peak: 5.2 GB."""
    import _colstats_ref
    torch = _torch()
    img = _image_a(w, 10 + w + offset)
    _past((ROWS_A - 1) * P26)
    src = _pitched(img, offset=offset)
    assert src.data_ptr() % 16 == 0
    acc = torch.zeros(3, w, dtype=torch.int64, device="cuda")
    ran = _kernels(ctx, lambda: ctx.colstats_u16(src.data_ptr() + 2 * offset, P26, w, ROWS_A, acc, 64, 65000))
    assert ran == {kernel}, ran
    assert np.array_equal(acc.cpu().numpy().view(np.uint64), _colstats_ref.totals(img, 64, 65000))
    del src
    _free()


@pytest.mark.parametrize("offset", [0, 2])
@pytest.mark.parametrize("F", [2, 64])
@pytest.mark.parametrize("spp", [1, 4])
def test_decimate_huge_pitch_and_plane_stride(ctx, spp, F, offset):
    """oip_decimate_box_u16 with pitch 2^26: a 16-byte aligned source (vector kernel) and one offset by 2 elements (block
    kernel); at spp 4 also with the output planes 2^30 elements apart (planes 2 and 3 are written past 2^31) in a buffer whose
    sentinel must survive around them.  Peak: 5.2 + 6.4 GB."""
    import _quicklook_ref
    w = 1000 // spp
    img = _image_a(1000, 20 + spp + F)
    want = _quicklook_ref.decimate(img.reshape(ROWS_A, w, spp) if spp == 4 else img, F)
    want = want.reshape(spp, -(-ROWS_A // F), -(-w // F))
    oh, ow = want.shape[1:]
    _past((ROWS_A - 1) * P26)
    src = _pitched(img, offset=offset)
    out = _full((spp, oh, ow))
    ran = _kernels(ctx, lambda: ctx.decimate_box_u16(src.data_ptr() + 2 * offset, P26, w, ROWS_A, spp, F, out, ow, oh * ow))
    assert ran == {"decimate_box_u16_block_kernel" if offset else "decimate_box_u16_kernel"}, ran
    assert np.array_equal(out.cpu().numpy(), want)
    if spp == 4:
        _past(2 * S30)
        far = _full((3 * S30 + oh * ow + 64,))
        ctx.decimate_box_u16(src.data_ptr() + 2 * offset, P26, w, ROWS_A, spp, F, far, ow, S30); ctx.sync()
        for c in range(4):
            assert np.array_equal(far[c * S30:c * S30 + oh * ow].cpu().numpy().reshape(oh, ow), want[c]), c
        assert _holds(far, SENT, [(c * S30, c * S30 + oh * ow) for c in range(4)])
        del far
    del src
    _free()


def test_histogram_and_lut_huge_pitch(ctx):
    """oip_histogram_u16 and oip_apply_lut_u8 (three planes, side by side in the same lines) with pitch 2^26.  Peak: 5.2 GB."""
    import _quicklook_ref
    torch = _torch()
    w = 1001
    planes = [_image_a(w, 30 + c) for c in range(3)]
    _past((ROWS_A - 1) * P26 + 2 * 1024)
    buf = _empty((ROWS_A - 1) * P26 + 4096)
    for c in range(3):
        _pitched(planes[c], offset=c * 1024, buf=buf)
    hist = torch.zeros(65536, dtype=torch.int64, device="cuda")
    ctx.histogram_u16(buf, P26, w, ROWS_A, hist); ctx.sync()
    assert np.array_equal(hist.cpu().numpy().view(np.uint64), _quicklook_ref.histogram(planes[0]))
    luts = np.random.default_rng(33).integers(0, 256, (3, 65536), dtype=np.uint8)
    out = torch.full((ROWS_A, w, 3), 7, dtype=torch.uint8, device="cuda")
    ctx.apply_lut_u8([buf.data_ptr() + 2 * c * 1024 for c in range(3)], P26, w, ROWS_A, _cuda(luts), out); ctx.sync()
    assert np.array_equal(out.cpu().numpy(), np.stack([luts[c][planes[c]] for c in range(3)], -1))
    del buf
    _free()


def test_window_to_f32_huge_pitch(ctx, oracle_mod):
    """oip_window_u16_to_f32 with pitch 2^26 and row0 33: every line it reads starts past 2^31.  Peak: 5.2 GB."""
    torch = _torch()
    img = _image_a(1000, 40)
    _past(33 * P26)
    src = _pitched(img)
    out = torch.zeros(7, 900, dtype=torch.float32, device="cuda")
    ctx.window_u16_to_f32(src, P26, 33, 50, 7, 900, out); ctx.sync()
    assert np.array_equal(out.cpu().numpy(), oracle_mod.window_u16_to_f32(img, 33, 50, 7, 900))
    del src
    _free()


# the first and the third geometry of test_gpu_resample.ALIGN_CASES (Wb, Lm, lps, off, ovl, keep, min_lines), its scene and its
# coefficients, restated here so that the two modules stay apart
ALIGN_A = [(75, 900, 400, 0, 52, False, 150), (64, 1000, 300, 17, 40, False, 100)]


def _align_scene(rng, Lm, Wb):
    img = rng.integers(64, 4096, (Lm, Wb)).astype(np.uint16)
    img[::97] = 65535
    img[::89] = 0
    return img


def _align_coef(rng, Wb):
    Wp = Wb * 4
    cx, cy = np.zeros((4, 2)), np.zeros((4, 3))
    for b in range(4):
        cx[b] = (rng.uniform(-6, 6), rng.uniform(-2e-4, 2e-4))
        cy[b] = (rng.uniform(-9, 9), rng.uniform(-4, 4) / Wp, rng.uniform(-8, 8) / (Wp * Wp))
    return cx, cy


@pytest.mark.parametrize("Wb,Lm,lps,off,ovl,keep,minl", ALIGN_A)
def test_align_mss_huge_plane_stride(ctx, oracle_mod, Wb, Lm, lps, off, ovl, keep, minl):
    """oip_align_mss_bicubic_u16x4 with the planes 2^30 elements apart: bands 2 and 3 are read past 2^31.  Wb = 75 is odd and
    takes the generic align_mss_kernel; Wb = 64 takes the kernels real strips use, align_mss8_kernel with align_fix_kernel
    behind it (the profiler says so).  Exact (MAX_DN = 0).  Peak: 6.4 GB."""
    rng = np.random.default_rng(0x0A11CE + Wb + Lm)
    bands = [_align_scene(rng, Lm, Wb) for _ in range(4)]
    cx, cy = _align_coef(rng, Wb)
    want, nvalid = oracle_mod.align_mss(bands, cx, cy, lps, off, ovl, keep, minl)
    _past(2 * S30)
    planes = _empty(3 * S30 + Lm * Wb)
    for b in range(4):
        planes[b * S30:b * S30 + Lm * Wb] = _cuda(bands[b]).reshape(-1)
    dst = _full(want.shape, 7)
    got = []
    ran = _kernels(ctx, lambda: got.append(ctx.align_mss_bicubic_u16x4(planes, S30, dst, Wb, Lm, cx, cy, lps, off, ovl, keep, minl)))
    assert got == [nvalid]
    assert ("align_fix_kernel" in ran) == (Wb % 2 == 0), ran
    assert np.array_equal(dst.cpu().numpy(), want)
    del planes
    _free()


def test_correlation_windows_huge_pitch(ctx):
    """oip_stt_correlate_windows and oip_interband_correlate_units on windows whose lines are 2^25 (160-line windows: lines 64
    on) and 2^26 (40-line band windows: lines 32 on) elements apart, so that pitch x row passes 2^31 inside a window: the bits
    of the same calls on contiguous copies of the windows.  Two units, the pair the call forms.
    Peak: 10.7 (2^25 x 159) + 5.2 GB."""
    P25, rows, cols = 1 << 25, 160, 64
    brows, bcols = rows // 4, cols // 4
    _past((rows - 1) * P25, (brows - 1) * P26)
    rng = np.random.default_rng(77)
    wins = [rng.integers(64, 4096, (rows, cols), dtype=np.uint16) for _ in range(4)]          # two pairs / two PAN windows
    bands = [[rng.integers(64, 4096, (brows, bcols), dtype=np.uint16) for _ in range(4)] for _ in range(2)]
    big = _empty((rows - 1) * P25 + 4 * 128)
    for i, wdw in enumerate(wins):
        for r in range(rows):
            big[r * P25 + 128 * i:r * P25 + 128 * i + cols] = _cuda(wdw[r])
    bbig = _empty((brows - 1) * P26 + 8 * 32)
    for u in range(2):
        for b in range(4):
            _pitched(bands[u][b], offset=32 * (4 * u + b), buf=bbig)
    ptr = [big.data_ptr() + 2 * 128 * i for i in range(4)]
    dense = [_cuda(wdw) for wdw in wins]
    got = ctx.stt_correlate_windows(ptr[:2], [P25] * 2, ptr[2:], [P25] * 2, rows, cols)
    want = ctx.stt_correlate_windows([d.data_ptr() for d in dense[:2]], [cols] * 2, [d.data_ptr() for d in dense[2:]], [cols] * 2, rows, cols)
    assert np.isfinite(want).all() and np.array_equal(got, want)
    bptr = [[bbig.data_ptr() + 2 * 32 * (4 * u + b) for b in range(4)] for u in range(2)]
    bdense = [[_cuda(x) for x in u] for u in bands]
    got = ctx.interband_correlate_units(ptr[:2], [P25] * 2, bptr, [P26] * 2, rows, cols)
    want = ctx.interband_correlate_units([d.data_ptr() for d in dense[:2]], [cols] * 2, [[x.data_ptr() for x in u] for u in bdense],
                                         [bcols] * 2, rows, cols)
    assert np.isfinite(want).all() and np.array_equal(got, want)
    del big, bbig
    _free()


def test_remap_window_huge_dst_pitch(ctx):
    """oip_remap_shift_bicubic_u16_window with dst_pitch 2^16 and L = 33000: destination lines from 32768 on start past 2^31.
    Equal to the plain call on a dense destination; the rest of the buffer keeps its sentinel.  Peak: 4.3 GB."""
    Wr, Lr, P, c0, coff = 1024, 33000, 1 << 16, 64, 2048
    dx, dy = 1.37, -2.4
    _past((Lr - 1) * P + coff)
    src = _rand12(Lr, Wr, 103)
    plain = _full((Lr, Wr))
    ctx.remap_shift_bicubic_u16(src, plain, Wr, Lr, dx, dy)
    far = _full((Lr, P))
    ctx.remap_shift_bicubic_u16_window(src, far, P, c0, coff, Wr, Lr, dx, dy); ctx.sync()
    n = Wr - c0
    assert _equal(far[:, coff:coff + n], plain[:, c0:])
    assert not bool((_i16(far[:, :coff]) != SENT - 65536).any()) and not bool((_i16(far[:, coff + n:]) != SENT - 65536).any())
    del src, plain, far
    _free()


def test_upload_staged_2d_past_4g_bytes(ctx):
    """oip_upload_staged_2d with device lines 2^27 bytes apart: lines 32 .. 39 land past byte 2^32.  Peak: 5.2 GB."""
    img = _image_a(1000, 60)
    pitch_b = 1 << 27
    assert (ROWS_A - 1) * pitch_b >= 1 << 32
    dev = _full(((ROWS_A - 1) * (pitch_b // 2) + 1024,))
    ctx.upload_staged_2d(dev, pitch_b, img); ctx.sync()
    rows = np.stack([dev[r * (pitch_b // 2):r * (pitch_b // 2) + 1000].cpu().numpy() for r in range(ROWS_A)])
    assert np.array_equal(rows, img)
    assert _holds(dev, SENT, [(r * (pitch_b // 2), r * (pitch_b // 2) + 1000) for r in range(ROWS_A)])
    del dev
    _free()
