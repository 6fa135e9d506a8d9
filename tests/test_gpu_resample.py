"""GPU parity: RRC, MSS split, constant-shift remap, inter-band align, RAW stitch.

Every test drives liboipgpu.so through the C ABI (opticalimageprocessor_amd.Context) on
cuda:0 and compares with the CPU oracle on the same seeded inputs.

Bars
  * RRC / MSS split / stitch: integer work, bit-exact.
  * remap / align (the float resampling path): the north star allows 1 ULP per pixel; the
    kernels reproduce OpenCV's f32 operation order, so the tests demand bit-exact output
    and only report the tolerance (MAX_DN = 0) in one place.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MAX_DN = 0   # allowed |GPU - oracle| in digital numbers for the resampling kernels


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _u16(t):
    # torch has no uint16 arithmetic but can carry the bytes
    return t.cpu().numpy()


def _rng(seed):
    return np.random.default_rng(0x0A11CE + seed)


def _lut(rng, w):
    k = np.round(rng.uniform(0.9, 1.1, w), 6)
    b = np.round(rng.uniform(-8, 8, w), 4)
    return np.stack([k, b], 1)


# ------------------------------------------------------------------------------------ RRC
@pytest.mark.parametrize("w,h", [(4096, 64), (30000, 37), (7500, 33), (12288, 8), (1001, 17), (8, 1), (3, 5)])
def test_rrc_matches_oracle(ctx, oracle_mod, w, h):
    import torch
    rng = _rng(w * 131 + h)
    img = rng.integers(0, 65536, (h, w), dtype=np.uint16)
    kb = _lut(rng, w)
    # adversarial columns: wrap, negative, huge, NaN, truncation boundary
    special = [(1.5015, 0.0), (-1.0, 0.0), (1.0, -90.0), (1.0, 70000.0), (3e5, 0.0), (1e9, 0.0), (-1e9, 0.0),
               (float("nan"), 0.0), (1.0, 0.999999999), (0.0, 65535.99999), (0.0, 2147483647.5), (0.0, 2147483648.0),
               (0.0, -2147483648.5), (0.0, -2147483649.0), (1.0, float("inf")), (0.0, -0.9999)]
    for i, (k, b) in enumerate(special[: max(0, min(len(special), w))]):
        kb[i] = (k, b)
    want = oracle_mod.rrc(img, kb)
    d_kb = ctx.upload_kb(kb)
    src = _cuda(img)
    dst = torch.empty_like(src)
    ctx.rrc_u16(src, dst, w, h, d_kb)      # out of place
    ctx.sync()
    assert np.array_equal(_u16(dst), want)
    ctx.rrc_u16(src, src, w, h, d_kb)      # in place, as IMO::InplaceRRC
    ctx.sync()
    assert np.array_equal(_u16(src), want)


def test_rrc_golden_fixture(ctx):
    import os
    import torch
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "rrc_reference.npz"))
    src = _cuda(g["src"])
    dst = torch.empty_like(src)
    h, w = g["src"].shape
    ctx.rrc_u16(src, dst, w, h, ctx.upload_kb(g["kb"]))
    ctx.sync()
    assert np.array_equal(_u16(dst), g["dst"])


def test_rrc_unaligned_views(ctx, oracle_mod):
    """sub-buffers that are only 2-byte aligned take the scalar kernel"""
    import torch
    rng = _rng(5)
    w, h = 1000, 9
    img = rng.integers(0, 65536, (h, w), dtype=np.uint16)
    kb = _lut(rng, w)
    base = torch.zeros(h * w + 8, dtype=torch.uint16, device="cuda")
    view = base[1:1 + h * w]
    view.copy_(_cuda(img).reshape(-1))
    ctx.rrc_u16(view, view, w, h, ctx.upload_kb(kb))
    ctx.sync()
    assert np.array_equal(_u16(view).reshape(h, w), oracle_mod.rrc(img, kb))


@pytest.mark.parametrize("off_px,w,h", [(8, 30000, 70), (24, 4096, 33), (504, 7504, 129), (0, 30000, 257), (64, 8, 3)])
def test_rrc_line_aligned_kernel_any_16B_offset(ctx, oracle_mod, off_px, w, h):
    """the flat kernel aligns its waves to the destination's 1 KiB frame: a raster that starts
    at any 16-byte offset inside an allocation (a row-block shard, a halo buffer) must come out
    the same, in place and out of place, and must not touch its neighbours"""
    import torch
    rng = _rng(off_px + w)
    img = rng.integers(0, 65536, (h, w), dtype=np.uint16)
    kb = _lut(rng, w)
    want = oracle_mod.rrc(img, kb)
    guard = 4096
    base = torch.full((guard + off_px + h * w + guard,), 0xABCD, dtype=torch.int32, device="cuda").to(torch.int16).view(torch.uint16)
    view = base[guard + off_px:guard + off_px + h * w]
    view.copy_(_cuda(img).reshape(-1))
    dst = torch.full_like(base, 0)
    dview = dst[guard + off_px:guard + off_px + h * w]
    d_kb = ctx.upload_kb(kb)
    ctx.rrc_u16(view, dview, w, h, d_kb); ctx.sync()
    assert np.array_equal(_u16(dview).reshape(h, w), want)
    assert int(dst.view(torch.int16).count_nonzero()) == int(np.count_nonzero(want))      # nothing outside
    ctx.rrc_u16(view, view, w, h, d_kb); ctx.sync()
    assert np.array_equal(_u16(view).reshape(h, w), want)
    b = _u16(base)
    assert (b[:guard + off_px] == 0xABCD).all() and (b[guard + off_px + h * w:] == 0xABCD).all()


def test_rrc_host_buffer(ctx, oracle_mod):
    rng = _rng(6)
    w, h = 4096, 20000     # 160 MB -> 3 staged blocks
    img = rng.integers(0, 4096, (h, w), dtype=np.uint16)
    kb = _lut(rng, w)
    want = oracle_mod.rrc(img, kb, threads=8)
    buf = img.copy()
    ctx.rrc_u16_host(buf, kb)
    assert np.array_equal(buf, want)


def test_staging_lanes_run_beside_the_compute_thread(ctx, oracle_mod):
    """The threading contract of include/oip_c.h: while the first thread drives kernels (with the profiler on) and
    downloads through the same context, a second thread runs oip_rrc_u16_host and a third uploads -- ring lane and
    download lane on their own streams and locks, the compute stream and the profiler untouched by them.  Every result
    must be exact and the profiler must have seen only the compute thread's launches."""
    import threading
    import torch
    rng = _rng(16)
    w, h = 4096, 12000
    kb = _lut(rng, w)
    imgs = [rng.integers(0, 4096, (h, w), dtype=np.uint16) for _ in range(3)]
    wants = [oracle_mod.rrc(a, kb, threads=8) for a in imgs]
    d_kb = ctx.upload_kb(kb)
    d_src = _cuda(imgs[0]); d_dst = torch.empty_like(d_src)
    d_up = torch.zeros(h, w, dtype=torch.uint16, device="cuda")
    host_bufs = [imgs[1].copy(), imgs[1].copy()]
    errors, tickets = [], []

    def host_rrc():
        try:
            for b in host_bufs:
                ctx.rrc_u16_host(b, kb)
        except Exception as e:      # noqa: BLE001
            errors.append(e)

    def uploader():
        try:
            for _ in range(2):
                tickets.append(ctx.upload_staged(d_up, imgs[2], want_ticket=True))
        except Exception as e:      # noqa: BLE001
            errors.append(e)
    ctx.sync()
    ctx.profile_reset(); ctx.profile_enable(True)
    th = [threading.Thread(target=host_rrc), threading.Thread(target=uploader)]
    [t.start() for t in th]
    downs = []
    for _ in range(6):
        ctx.rrc_u16(d_src, d_dst, w, h, d_kb)
        out = np.empty((h, w), np.uint16)
        ctx.download_staged(out, d_dst)
        downs.append(out)
    [t.join() for t in th]
    ctx.sync()
    ctx.profile_enable(False)
    prof = ctx.profile()
    assert not errors, errors
    for out in downs:
        assert np.array_equal(out, wants[0])
    for b in host_bufs:
        assert np.array_equal(b, wants[1])
    ctx.stage_wait(tickets[-1]); ctx.sync()
    assert np.array_equal(_u16(d_up), imgs[2])
    assert prof["rrc_u16_flat_kernel"][1] == 6, prof         # the staged RRC launches are not the compute thread's


@pytest.mark.parametrize("w,spitch,dpitch,soff,doff", [(4096, 4096, 8192, 0, 0), (29900, 30000, 59800, 0, 0), (1003, 1024, 2048, 0, 8),
                                                         (1000, 1001, 2003, 1, 3), (7, 64, 64, 0, 0)])
def test_rrc_window(ctx, oracle_mod, w, spitch, dpitch, soff, doff):
    """oip_rrc_u16_window: RRC of the first w columns into a window of a wider raster (the left half of the stitched line);
    aligned 8-column groups, a width that is not a multiple of 8, and pitches / offsets that force the scalar kernel.
    Nothing outside the window is written."""
    import torch
    rng = _rng(w + dpitch)
    h = 37
    src = rng.integers(0, 65536, (h, spitch), dtype=np.uint16)
    kb = _lut(rng, w)
    d_src = _cuda(src).reshape(-1)[soff:]
    dst = torch.full((h * dpitch + 64,), 0x5A5A, dtype=torch.int32, device="cuda").to(torch.int16).view(torch.uint16)
    rows_src = h - 1 if soff else h                  # an offset source window: keep the last line inside the allocation
    ctx.rrc_u16_window(d_src, spitch, dst[doff:], dpitch, w, rows_src, ctx.upload_kb(kb))
    ctx.sync()
    got = _u16(dst)
    flat = src.reshape(-1)[soff:]
    want_in = np.stack([flat[r * spitch:r * spitch + w] for r in range(rows_src)])
    want = oracle_mod.rrc(want_in, kb)
    canvas = np.full(h * dpitch + 64, 0x5A5A, np.uint16)
    for r in range(rows_src):
        canvas[doff + r * dpitch:doff + r * dpitch + w] = want[r]
    assert np.array_equal(got, canvas)


@pytest.mark.parametrize("W,fold,dx,dy,f16", [(2048, 100, 3.37, -1.62, False), (2048, 100, 3.37, -1.62, True), (1016, 37, -2.25, 4.5, False), (4096, 2500, -37.8, 2.25, True),
                                              (1001, 10, 0.5, -0.5, False), (4096, 2500, -37.8, 2.25, False),
                                              (6144, 40, 61.03, -0.75, False)])
def test_remap_window_equals_remap_then_stitch(ctx, W, fold, dx, dy, f16):
    """oip_remap_shift_bicubic_u16_window with the stitched raster's geometry (pitch 2 (W - fold), columns >= fold at offset
    W - fold) against the plain call followed by the stitch kernel: the right half must hold the same bits, the left half
    must stay untouched -- aligned vector stores (fold 100, W 2048), the group that straddles the fold, a misaligned
    destination (scalar stores) and a width that takes the generic kernel."""
    import torch
    rng = _rng(W + fold)
    L = 33000
    src = _cuda(rng.integers(0, 4096, (L, W), dtype=np.uint16))
    plain = torch.zeros(L, W, dtype=torch.uint16, device="cuda")
    ctx.remap_shift_bicubic_u16(src, plain, W, L, dx, dy, f16acc=f16)
    left = _cuda(rng.integers(0, 4096, (L, W), dtype=np.uint16))
    want = torch.zeros(L, 2 * (W - fold), dtype=torch.uint16, device="cuda")
    ctx.stitch_rows_u16(left, plain, want, W, L, fold)
    got = torch.zeros(L, 2 * (W - fold), dtype=torch.uint16, device="cuda")
    got[:, :W - fold] = left[:, :W - fold]
    ctx.remap_shift_bicubic_u16_window(src, got, 2 * (W - fold), fold, W - fold, W, L, dx, dy, f16acc=f16)
    ctx.sync()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    # the RAW strip as source, corrected on load (oip_remap_shift_rrc_bicubic_u16_window): src is the RRC of `raw` under a
    # LUT that maps 12-bit data onto other 12-bit data, so the three-pass result above is the reference bit for bit
    kb = np.stack([np.full(W, 1.0), np.zeros(W)], 1)
    kb[:, 0] += rng.integers(-3, 4, W) / 64.0
    kb[:, 1] = rng.integers(-8, 9, W) / 4.0
    raw = _cuda(rng.integers(16, 3900, (L, W), dtype=np.uint16))
    d_kb = ctx.upload_kb(kb)
    corrected = torch.empty_like(raw)
    ctx.rrc_u16(raw, corrected, W, L, d_kb)
    want2 = torch.zeros_like(want)
    want2[:, :W - fold] = left[:, :W - fold]
    ctx.remap_shift_bicubic_u16_window(corrected, want2, 2 * (W - fold), fold, W - fold, W, L, dx, dy, f16acc=f16)
    got2 = torch.zeros_like(want)
    got2[:, :W - fold] = left[:, :W - fold]
    ctx.remap_shift_rrc_bicubic_u16_window(raw, d_kb, got2, 2 * (W - fold), fold, W - fold, W, L, dx, dy, f16acc=f16)
    ctx.sync()
    assert torch.equal(got2.view(torch.int16), want2.view(torch.int16))
    assert not torch.equal(corrected.view(torch.int16), raw.view(torch.int16))
    # a row-block shard of the same call (rows 20000..26000 with their halo) writes the same lines
    o0, n = 20000, 6000
    import opticalimageprocessor_amd as oip
    f, l = oip.remap_shift_src_range(o0, n, L, dy)
    part = torch.zeros(n, 2 * (W - fold), dtype=torch.uint16, device="cuda")
    part[:, :W - fold] = left[o0:o0 + n, :W - fold]
    ctx.remap_shift_bicubic_u16_window(src[f:l], part, 2 * (W - fold), fold, W - fold, W, L, dx, dy, src_row0=f, src_rows=l - f,
                                       out_row0=o0, out_rows=n, f16acc=f16)
    ctx.sync()
    assert torch.equal(part.view(torch.int16), want[o0:o0 + n].view(torch.int16))


def test_remap_rrc_on_load_with_a_lut_that_leaves_the_int32_range(ctx):
    """remap_shift8_rrc_kernel drops the range test of IMO::InplaceRRC's double -> uint16_t cast when every (k, b) pair of a
    workgroup's columns keeps k s + b inside int32 (round 4).  Here some columns do not: k = 40000 (k s wraps past 2^31 for
    s > 53687: the x86 conversion gives 0x80000000 -> low half 0), a NaN gain, a hugely negative bias -- in one workgroup's
    columns only, so that the launch runs BOTH instantiations of the loop.  Reference: oip_rrc_u16 (bit-exact against the
    reference's own loop, tests/golden) followed by the plain window call."""
    import torch
    W, L, fold, dx, dy = 4096, 33000, 64, 2.37, -1.4
    rng = _rng(91)
    kb = np.stack([1.0 + rng.integers(-3, 4, W) / 64.0, rng.integers(-8, 9, W) / 4.0], 1)
    kb[2100, 0] = 40000.0
    kb[2101, 0] = np.nan
    kb[2102, 1] = -3.0e9
    kb[2103] = (-70000.0, 5.0)
    d_kb = ctx.upload_kb(kb)
    raw = _cuda(rng.integers(0, 65536, (L, W), dtype=np.uint16))
    corrected = torch.empty_like(raw)
    ctx.rrc_u16(raw, corrected, W, L, d_kb)
    P = 2 * (W - fold)
    for f16 in (False, True):
        want = torch.zeros(L, P, dtype=torch.uint16, device="cuda")
        ctx.remap_shift_bicubic_u16_window(corrected, want, P, fold, W - fold, W, L, dx, dy, f16acc=f16)
        got = torch.zeros_like(want)
        ctx.remap_shift_rrc_bicubic_u16_window(raw, d_kb, got, P, fold, W - fold, W, L, dx, dy, f16acc=f16)
        ctx.sync()
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), f16
    c = corrected.cpu().numpy()
    assert (c[:, 2101] == 0).all() and (c[:, 2100] == 0).any() and (c[:, 2100] != 0).any()      # NaN -> 0; the wrap does occur


def test_remap_rrc_on_load_with_a_misaligned_source(ctx):
    """oip_remap_shift_rrc_bicubic_u16_window stages 16-byte chunks of the raw lines through LDS; a source that is only 4-byte
    aligned takes the general kernel (which corrects on load as well) in fp32 -- same bits -- and is refused in the
    fp16-accumulate mode (OIP_E_UNSUPPORTED, nothing written)."""
    import torch
    W, L, fold, dx, dy = 1024, 33000, 64, 1.37, -2.4
    rng = _rng(77)
    kb = np.stack([1.0 + rng.integers(-3, 4, W) / 64.0, rng.integers(-8, 9, W) / 4.0], 1)
    d_kb = ctx.upload_kb(kb)
    flat = _cuda(rng.integers(16, 3900, L * W + 8, dtype=np.uint16))
    raw_al, raw_mis = flat[:L * W].view(L, W), flat[2:L * W + 2].view(L, W)
    raw_copy = raw_mis.clone()                                   # the same lines in an aligned allocation
    P = 2 * (W - fold)
    want = torch.zeros(L, P, dtype=torch.uint16, device="cuda")
    ctx.remap_shift_rrc_bicubic_u16_window(raw_copy, d_kb, want, P, fold, W - fold, W, L, dx, dy)
    got = torch.zeros_like(want)
    ctx.remap_shift_rrc_bicubic_u16_window(raw_mis, d_kb, got, P, fold, W - fold, W, L, dx, dy)
    ctx.sync()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert int(want[:, W - fold:].to(torch.int32).max()) > 0
    untouched = torch.full_like(want, 7)
    with pytest.raises(NotImplementedError):                     # OIP_E_UNSUPPORTED in the Python binding
        ctx.remap_shift_rrc_bicubic_u16_window(raw_mis, d_kb, untouched, P, fold, W - fold, W, L, dx, dy, f16acc=True)
    ctx.sync()
    assert int((untouched.to(torch.int32) != 7).sum()) == 0
    del raw_al


def test_upload_staged_2d_column_block(ctx):
    """oip_upload_staged_2d: a column block of a pageable raster into the same columns of a device raster, through the pinned ring
    (more than one 32 MiB slot), with a ticket; the columns beside it stay as they were."""
    import torch
    L, W, c0, c1 = 9000, 6000, 1504, 5008
    rng = _rng(9)
    host = rng.integers(0, 65536, (L, W), dtype=np.uint16)
    dev = torch.full((L, W), 0x1111, dtype=torch.int32, device="cuda").to(torch.int16).view(torch.uint16)
    t = ctx.upload_staged_2d(dev, W * 2, host[:, c0:c1], want_ticket=True, byte_offset=c0 * 2)
    ctx.stage_wait(t)
    ctx.sync()
    got = _u16(dev)
    want = np.full((L, W), 0x1111, np.uint16)
    want[:, c0:c1] = host[:, c0:c1]
    assert np.array_equal(got, want)
    # a row range of the block, no ticket (the compute stream is ordered behind it by the call)
    ctx.upload_staged_2d(dev, W * 2, host[100:200, 0:64], byte_offset=100 * W * 2)
    ctx.sync()
    want[100:200, 0:64] = host[100:200, 0:64]
    assert np.array_equal(_u16(dev), want)


def test_rrc_idempotent_lut_full_size(ctx):
    """BASELINE config 2 size (30000 x 65536): k=1,b=0 is the identity, k=0,b=c a constant --
    size-independent properties, no oracle run at this size."""
    import torch
    w, h = 30000, 65536
    g = torch.Generator(device="cuda").manual_seed(7)
    src = torch.randint(-32768, 32768, (h, w), device="cuda", generator=g, dtype=torch.int32).to(torch.int16).view(torch.uint16)
    dst = torch.empty_like(src)
    kb = np.zeros((w, 2)); kb[:, 0] = 1.0
    ctx.rrc_u16(src, dst, w, h, ctx.upload_kb(kb)); ctx.sync()
    assert torch.equal(dst.view(torch.int16), src.view(torch.int16))
    kb[:, 0] = 0.0; kb[:, 1] = np.arange(w) % 65536 + 0.75
    ctx.rrc_u16(src, dst, w, h, ctx.upload_kb(kb)); ctx.sync()
    want = torch.from_numpy((np.arange(w) % 65536).astype(np.uint16)).cuda()
    assert torch.equal(dst.view(torch.int16), want.view(torch.int16).expand(h, w))


# ------------------------------------------------------------------------------ MSS split
@pytest.mark.parametrize("w,lines,rrc", [(12288, 40, True), (30000, 21, True), (30000, 21, False), (4000, 7, True), (1004, 9, True), (1002, 5, True)])
def test_mss_split_rrc(ctx, oracle_mod, w, lines, rrc):
    import torch
    rng = _rng(w + lines)
    bil = rng.integers(0, 65536, (lines, w), dtype=np.uint16)
    bw = w // 4
    kbs = [_lut(rng, bw) for _ in range(4)]
    bands = oracle_mod.split_mss(bil)
    if rrc:
        bands = [oracle_mod.rrc(b, kb) for b, kb in zip(bands, kbs)]
    stride = bw * lines + 12            # deliberately not the tight size (multiple of 4)
    planes = torch.zeros(4 * stride, dtype=torch.uint16, device="cuda")
    d_kb = ctx.upload_kb(np.concatenate(kbs, 0)) if rrc else None
    ctx.mss_split_rrc_u16(_cuda(bil), planes, stride, w, lines, d_kb)
    ctx.sync()
    got = _u16(planes)
    for b in range(4):
        assert np.array_equal(got[b * stride:b * stride + bw * lines].reshape(lines, bw), bands[b]), b


# ---------------------------------------------------------------------------------- stitch
@pytest.mark.parametrize("W,L,fold", [(12288, 33, 100), (30000, 17, 100), (1000, 21, 25), (1000, 21, 24), (999, 7, 3), (64, 5, 0), (200, 9, 1)])
def test_stitch_rows(ctx, oracle_mod, W, L, fold):
    import torch
    rng = _rng(W + fold)
    left = rng.integers(0, 65536, (L, W), dtype=np.uint16)
    right = rng.integers(0, 65536, (L, W), dtype=np.uint16)
    want = oracle_mod.stitch_raw(left, right, fold)
    out = torch.zeros(L, 2 * (W - fold), dtype=torch.uint16, device="cuda")
    ctx.stitch_rows_u16(_cuda(left), _cuda(right), out, W, L, fold)
    ctx.sync()
    assert np.array_equal(_u16(out), want)


# ------------------------------------------------------------------- constant-shift remap
def _scene(rng, L, W):
    img = rng.integers(64, 4096, (L, W)).astype(np.uint16)
    img[::97] = 65535      # saturating rows exercise the clamp at bicubic overshoot
    img[::89] = 0
    return img


SHIFT_CASES = [
    # W,   L,    dx,      dy,     section_rows, row_guard
    (96,  700,  3.37,   -1.62,   300, 327),      # negative dy: upper cut
    (96,  700,  -2.25,  2.4,     300, 327),      # positive dy: bottom cut, short last section (stale tail)
    (64,  900,  0.0,    0.0,     300, 300),      # identity except seams
    (80,  601,  5.999,  7.03125, 300, 327),      # phase rounding near integer; last section 1 line over
    (33,  1000, -40.5,  -12.49,  256, 300),      # big negative shift: left border, large ucut
    (200, 640,  197.3,  3.0,     320, 327),      # almost everything right of the image
    (128, 35000, 1.53,  -0.77,   30000, 32767),  # the reference's real constants
]


@pytest.mark.parametrize("W,L,dx,dy,sr,guard", SHIFT_CASES)
def test_remap_shift_matches_oracle(ctx, oracle_mod, W, L, dx, dy, sr, guard):
    import torch
    rng = _rng(int(W * 7 + L))
    src = _scene(rng, L, W)
    want, row_off = oracle_mod.prestitch(src, dx, dy, sr, guard)
    dst = torch.zeros(L, W, dtype=torch.uint16, device="cuda")
    ctx.remap_shift_bicubic_u16(_cuda(src), dst, W, L, dx, dy, sr, guard)
    ctx.sync()
    got = _u16(dst).astype(np.int32)
    diff = np.abs(got - want.astype(np.int32))
    assert diff.max() <= MAX_DN, (diff.max(), np.argwhere(diff > MAX_DN)[:5])


def test_remap_shift_too_few_rows(ctx):
    import torch
    src = torch.zeros(100, 64, dtype=torch.uint16, device="cuda")
    with pytest.raises(ValueError, match="too few data rows"):
        ctx.remap_shift_bicubic_u16(src, src.clone(), 64, 100, 1.0, 1.0)   # imageop.h:242-244


@pytest.mark.parametrize("nshards", [2, 3, 8])
def test_remap_shift_row_shards_equal_whole(ctx, oracle_mod, nshards):
    """scan-line-block sharding: every shard computes from [halo] lines only and the
    concatenation equals the unsharded result."""
    import torch
    import opticalimageprocessor_amd as oip
    W, L, dx, dy, sr, guard = 96, 1500, 2.6, 3.3, 300, 327
    src = _scene(_rng(99), L, W)
    want, _ = oracle_mod.prestitch(src, dx, dy, sr, guard)
    got = np.zeros_like(want)
    for k in range(nshards):
        o0, o1 = L * k // nshards, L * (k + 1) // nshards
        s0, s1 = oip.remap_shift_src_range(o0, o1 - o0, L, dy, sr)
        assert 0 <= s0 <= s1 <= L
        part = torch.zeros(o1 - o0, W, dtype=torch.uint16, device="cuda")
        ctx.remap_shift_bicubic_u16(_cuda(src[s0:s1]), part, W, L, dx, dy, sr, guard, src_row0=s0, src_rows=s1 - s0,
                                    out_row0=o0, out_rows=o1 - o0)
        ctx.sync()
        got[o0:o1] = _u16(part)
    assert np.array_equal(got, want)
    # a shard without its halo must be refused, not silently wrong
    # (dy > 0: the taps of the first half reach below its last line)
    with pytest.raises(ValueError, match="halo"):
        o0, o1 = 0, L // 2
        part = torch.zeros(o1 - o0, W, dtype=torch.uint16, device="cuda")
        ctx.remap_shift_bicubic_u16(_cuda(src[o0:o1]), part, W, L, dx, dy, sr, guard, src_row0=o0, src_rows=o1 - o0,
                                    out_row0=o0, out_rows=o1 - o0)


@pytest.mark.parametrize("nshards", [2, 3, 8])
def test_remap_shift_row_shards_equal_whole_f16acc(ctx, nshards):
    """the fp16-accumulate mode in scan-line blocks, as `oip prestitch --gpus N --fp16-accumulate` runs it: the shards put
    together equal the unsharded fp16 call bit for bit (that call's distance from the oracle has its own test)"""
    import torch
    import opticalimageprocessor_amd as oip
    W, L, dx, dy, sr, guard = 96, 1500, 2.6, 3.3, 300, 327
    src = _scene(_rng(99), L, W)
    whole = torch.zeros(L, W, dtype=torch.uint16, device="cuda")
    ctx.remap_shift_bicubic_u16(_cuda(src), whole, W, L, dx, dy, sr, guard, f16acc=True)
    ctx.sync()
    want = _u16(whole)
    assert want.any()
    got = np.zeros_like(want)
    for k in range(nshards):
        o0, o1 = L * k // nshards, L * (k + 1) // nshards
        s0, s1 = oip.remap_shift_src_range(o0, o1 - o0, L, dy, sr)
        part = torch.zeros(o1 - o0, W, dtype=torch.uint16, device="cuda")
        ctx.remap_shift_bicubic_u16(_cuda(src[s0:s1]), part, W, L, dx, dy, sr, guard, src_row0=s0, src_rows=s1 - s0,
                                    out_row0=o0, out_rows=o1 - o0, f16acc=True)
        ctx.sync()
        got[o0:o1] = _u16(part)
    assert np.array_equal(got, want)


def test_remap_integer_shift_is_copy(ctx):
    """known answer: integer shift == shifted copy with zero border (per section)"""
    import torch
    W, L = 64, 400                              # section_rows 390, guard 399: L just passes the guard
    rng = _rng(3)
    src = rng.integers(0, 65536, (L, W), dtype=np.uint16)
    dst = torch.zeros(L, W, dtype=torch.uint16, device="cuda")
    ctx.remap_shift_bicubic_u16(_cuda(src), dst, W, L, 5.0, 0.0, 390, 399)
    ctx.sync()
    got = _u16(dst)
    assert np.array_equal(got[:380, :W - 5], src[:380, 5:])
    assert (got[:380, W - 5:] == 0).all()


# ------------------------------------------------------------------------ inter-band align
ALIGN_CASES = [
    # Wb,  Lm,   lps,  off, ovl, keep, min_lines
    (75,   900,  400,  0,   52,  False, 150),
    (75,   900,  400,  0,   52,  True,  150),
    (64,   1000, 300,  17,  40,  False, 100),
    (96,   650,  300,  0,   30,  False, 200),     # last section shorter than min_lines: zero tail
    (3072, 1600, 20000, 0,  520, False, 1500),    # reference constants, single section
]


def _coef(rng, Wb, big=False):
    W = Wb * 4
    cx = np.zeros((4, 2)); cy = np.zeros((4, 3))
    for b in range(4):
        cx[b] = (rng.uniform(-6, 6), rng.uniform(-2e-4, 2e-4))
        # dy = c0 + c1*x + c2*x^2, a few PAN pixels of curvature across the line
        c2 = rng.uniform(-8, 8) / (W * W)
        cy[b] = (rng.uniform(-9, 9), rng.uniform(-4, 4) / W, c2)
    if big:
        cx[0, 0] = -3.0 * W      # band 0 mapped completely off the left edge
        cy[1, 0] = 5000.0        # band 1 far below its section
    return cx, cy


@pytest.mark.parametrize("Wb,Lm,lps,off,ovl,keep,minl", ALIGN_CASES)
def test_align_mss_matches_oracle(ctx, oracle_mod, Wb, Lm, lps, off, ovl, keep, minl):
    import torch
    rng = _rng(Wb + Lm + int(keep))
    bands = [_scene(rng, Lm, Wb) for _ in range(4)]
    cx, cy = _coef(rng, Wb)
    want, nvalid = oracle_mod.align_mss(bands, cx, cy, lps, off, ovl, keep, minl)
    planes = _cuda(np.stack(bands, 0))
    dst = torch.full(want.shape, 7, dtype=torch.uint16, device="cuda")
    got_valid = ctx.align_mss_bicubic_u16x4(planes, Wb * Lm, dst, Wb, Lm, cx, cy, lps, off, ovl, keep, minl)
    ctx.sync()
    assert got_valid == nvalid
    diff = np.abs(_u16(dst).astype(np.int32) - want.astype(np.int32))
    assert diff.max() <= MAX_DN, (diff.max(), np.argwhere(diff > MAX_DN)[:5])


def test_align_mss_out_of_image_bands(ctx, oracle_mod):
    import torch
    Wb, Lm = 80, 500
    rng = _rng(11)
    bands = [_scene(rng, Lm, Wb) for _ in range(4)]
    cx, cy = _coef(rng, Wb, big=True)
    want, _ = oracle_mod.align_mss(bands, cx, cy, 300, 0, 40, False, 100)
    dst = torch.zeros(want.shape, dtype=torch.uint16, device="cuda")
    ctx.align_mss_bicubic_u16x4(_cuda(np.stack(bands, 0)), Wb * Lm, dst, Wb, Lm, cx, cy, 300, 0, 40, False, 100)
    ctx.sync()
    assert np.array_equal(_u16(dst), want)


def test_align_argument_errors(ctx):
    import torch
    planes = torch.zeros(4 * 64 * 2000, dtype=torch.uint16, device="cuda")
    dst = torch.zeros(2000 * 64 * 4, dtype=torch.uint16, device="cuda")
    z2, z3 = np.zeros((4, 2)), np.zeros((4, 3))
    with pytest.raises(ValueError, match="exceeds maximum"):       # preproc.h:355-358
        ctx.align_mss_bicubic_u16x4(planes, 64 * 2000, dst, 64, 2000, z2, z3, 20000, 0, 3001)
    with pytest.raises(ValueError, match="OpenCV allowed"):        # preproc.h:359-361
        ctx.align_mss_bicubic_u16x4(planes, 64 * 2000, dst, 64, 2000, z2, z3, 40000, 0, 520)
    with pytest.raises(ValueError, match="too small"):             # preproc.h:362-364
        ctx.align_mss_bicubic_u16x4(planes, 64 * 2000, dst, 64, 2000, z2, z3, 1000, 0, 520)
    with pytest.raises(ValueError, match="Too few"):               # preproc.h:365-367
        ctx.align_mss_bicubic_u16x4(planes, 64 * 2000, dst, 64, 2000, z2, z3, 20000, 600, 520)


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


def _align_row_shards(ctx, oracle_mod, nshards, Wb, head=0, tail=0):
    """every shard of output rows computed from its window of source lines [s0, s1) only; the window sits `head` lines into
    planes of head + (s1 - s0) + tail lines whose other lines hold 0xFFFF.  -> (result, oracle, kernels that ran)"""
    import torch
    import opticalimageprocessor_amd as oip
    Lm, lps, ovl, minl = 1200, 400, 52, 150
    rng = _rng(21)
    bands = [_scene(rng, Lm, Wb) for _ in range(4)]
    cx, cy = _coef(rng, Wb)
    want, _ = oracle_mod.align_mss(bands, cx, cy, lps, 0, ovl, False, minl)
    R = want.shape[0]
    got = np.zeros_like(want)
    stack = np.stack(bands, 0)
    ran = set()
    for k in range(nshards):
        o0, o1 = R * k // nshards, R * (k + 1) // nshards
        s0, s1 = oip.align_mss_src_range(o0, o1 - o0, Lm, cy, Wb, lps, 0, ovl, False, minl)
        cap = head + (s1 - s0) + tail
        sub = np.full((4, cap, Wb), 0xFFFF, np.uint16)
        sub[:, head:head + s1 - s0] = stack[:, s0:s1]
        planes = _cuda(sub).view(-1)[head * Wb:]
        part = torch.zeros(o1 - o0, Wb, 4, dtype=torch.uint16, device="cuda")
        ran |= _kernels(ctx, lambda: ctx.align_mss_bicubic_u16x4(planes, Wb * cap, part, Wb, Lm, cx, cy, lps, 0, ovl, False, minl,
                                                                 src_row0=s0, src_rows=s1 - s0, out_row0=o0, out_rows=o1 - o0))
        got[o0:o1] = _u16(part)
    return got, want, ran


@pytest.mark.parametrize("nshards", [2, 5])
def test_align_row_shards_equal_whole(ctx, oracle_mod, nshards):
    got, want, ran = _align_row_shards(ctx, oracle_mod, nshards, 75)
    assert "align_fix_kernel" not in ran, ran          # an odd width: the general kernel
    assert np.array_equal(got, want)


@pytest.mark.parametrize("nshards,head,tail", [(2, 0, 0), (5, 0, 0), (5, 3, 7)])
def test_align_row_shards_equal_whole_even_width(ctx, oracle_mod, nshards, head, tail):
    """The same at Wb = 96, the form the N-GPU host calls (RunDefaultActionMultiGpu): an even width takes align_mss8_kernel with
    align_fix_kernel behind it (the profiler says so) on a row window with src_row0 != 0, where the fast kernel's hand-off
    conditions `l0 >= 0 && l0 + 3 < src_rows` and its prefetch guard `nline < src_rows` decide.  (5, 3, 7): the window sits
    inside planes with plane_stride > src_rows * Wb, as in the host's m_cap layout; the lines around it hold 0xFFFF, so a tap
    taken outside the window shows.  Exact equality with the oracle."""
    got, want, ran = _align_row_shards(ctx, oracle_mod, nshards, 96, head, tail)
    assert "align_fix_kernel" in ran, ran
    assert np.array_equal(got, want)


# ------------------------------------------------------- BASELINE sizes: size-independent properties
def _rand_u16(shape, seed):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(-32768, 32768, shape, device="cuda", generator=g, dtype=torch.int32).to(torch.int16).view(torch.uint16)


def test_full_size_remap_integer_shift_is_copy(ctx):
    """30000 x 65536 (BASELINE config 2/3 width and length): an integer shift has phase 0, weights
    [0,1,0,0], so every section body must be an exact shifted copy; the lines next to the 30000-row
    section seams are exact too (the zeroed taps carry weight 0)."""
    import torch
    W, L, sx, sy = 30000, 65536, 7, 3
    src = _rand_u16((L, W), 11)
    dst = torch.empty_like(src)
    ctx.remap_shift_bicubic_u16(src, dst, W, L, float(sx), float(sy))
    ctx.sync()
    bcut = sy + 1
    body = L - bcut - sy           # lines whose source line exists
    assert torch.equal(dst[:body, :W - sx].view(torch.int16), src[sy:sy + body, sx:].view(torch.int16))
    assert int(dst[:body, W - sx:].view(torch.int16).count_nonzero()) == 0


def test_full_size_align_zero_coefficients_interleaves_bands(ctx):
    """MSS of BASELINE config 3 (4 x 7500 x 16384): zero polynomials map every pixel onto itself,
    so the 16UC4 output is the band interleave of lines [overlap, L) (leading overlap dropped)."""
    import torch
    Wb, Lm = 7500, 16384
    planes = _rand_u16((4, Lm, Wb), 12)
    out = torch.empty(Lm - 520, Wb, 4, dtype=torch.uint16, device="cuda")
    n = ctx.align_mss_bicubic_u16x4(planes, Lm * Wb, out, Wb, Lm, np.zeros((4, 2)), np.zeros((4, 3)))
    ctx.sync()
    assert n == Lm - 520
    want = planes[:, 520:].permute(1, 2, 0).contiguous()
    assert torch.equal(out.view(torch.int16), want.view(torch.int16))


def test_full_size_stitch_columns(ctx):
    """two 30000 x 65536 strips, fold 100: left part == left[:, :W-f], right part == right[:, f:]"""
    import torch
    W, L, f = 30000, 65536, 100
    left, right = _rand_u16((L, W), 13), _rand_u16((L, W), 14)
    out = torch.empty(L, 2 * (W - f), dtype=torch.uint16, device="cuda")
    ctx.stitch_rows_u16(left, right, out, W, L, f)
    ctx.sync()
    assert torch.equal(out[:, :W - f].view(torch.int16), left[:, :W - f].view(torch.int16))
    assert torch.equal(out[:, W - f:].view(torch.int16), right[:, f:].view(torch.int16))


def test_full_size_mss_split_round_trip(ctx):
    """BIL 30000 x 16384 -> 4 planar bands without RRC: re-interleaving gives the input back"""
    import torch
    W, L = 30000, 16384
    bil = _rand_u16((L, W), 15)
    planes = torch.empty(4, L, W // 4, dtype=torch.uint16, device="cuda")
    ctx.mss_split_rrc_u16(bil, planes, L * (W // 4), W, L, None)
    ctx.sync()
    back = planes.permute(1, 0, 2).reshape(L, W)
    assert torch.equal(back.view(torch.int16), bil.view(torch.int16))


@pytest.mark.parametrize("shape", [(5, 8, 256, 1536), (2, 3, 5, 7), (3, 2, 16, 24), (1, 1, 1, 8)])
def test_merge_subimages_be16(ctx, oracle_mod, shape):
    """sub-image merge + byte-order pass of the de-framer (aux_separator.h:341-393), the
    reference frame geometry and odd ones (scalar fall-back), bit-exact against the oracle"""
    import torch
    rng = np.random.default_rng(sum(shape))
    tiles = rng.integers(0, 65536, shape).astype(np.uint16)
    d_in = torch.from_numpy(tiles.view(np.int16)).cuda()
    d_out = torch.zeros(shape[0] * shape[2], shape[1] * shape[3], dtype=torch.int16, device="cuda")
    ctx.merge_subimages_be16(d_in, d_out, *shape)
    ctx.sync()
    got = d_out.cpu().numpy().view(np.uint16)
    assert np.array_equal(got, oracle_mod.merge_subimages_be16(tiles))
    with pytest.raises(ValueError):
        ctx.merge_subimages_be16(d_in, d_in, *shape)


def test_profile_filter_times_only_the_named_kernel(ctx):
    """oip_profile_filter: bench.py times only the dominant kernel inside its timed region"""
    import torch
    W, H = 4096, 64
    src = torch.zeros(H, W, dtype=torch.int16, device="cuda")
    dst = torch.empty_like(src)
    left = torch.zeros(H, W, dtype=torch.int16, device="cuda")
    out = torch.empty(H, 2 * (W - 8), dtype=torch.int16, device="cuda")
    kb = ctx.upload_kb(np.stack([np.ones(W), np.zeros(W)], 1))
    try:
        ctx.profile_reset()
        ctx.profile_filter("stitch_rows_kernel")
        ctx.profile_enable(True)
        ctx.rrc_u16(src, dst, W, H, kb)
        ctx.stitch_rows_u16(left, dst, out, W, H, 8)
        ctx.rrc_u16(src, dst, W, H, kb)
        ctx.sync()
        ctx.profile_enable(False)
        prof = ctx.profile()
        assert list(prof) == ["stitch_rows_kernel"] and prof["stitch_rows_kernel"][1] == 1 and prof["stitch_rows_kernel"][0] > 0
        ctx.profile_filter(None)
        ctx.profile_reset()
        ctx.profile_enable(True)
        ctx.rrc_u16(src, dst, W, H, kb)
        ctx.stitch_rows_u16(left, dst, out, W, H, 8)
        ctx.sync()
        ctx.profile_enable(False)
        assert len(ctx.profile()) == 2
    finally:
        ctx.profile_filter(None)
        ctx.profile_enable(False)
        ctx.profile_reset()
