"""The device Deflate encoder (csrc/tiffdeflate.hip, oip_tiff_deflate_strips_u16: a zlib stream per wave, the encoder of
csrc/oip_deflate.h) against zlib, against the host instantiation of the same coder (oip_deflate_stream_host: byte for byte) and
against the project's own device decoder.  The host build of this code has been through the same kinds of input under ASan + UBSan
(tests/test_deflate_encode_cpu.py)."""
import zlib

import numpy as np
import pytest
import torch

import opticalimageprocessor_amd as oip
import _deflate_write_ref as R
import _tiff_boundary as B

pytestmark = pytest.mark.gpu

GUARD = 4096            # bytes behind the payload, pre-filled, that no encode may touch
PATTERN = 0xA5


def _two_row_period(rows, width, spp, seed):
    """blocky along the row, and row r + 2 repeats row r"""
    two = R.blocks(2, width, spp, seed, 28)
    return np.ascontiguousarray(np.tile(two, (-(-rows // 2), 1))[:rows])


def _zero_then_noise(rows, width, spp, seed):
    a = R.noise12(rows, width, spp, seed)
    a[:rows // 2] = 0
    return a


SHAPES = [
    (1, 1, 1, 1, R.noise12),               # a 2-byte stream
    (3, 1, 4, 1, R.noise12),               # predictor with nothing before it
    (5, 7, 1, 2, R.noise12),               # 14-byte rows, odd-length streams, a short last strip, even offsets
    (33, 700, 4, 11, lambda h, w, s, seed: R.blocks(h, w, s, seed, 28)),       # matches at distance 5600, 61.6 KB strips
    (6, 4100, 4, 1, _two_row_period),      # 32800-byte rows: the window wraps inside a stream
    (64, 1000, 1, 32, R.noise12),          # dynamic codes
    (1024, 512, 4, 512, _zero_then_noise), # two 2 MiB streams, one all zero and one noise
]


@pytest.mark.parametrize("rows,width,spp,rps,make", SHAPES, ids=["%dx%dx%d_rps%d" % s[:4] for s in SHAPES])
def test_strips_are_zlib_streams_and_the_host_coders_bytes(ctx, rows, width, spp, rps, make):
    img = make(rows, width, spp, rows + width)
    d_img = torch.from_numpy(img.view(np.int16)).cuda()
    worst = ctx.tiff_deflate_worst_bytes(rows, width, spp, rps)
    n = -(-rows // rps)
    full = rps * width * spp * 2
    assert worst >= n * (R.stored_bound(full) + 1) and worst <= n * (R.stored_bound(full) + 2)
    payload = torch.full((worst + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
    off, ln, total = ctx.tiff_deflate_strips(d_img, rows, width, spp, rps, payload, payload_cap=worst)
    host = payload.cpu().numpy()
    assert (host[worst:] == PATTERN).all() and total <= worst
    want = R.strip_bytes(img, spp, rps=rps)
    assert len(off) == len(want) == n
    pos = 0
    for k, data in enumerate(want):
        assert off[k] % 2 == 0 and off[k] >= pos and off[k] - pos <= 1, (k, off[k], pos)      # even, ascending, packed
        z = host[int(off[k]):int(off[k] + ln[k])].tobytes()
        o = zlib.decompressobj()
        assert o.decompress(z) == data and o.eof and not o.unused_data, k
        assert z == oip.deflate_stream_host(data), "strip %d: device and host bytes differ" % k
        assert len(z) <= R.stored_bound(len(data))
        pos = int(off[k] + ln[k])
    assert total == pos
    if rows == 1024:
        # the zero stream stays under the reader's plausibility check of 1032 : 1 (a match of 258 bytes costs at least 2 bits)
        # -- and is a few KB: 128 blocks of 64 matches at 2 bits plus a header of about a dozen bytes
        assert (2 << 20) // 1032 <= ln[0] + 16 and ln[0] < 8192, ln[0]
    # the project's own decoder returns the image
    back = torch.zeros(rows * width * spp, dtype=torch.int16, device="cuda")
    ctx.tiff_deflate_decode(payload[:total], off, ln, rows, width, spp, rps, 2, back)
    assert np.array_equal(back.cpu().numpy().view(np.uint16).reshape(img.shape), img)
    # a caller's scratch buffer gives the same payload
    scratch = torch.zeros(ctx.tiff_deflate_scratch_bytes(rows, width, spp, rps), dtype=torch.uint8, device="cuda")
    payload2 = torch.full((worst + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
    off2, ln2, total2 = ctx.tiff_deflate_strips(d_img, rows, width, spp, rps, payload2, scratch=scratch, payload_cap=worst)
    assert total2 == total and np.array_equal(off2, off) and np.array_equal(ln2, ln)
    for k in range(n):
        a, b = int(off[k]), int(off[k] + ln[k])
        assert np.array_equal(payload2[a:b].cpu().numpy(), host[a:b]), k
    assert (payload2[worst:].cpu().numpy() == PATTERN).all()
    # the image is read, never written
    assert np.array_equal(d_img.cpu().numpy().view(np.uint16), img)


def test_output_does_not_depend_on_the_batch_or_the_streams_index(ctx):
    """the strips of an image encoded alone, from a misaligned view, are the strips they are inside the image"""
    rows, width, spp, rps = 12, 300, 1, 2
    img = R.blocks(rows, width, spp, 77)
    d_img = torch.from_numpy(img.view(np.int16)).cuda()
    payload = torch.zeros(ctx.tiff_deflate_worst_bytes(rows, width, spp, rps), dtype=torch.uint8, device="cuda")
    off, ln, _ = ctx.tiff_deflate_strips(d_img, rows, width, spp, rps, payload)
    whole = payload.cpu().numpy()
    shifted = torch.zeros(rows * width + 1, dtype=torch.int16, device="cuda")
    shifted[1:] = d_img.reshape(-1)
    for k in (1, 4):
        one = torch.zeros(ctx.tiff_deflate_worst_bytes(rps, width, spp, rps), dtype=torch.uint8, device="cuda")
        o1, l1, t1 = ctx.tiff_deflate_strips(shifted[1 + k * rps * width:], rps, width, spp, rps, one)
        assert t1 == ln[k] and one[:t1].cpu().numpy().tobytes() == whole[int(off[k]):int(off[k] + ln[k])].tobytes(), k


def test_refusals_launch_nothing(ctx):
    rows, width, spp, rps = 8, 64, 4, 2
    img = R.noise12(rows, width, spp, 3)
    d_img = torch.from_numpy(img.view(np.int16)).cuda()
    worst = ctx.tiff_deflate_worst_bytes(rows, width, spp, rps)
    payload = torch.full((worst,), PATTERN, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        ctx.tiff_deflate_strips(d_img, rows, width, spp, rps, payload, payload_cap=worst - 1)
    with pytest.raises(ValueError):
        ctx.tiff_deflate_strips(d_img, rows, width, 3, rps, payload)
    with pytest.raises(ValueError):
        ctx.tiff_deflate_strips(d_img, rows, 0, spp, rps, payload)
    need = ctx.tiff_deflate_scratch_bytes(rows, width, spp, rps)
    scratch = torch.zeros(need, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        ctx.tiff_deflate_strips(d_img, rows, width, spp, rps, payload, scratch=scratch, scratch_bytes=need - 1)
    assert ctx.tiff_deflate_worst_bytes(rows, 0, spp, rps) == 0 and ctx.tiff_deflate_scratch_bytes(0, width, spp, rps) == 0
    ctx.sync()
    assert (payload.cpu().numpy() == PATTERN).all()
    off, ln, total = ctx.tiff_deflate_strips(d_img, rows, width, spp, rps, payload, scratch=scratch)
    assert total > 0 and zlib.decompress(payload[:int(ln[0])].cpu().numpy().tobytes()) == R.strip_bytes(img, spp, rps=rps)[0]


@pytest.mark.parametrize("own_scratch", [True, False], ids=["own_scratch", "callers_scratch"])
def test_strips_across_the_launch_boundary(ctx, own_scratch):
    """32770 one-row strips: launches of 32768 and 2 (tests/_tiff_boundary.py).  Stream 32767 is odd by the host coder's count, so the
    second launch's first offset carries the pad byte of the first launch's last stream."""
    rows = B.rows_named(["zero", "noise16", "const", "small", "noise12"])
    streams = [oip.deflate_stream_host(B.predict2(r)) for r in rows]
    for r, z in zip(rows, streams):
        assert zlib.decompress(z) == B.predict2(r)
    B.check_two_launches(ctx, ctx.tiff_deflate_strips, ctx.tiff_deflate_worst_bytes, ctx.tiff_deflate_scratch_bytes, rows, B.WIDTH, 1,
                         B.pattern_of_rows(len(rows)), streams, own_scratch)


def test_misaligned_scratch_is_refused(ctx):
    rows, width, spp, rps = 8, 64, 4, 2
    d_img = torch.zeros(rows * width * spp, dtype=torch.int16, device="cuda")
    payload = torch.full((ctx.tiff_deflate_worst_bytes(rows, width, spp, rps),), PATTERN, dtype=torch.uint8, device="cuda")
    need = ctx.tiff_deflate_scratch_bytes(rows, width, spp, rps)
    scratch = torch.zeros(need + 8, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="scratch too small or misaligned"):
        ctx.tiff_deflate_strips(d_img, rows, width, spp, rps, payload, scratch=scratch[4:], scratch_bytes=need)
    ctx.sync()
    assert (payload.cpu().numpy() == PATTERN).all()
