"""The device LZW strip encoder (csrc/tifflzw.hip, oip_tiff_lzw_strips_u16) against an independent restatement of TIFF 6.0
sections 13 (LZW as libtiff writes it) and 14 (horizontal predictor): tests/_tiff.py::lzw_encode -- a dictionary of byte strings,
nothing in common with the open-addressing coders of the product -- on the predictor-2 byte stream of every strip, bit for bit.
The reference encodes these strips on the host through cv::imwrite (preproc.h:167-185) and GDAL (imageop.h:460-567)."""
import functools

import numpy as np
import pytest
import torch

import _lzw_cases as L
import _tiff
import _tiff_boundary as B

pytestmark = pytest.mark.gpu


def _image(kind, rows, width, spp, seed):
    rng = np.random.default_rng(seed)
    n = rows * width * spp
    if kind == "noise12":                      # sensor-like: barely compresses, the table fills every ~5 KB
        a = np.clip(rng.normal(1800.0, 300.0, n), 64, 4095).astype(np.uint16)
    elif kind == "noise16":                    # nothing repeats: a code per byte, ClearCode every 3836 bytes
        a = rng.integers(0, 65536, n, dtype=np.uint16)
    elif kind == "ramp":                       # constant differences: long matches, slow code-width growth
        a = (np.arange(n, dtype=np.uint64) * 3 % 65536).astype(np.uint16)
    elif kind == "constant":
        a = np.full(n, 4242, dtype=np.uint16)
    else:                                      # smooth scene + a little noise
        x = np.arange(n, dtype=np.float64)
        a = (2000 + 800 * np.sin(x / 977.0) + rng.integers(0, 4, n)).astype(np.uint16)
    return a.reshape(rows, width * spp)


def _predict(block, spp):
    """TIFF predictor 2 on 16-bit samples, row by row, as the little-endian byte stream the coder sees"""
    d = block.astype(np.uint16).copy()
    d[:, spp:] = (block[:, spp:].astype(np.int32) - block[:, :-spp].astype(np.int32)).astype(np.uint16)
    return d.astype("<u2").tobytes()


@pytest.mark.parametrize("rows,width,spp,rps,kind", [
    (40, 720, 4, 11, "noise12"),               # 63 KB strips of 11 rows, the last one short
    (9, 7500, 4, 1, "scene"),                  # the product's own strips: one 60000-byte row each
    (6, 2048, 1, 3, "ramp"),                   # one sample per pixel
    (5, 1000, 4, 2, "constant"),
    (3, 16384, 4, 1, "noise16"),               # 128 KB strips: ~34 table generations each
    (150, 64, 4, 1, "noise12"),                # 150 small strips: three workgroups of lanes
    (4, 33, 1, 4, "scene"),                    # odd widths, an odd number of bytes per strip is likely
])
def test_device_lzw_strips_equal_the_independent_coder(ctx, rows, width, spp, rps, kind):
    oip = ctx
    img = _image(kind, rows, width, spp, seed=rows * 31 + width)
    d_img = torch.from_numpy(img.view(np.int16)).cuda()
    cap = oip.tiff_lzw_worst_bytes(rows, width, spp, rps)
    d_pay = torch.full((cap,), 0xEE, dtype=torch.uint8, device="cuda")
    off, ln, total = oip.tiff_lzw_strips(d_img, rows, width, spp, rps, d_pay)
    pay = d_pay.cpu().numpy()
    nstrips = (rows + rps - 1) // rps
    assert len(off) == nstrips and off[0] == 0 and total == off[-1] + ln[-1] and total <= cap
    pos = 0
    for k in range(nstrips):
        want = _tiff.lzw_encode(_predict(img[k * rps:(k + 1) * rps], spp))
        assert off[k] % 2 == 0 and off[k] == pos + (pos & 1), k
        got = pay[int(off[k]):int(off[k] + ln[k])].tobytes()
        assert got == want, (k, len(got), len(want))
        if ln[k] % 2 and k + 1 < nstrips:
            assert pay[int(off[k] + ln[k])] == 0          # the pad byte between an odd strip and the next
        pos = int(off[k] + ln[k])
    # and the streams decode (the independent decoder) to the predictor bytes
    k = nstrips - 1
    assert _tiff.lzw_decode(pay[int(off[k]):int(off[k] + ln[k])].tobytes()) == _predict(img[k * rps:(k + 1) * rps], spp)


def test_device_lzw_rejects_bad_arguments(ctx):
    oip = ctx
    d_img = torch.zeros(64 * 4, dtype=torch.int16, device="cuda")
    d_pay = torch.zeros(16, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        oip.tiff_lzw_strips(d_img, 1, 64, 3, 1, d_pay)               # spp 3
    with pytest.raises(ValueError):
        oip.tiff_lzw_strips(d_img, 1, 64, 4, 1, d_pay)               # payload too small


def _pack(strips):
    """strips one behind the other at even offsets, as a TIFF file holds them"""
    blob, off, ln = bytearray(b"\x00" * 6), [], []              # some bytes in front: the strips need not start the buffer
    for s in strips:
        if len(blob) & 1:
            blob.append(0)
        off.append(len(blob)); ln.append(len(s))
        blob += s
    return np.frombuffer(bytes(blob), dtype=np.uint8).copy(), off, ln


@pytest.mark.parametrize("rows,width,spp,rps,kind,pred", [
    (40, 720, 4, 11, "noise12", 2),
    (6, 7500, 4, 1, "scene", 2),
    (6, 2048, 1, 3, "ramp", 2),
    (5, 1000, 4, 2, "constant", 2),            # one long run: nothing but KwKwK-style growth
    (2, 16384, 4, 1, "noise16", 1),            # no predictor; many table generations
    (130, 64, 4, 1, "noise12", 2),
    (4, 33, 1, 4, "scene", 1),
])
def test_device_lzw_decoder_reads_the_independent_coders_strips(ctx, rows, width, spp, rps, kind, pred):
    """strips written by tests/_tiff.py::lzw_encode (an independent coder) decode on the device to the image, predictor undone"""
    img = _image(kind, rows, width, spp, seed=rows * 17 + width)
    strips = []
    for k in range((rows + rps - 1) // rps):
        block = img[k * rps:(k + 1) * rps]
        strips.append(_tiff.lzw_encode(_predict(block, spp) if pred == 2 else block.astype("<u2").tobytes()))
    blob, off, ln = _pack(strips)
    d_file = torch.from_numpy(blob).cuda()
    d_img = torch.full((rows, width * spp), -1, dtype=torch.int16, device="cuda")
    ctx.tiff_lzw_decode(d_file, off, ln, rows, width, spp, rps, pred, d_img)
    assert np.array_equal(d_img.cpu().numpy().view(np.uint16), img)


def test_device_lzw_round_trip_at_product_width(ctx):
    """the device encoder's strips through the device decoder: 300 rows of a 7500 x 4 product"""
    rows, width, spp = 300, 7500, 4
    img = _image("noise12", rows, width, spp, seed=5)
    d_img = torch.from_numpy(img.view(np.int16)).cuda()
    d_pay = torch.empty(ctx.tiff_lzw_worst_bytes(rows, width, spp, 1), dtype=torch.uint8, device="cuda")
    off, ln, total = ctx.tiff_lzw_strips(d_img, rows, width, spp, 1, d_pay)
    d_back = torch.zeros_like(d_img)
    ctx.tiff_lzw_decode(d_pay, off, ln, rows, width, spp, 1, 2, d_back)
    assert torch.equal(d_back, d_img) and total < img.nbytes * 1.2


def test_device_lzw_decoder_rejects_corrupt_strips(ctx):
    """the rules of the host decoder (csrc/oip_tiff.hpp::lzw_decode): a first code >= 256, a code beyond the table and a strip that
    does not decode to its rows are errors that name the strip; a stream cut before EndOfInformation is read as far as it goes"""
    rows, width, spp = 2, 64, 1
    img = _image("ramp", rows, width, spp, seed=1)
    good = [_tiff.lzw_encode(_predict(img[k:k + 1], spp)) for k in range(rows)]

    def codes(vals, w=9):
        acc, n, out = 0, 0, bytearray()
        for v in vals:
            acc = (acc << w) | v; n += w
            while n >= 8:
                out.append((acc >> (n - 8)) & 255); n -= 8
        if n:
            out.append((acc << (8 - n)) & 255)
        return bytes(out)

    d_img = torch.zeros((rows, width), dtype=torch.int16, device="cuda")
    for bad, what in ((codes([256, 300, 257]), "bad first code"), (codes([256, 65, 400, 257]), "code beyond the table"),
                      (good[1][:len(good[1]) // 2], "decodes to"), (codes([256, 65, 66, 257]), "decodes to")):
        blob, off, ln = _pack([good[0], bad])
        with pytest.raises(RuntimeError, match=what + ".*strip 1|strip 1.*" + what):
            ctx.tiff_lzw_decode(torch.from_numpy(blob).cuda(), off, ln, rows, width, spp, 1, 2, d_img)
    blob, off, ln = _pack(good)
    with pytest.raises(ValueError):
        ctx.tiff_lzw_decode(torch.from_numpy(blob).cuda(), off, [ln[0], len(blob)], rows, width, spp, 1, 2, d_img)     # strip outside the buffer
    # a stream without EndOfInformation that carries all its bytes is fine (libtiff tolerates it)
    full = _tiff.lzw_encode(_predict(img[1:2], spp))
    blob, off, ln = _pack([good[0], full[:-1]])
    try:
        ctx.tiff_lzw_decode(torch.from_numpy(blob).cuda(), off, ln, rows, width, spp, 1, 2, d_img)
        assert np.array_equal(d_img.cpu().numpy().view(np.uint16), img)
    except RuntimeError as e:                      # (cutting the last byte may also cut the last code: then the strip is short)
        assert "decodes to" in str(e)


# ---- the coder states random data reaches only by luck (tests/_lzw_cases.py) ---------------------------------------------------
# Every case is one strip whose predictor-2 bytes put the independent coder into a named state: the end of a strip at a code-width
# boundary or at the table clear, a width change or a clear on the strip's last byte, KwKwK codes around the decoder's early width
# change.  Each test first asserts, through _tiff.lzw_trace, that its input still produces the event it is named for.


@functools.lru_cache(maxsize=None)
def _ref_strip(seed, width, spp, kind, prefix):
    """(row, its predictor-2 bytes, the independent coder's strip) of one generator at one width, computed once"""
    row = L.row_of(seed, width, spp, kind, prefix)
    data = L.predict2(row, spp)
    return row, data, _tiff.lzw_encode(data)


def _neighbourhood(case):
    """A 3-row image at the case's width: the case in the middle, above and below it the generators of the cases before and after it
    in the table (same samples per pixel), cut or continued to this width -- adjacent lanes of the wave sit in other states.
    Returns (image rows x (width * spp), the independent coder's three strips)."""
    same = [c for c in L.CASES if c[2] == case[2]]
    i = same.index(case)
    rows, strips = [], []
    for c in (same[i - 1], case, same[(i + 1) % len(same)]):
        row, data, strip = _ref_strip(c[0], case[1], c[2], c[3], c[5])
        rows.append(row); strips.append(strip)
    t = _tiff.lzw_trace(_ref_strip(case[0], case[1], case[2], case[3], case[5])[1])
    assert L.has_event(t, case[4]), "the input no longer produces %s" % case[4]
    return np.stack(rows), strips


def _device_strips(ctx, img, rows, width, spp, rps):
    """the device encoder's strips, with the layout rules every caller relies on: even offsets, a zero pad byte after an odd strip"""
    d_img = torch.from_numpy(np.ascontiguousarray(img).view(np.int16)).cuda()
    cap = ctx.tiff_lzw_worst_bytes(rows, width, spp, rps)
    d_pay = torch.full((cap,), 0xEE, dtype=torch.uint8, device="cuda")
    off, ln, total = ctx.tiff_lzw_strips(d_img, rows, width, spp, rps, d_pay)
    pay = d_pay.cpu().numpy()
    nstrips = (rows + rps - 1) // rps
    assert len(off) == nstrips and off[0] == 0 and total == off[-1] + ln[-1] and total <= cap
    pos, out = 0, []
    for k in range(nstrips):
        assert off[k] % 2 == 0 and off[k] == pos + (pos & 1), k
        out.append(pay[int(off[k]):int(off[k] + ln[k])].tobytes())
        if ln[k] % 2 and k + 1 < nstrips:
            assert pay[int(off[k] + ln[k])] == 0, k              # the pad byte between an odd strip and the next
        pos = int(off[k] + ln[k])
    return out, (d_img, d_pay, off, ln)


def _device_decode(ctx, strips, rows, width, spp, rps, pred):
    blob, off, ln = _pack(strips)
    d_img = torch.full((rows, width * spp), -1, dtype=torch.int16, device="cuda")
    ctx.tiff_lzw_decode(torch.from_numpy(blob).cuda(), off, ln, rows, width, spp, rps, pred, d_img)
    return d_img.cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("case", L.CASES, ids=L.case_id)
def test_device_encoder_at_a_named_coder_state(ctx, case):
    img, want = _neighbourhood(case)
    got, _ = _device_strips(ctx, img, 3, case[1], case[2], 1)
    for k in range(3):
        assert got[k] == want[k], (k, len(got[k]), len(want[k]))


@pytest.mark.parametrize("case", L.CASES, ids=L.case_id)
def test_device_decoder_at_a_named_coder_state(ctx, case):
    """the independent coder's strips; with predictor 2 the image is the case's row, with predictor 1 it is the row's differences:
    the same strip, the same coder states, either way"""
    img, strips = _neighbourhood(case)
    width, spp = case[1], case[2]
    assert np.array_equal(_device_decode(ctx, strips, 3, width, spp, 1, 2), img)
    diff = np.frombuffer(L.predict2(img, spp), dtype="<u2").reshape(3, -1)
    assert np.array_equal(_device_decode(ctx, strips, 3, width, spp, 1, 1), diff)


@pytest.mark.parametrize("spp", L.SPPS)
def test_device_round_trip_through_every_named_state(ctx, spp):
    """Device encoder into device decoder.  Rows of one image share a width and the cases do not, so there is one image per distinct
    width: every generator of the table at that width, one row each; the rows whose case has that width end in their state."""
    inputs = [c for c in L.distinct_inputs() if c[2] == spp]
    for c in [c for c in L.CASES if c[2] == spp]:
        assert L.has_event(_tiff.lzw_trace(_ref_strip(c[0], c[1], c[2], c[3], c[5])[1]), c[4])
    for width in sorted({c[1] for c in inputs}):
        img = np.stack([L.row_of(c[0], width, spp, c[3], c[5]) for c in inputs])
        rows = len(inputs)
        strips, (d_img, d_pay, off, ln) = _device_strips(ctx, img, rows, width, spp, 1)
        for k, c in enumerate(inputs):
            if c[1] == width:
                assert strips[k] == _ref_strip(c[0], c[1], c[2], c[3], c[5])[2], (width, k)
        d_back = torch.zeros_like(d_img)
        ctx.tiff_lzw_decode(d_pay, off, ln, rows, width, spp, 1, 2, d_back)
        assert torch.equal(d_back, d_img), width


@pytest.mark.parametrize("spp", L.SPPS)
@pytest.mark.parametrize("name", list(L.VARIANTS))
def test_device_decoder_reads_legal_streams_libtiff_never_writes(ctx, name, spp):
    """16000-byte noise strips as a foreign encoder may write them (tests/_lzw_cases.py::VARIANTS: those the independent decoder and
    libtiff read -- tests/test_tifflzw_cpu.py); libtiff's own form of the same row in the lane beside it"""
    knobs, width = L.VARIANTS[name], L.VARIANT_WIDTH[spp]
    row = L.variant_row(spp)
    data = L.predict2(row, spp)
    t = _tiff.lzw_trace(data, **knobs)
    assert L.variant_reaches_its_state(t, knobs) and _tiff.lzw_decode(t.stream) == data
    img = np.stack([row, row])
    for strips in ([_tiff.lzw_encode(data), t.stream], [t.stream, _tiff.lzw_encode(data)]):
        assert np.array_equal(_device_decode(ctx, strips, 2, width, spp, 1, 2), img)


def test_device_decoder_reports_a_table_that_fills_without_clearcode(ctx):
    """status 3: literal codes for ever and no ClearCode; the decoder's next reaches 4096 after 3839 of them (3839 bytes, less than the
    strip).  The error names that strip, whichever side of the good one it is on."""
    rows, width, spp = 2, 2048, 1
    img = _image("noise12", rows, width, spp, seed=9)
    good = [_tiff.lzw_encode(_predict(img[k:k + 1], spp)) for k in range(rows)]
    acc = nb = 0
    out = bytearray()
    w, nxt, first = 9, 258, True
    for c in [256] + [(i * 37) % 256 for i in range(6000)]:    # packed at the widths the decoder reads them with
        acc = (acc << w) | c; nb += w
        while nb >= 8:
            out.append((acc >> (nb - 8)) & 0xFF); nb -= 8
        if c == 256 or first:
            first = c == 256
        else:
            nxt += 1
            if nxt >= (1 << w) - 1 and w < 12:
                w += 1
    assert nxt > 4096 and w == 12
    bad = bytes(out)
    d_img = torch.zeros((rows, width), dtype=torch.int16, device="cuda")
    for strips, k in (([good[0], bad], 1), ([bad, good[1]], 0)):
        blob, off, ln = _pack(strips)
        with pytest.raises(RuntimeError, match="table full without ClearCode.*strip %d" % k):
            ctx.tiff_lzw_decode(torch.from_numpy(blob).cuda(), off, ln, rows, width, spp, 1, 2, d_img)
    assert np.array_equal(_device_decode(ctx, good, rows, width, spp, 1, 2), img)


def test_device_decoder_packed_predictor_add_at_full_range(ctx):
    """Predictor 2 of 4 samples is undone by four 16-bit adds in one 64-bit register: 15 bits carry on their own, the top bits go by
    xor.  Full-range samples, and 0x7FFF, 0x8000, 0xFFFF, 0x0000 side by side in every order (a sequence that holds all 16 ordered
    pairs), each channel one step further along it than the one before -- so every carry out of bit 14 meets every pair of top bits, and
    neighbouring 16-bit fields differ in it."""
    rows, width, spp = 6, 257, 4
    img = np.random.default_rng(11).integers(0, 65536, (rows, width, spp), dtype=np.uint16)
    vals = np.array([0x7FFF, 0x8000, 0xFFFF, 0x0000], dtype=np.uint16)
    seq = [0, 0, 1, 0, 2, 0, 3, 1, 1, 2, 1, 3, 2, 2, 3, 3, 0]
    assert {(a, b) for a, b in zip(seq, seq[1:])} == {(a, b) for a in range(4) for b in range(4)}
    ring = seq[:-1]
    for r in range(rows):
        for c in range(spp):
            x0 = (0, 1, 100, 239, 240 - 17, 57)[r]              # from the row's first pixel on, up to its last, in between
            n = min(len(seq) + 3, width - x0)
            img[r, x0:x0 + n, c] = vals[[ring[(i + c) % 16] for i in range(n)]]
    img = img.reshape(rows, width * spp)
    strips = [_tiff.lzw_encode(_predict(img[k:k + 1], spp)) for k in range(rows)]
    assert np.array_equal(_device_decode(ctx, strips, rows, width, spp, 1, 2), img)
    got, _ = _device_strips(ctx, img, rows, width, spp, 1)
    assert got == strips


@pytest.mark.parametrize("rows,width,spp,rps", [(3, 1, 1, 1), (3, 1, 4, 1), (1, 2, 4, 1), (5, 1, 4, 2)])
def test_device_lzw_on_tiny_strips(ctx, rows, width, spp, rps):
    """strips of 2 to 16 bytes, a one-pixel row (the 4-sample loader's look-ahead guard on its first pixel), a short last strip"""
    img = np.random.default_rng(rows * 7 + width + spp).integers(0, 65536, (rows, width * spp), dtype=np.uint16)
    want = [_tiff.lzw_encode(_predict(img[k:k + rps], spp)) for k in range(0, rows, rps)]
    got, _ = _device_strips(ctx, img, rows, width, spp, rps)
    assert got == want
    assert np.array_equal(_device_decode(ctx, want, rows, width, spp, rps, 2), img)
    plain = [_tiff.lzw_encode(img[k:k + rps].astype("<u2").tobytes()) for k in range(0, rows, rps)]
    assert np.array_equal(_device_decode(ctx, plain, rows, width, spp, rps, 1), img)


# ---- the driver around the coder: two launches, refusals before anything runs ------------------------------------------------------
@pytest.mark.parametrize("own_scratch", [True, False], ids=["own_scratch", "callers_scratch"])
def test_device_lzw_across_the_launch_boundary(ctx, own_scratch):
    """32770 one-row strips: launches of 32768 and 2 (tests/_tiff_boundary.py).  Strip 32767 is odd, so the second launch's first
    offset carries the pad byte of the first launch's last strip."""
    rows = B.rows_named(["zero", "const", "noise16", "small", "ramp"])
    streams = [_tiff.lzw_encode(B.predict2(r)) for r in rows]
    B.check_two_launches(ctx, ctx.tiff_lzw_strips, ctx.tiff_lzw_worst_bytes, ctx.tiff_lzw_scratch_bytes, rows, B.WIDTH, 1,
                         B.pattern_of_rows(len(rows)), streams, own_scratch)


def test_device_lzw_refusals_launch_nothing(ctx):
    """the twin of test_gpu_deflate_encode.py::test_refusals_launch_nothing"""
    rows, width, spp, rps = 8, 64, 4, 2
    img = _image("noise12", rows, width, spp, seed=3)
    d_img = torch.from_numpy(img.view(np.int16)).cuda()
    worst = ctx.tiff_lzw_worst_bytes(rows, width, spp, rps)
    payload = torch.full((worst,), B.PATTERN, dtype=torch.uint8, device="cuda")
    need = ctx.tiff_lzw_scratch_bytes(rows, width, spp, rps)
    scratch = torch.zeros(need, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        ctx.tiff_lzw_strips(d_img, rows, width, spp, rps, payload, payload_cap=worst - 1)
    with pytest.raises(ValueError):
        ctx.tiff_lzw_strips(d_img, rows, width, spp, rps, payload, scratch=scratch, scratch_bytes=need - 1)
    with pytest.raises(ValueError):
        ctx.tiff_lzw_strips(d_img, rows, width, 3, rps, payload)
    with pytest.raises(ValueError):
        ctx.tiff_lzw_strips(d_img, rows, 0, spp, rps, payload)
    assert ctx.tiff_lzw_worst_bytes(rows, 0, spp, rps) == 0 and ctx.tiff_lzw_scratch_bytes(0, width, spp, rps) == 0
    ctx.sync()
    assert (payload.cpu().numpy() == B.PATTERN).all()
    off, ln, total = ctx.tiff_lzw_strips(d_img, rows, width, spp, rps, payload, scratch=scratch)
    assert total > 0 and _tiff.lzw_decode(payload[:int(ln[0])].cpu().numpy().tobytes()) == _predict(img[:rps], spp)


def test_device_lzw_refuses_misaligned_scratch(ctx):
    rows, width, spp, rps = 8, 64, 4, 2
    d_img = torch.zeros(rows * width * spp, dtype=torch.int16, device="cuda")
    payload = torch.full((ctx.tiff_lzw_worst_bytes(rows, width, spp, rps),), B.PATTERN, dtype=torch.uint8, device="cuda")
    need = ctx.tiff_lzw_scratch_bytes(rows, width, spp, rps)
    scratch = torch.zeros(need + 8, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="scratch too small or misaligned"):
        ctx.tiff_lzw_strips(d_img, rows, width, spp, rps, payload, scratch=scratch[4:], scratch_bytes=need)
    ctx.sync()
    assert (payload.cpu().numpy() == B.PATTERN).all()
