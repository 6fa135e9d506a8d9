"""The device Deflate decoder (csrc/tiffdeflate.hip, oip_tiff_deflate_decode_u16: a zlib stream per wave, the decoder of
csrc/oip_inflate.h) against zlib and against the streams of tests/_deflate_cases.py, each of which is first shown by that module's
bit-level tracer to hold what it is named for.  The corrupt streams are refusals of a decoder whose reads and writes are bounded by
construction (the host build of the same code has been through them under ASan + UBSan: tests/test_deflate_cpu.py)."""
import zlib

import numpy as np
import pytest
import torch

import _deflate_cases as D
import _deflate_tiff as T

pytestmark = pytest.mark.gpu

GUARD = 4096            # samples behind the image, pre-filled, that no decode may touch
PATTERN = 0x5A3C


def _image(kind, rows, width, spp, seed):
    rng = np.random.default_rng(seed)
    n = rows * width * spp
    if kind == "noise12":
        a = np.clip(rng.normal(1800.0, 300.0, n), 64, 4095).astype(np.uint16)
    elif kind == "noise16":
        a = rng.integers(0, 65536, n, dtype=np.uint16)
    elif kind == "ramp":
        a = (np.arange(n, dtype=np.uint64) * 3 % 65536).astype(np.uint16)
    elif kind == "constant":
        a = np.full(n, 4242, dtype=np.uint16)
    else:
        x = np.arange(n, dtype=np.float64)
        a = (2000 + 800 * np.sin(x / 977.0) + rng.integers(0, 4, n)).astype(np.uint16)
    return a.reshape(rows, width * spp)


def _decode(ctx, streams, rows, width, spp, rps, pred):
    """-> (the image as decoded, the guard behind it, the error or None)"""
    blob, off, ln = D.pack(streams)
    n = rows * width * spp
    buf = torch.full((n + GUARD,), PATTERN, dtype=torch.int16, device="cuda")
    err = None
    try:
        ctx.tiff_deflate_decode(torch.from_numpy(blob).cuda(), off, ln, rows, width, spp, rps, pred, buf[:n])
    except RuntimeError as e:
        err = e
    host = buf.cpu().numpy().view(np.uint16)
    return host[:n].reshape(rows, width * spp), host[n:], err


@pytest.mark.parametrize("name", list(D.accepted()))
def test_accepted_case_decodes_to_what_zlib_gives(ctx, name):
    """the case as the middle one of three strips of its size (the neighbours: its bytes reversed, stored and compressed)"""
    D.check_event(name)
    D.check_against_zlib(name)
    case = D.accepted()[name]
    want = zlib.decompressobj().decompress(case.stream)
    assert want == case.out
    rev = case.out[::-1]
    streams = [T.deflate(rev, 0), case.stream, T.deflate(rev, 6)]
    img, guard, err = _decode(ctx, streams, 3, len(want) // 2, 1, 1, 1)
    assert err is None, err
    assert img[1].astype("<u2").tobytes() == want and img[0].astype("<u2").tobytes() == rev and img[2].astype("<u2").tobytes() == rev
    assert (guard == PATTERN).all()


@pytest.mark.parametrize("rows,width,spp,rps,kind", [
    (40, 720, 4, 11, None),                    # 63 KB strips of 11 rows, the last one short
    (6, 7500, 4, 1, None),                     # the product's own strips: one 60000-byte row each
    (6, 2048, 1, 3, None),                     # one sample per pixel
    (5, 1000, 4, 2, "constant"),
    (2, 16384, 4, 1, "noise16"),               # 128 KB streams: four times round the 32 KB ring
    (4, 33, 1, 4, None),                       # odd widths, streams of odd lengths
])
def test_images_at_every_level_and_predictor(ctx, rows, width, spp, rps, kind):
    """every kind of image (where the shape does not name one), predictor 1 and 2, zlib levels 0, 1, 6, 9 and Z_FIXED: stored blocks
    that split at 65535, fixed and dynamic codes, few and many matches"""
    kinds = [kind] if kind else ["noise12", "scene", "ramp", "constant", "noise16"]
    levels = [(0, zlib.Z_DEFAULT_STRATEGY), (1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED)]
    k = 0
    for kd in kinds:
        img = _image(kd, rows, width, spp, seed=rows * 17 + width)
        for pred in (1, 2):
            for level, strategy in levels if len(kinds) == 1 else [levels[(k + j) % 5] for j in range(2)]:
                streams = T.streams_of(img, spp, pred, rps=rps, level=level, strategy=strategy)
                got, guard, err = _decode(ctx, streams, rows, width, spp, rps, pred)
                assert err is None, (kd, pred, level, err)
                assert np.array_equal(got, img), (kd, pred, level, strategy)
                assert (guard == PATTERN).all()
            k += 1


def test_more_streams_than_waves_and_one_corrupt_in_the_middle(ctx):
    """300 strips of 64 x 4: more single-wave workgroups than a first wave-front of the grid holds per CU; strip 150 is cut short"""
    rows, width, spp = 300, 64, 4
    img = _image("noise12", rows, width, spp, seed=3)
    streams = T.streams_of(img, spp, 2, rps=1)
    got, guard, err = _decode(ctx, streams, rows, width, spp, 1, 2)
    assert err is None and np.array_equal(got, img) and (guard == PATTERN).all()
    bad = list(streams)
    bad[150] = bad[150][:len(bad[150]) // 2]
    got, guard, err = _decode(ctx, bad, rows, width, spp, 1, 2)
    assert err is not None and "strip 150" in str(err) and "stream ends inside a block" in str(err), err
    keep = np.arange(rows) != 150
    assert np.array_equal(got[keep], img[keep]) and (guard == PATTERN).all()
    # and more workgroups than the whole device holds at once (four a CU)
    rows = 1300
    img = _image("scene", rows, width, spp, seed=4)
    got, guard, err = _decode(ctx, T.streams_of(img, spp, 2, rps=1), rows, width, spp, 1, 2)
    assert err is None and np.array_equal(got, img) and (guard == PATTERN).all()


_GOOD = bytes(np.random.default_rng(8).integers(0, 256, 128, dtype=np.uint8))


@pytest.mark.parametrize("name", list(D.rejected()) + list(D.size_cases()))
def test_rejected_case_is_refused_with_its_strip_and_cause(ctx, name):
    """[good, the case, good] as three strips: the error names strip 1 and the rule; strips 0 and 2 are decoded, and nothing is written
    outside the image"""
    D.check_event(name)
    D.check_against_zlib(name)
    case = {**D.rejected(), **D.size_cases()}[name]
    cap = case.cap
    good = (_GOOD * (cap // 128 + 1))[:cap]
    streams = [T.deflate(good, 6), case.stream, T.deflate(good, 0)]
    img, guard, err = _decode(ctx, streams, 3, cap // 2, 1, 1, 1)
    assert err is not None, name
    if case.event == "size":
        assert ("strip 1 decodes to 400 bytes, %d expected" % cap if cap > 400 else "more bytes than expected") in str(err), err
    else:
        assert D.CAUSE[case.event][1] in str(err), err
    assert "strip 1" in str(err), err
    assert img[0].astype("<u2").tobytes() == good and img[2].astype("<u2").tobytes() == good
    assert (guard == PATTERN).all()


def test_truncations_on_the_device(ctx):
    """every eighth prefix of the stored + fixed + dynamic stream, and the last six: an error that names the strip, or -- where only the
    trailer is cut -- the image"""
    s, out = D.truncation_stream()
    cuts = sorted(set(range(0, len(s), 8)) | set(range(len(s) - 6, len(s))))
    good = T.deflate(out[::-1], 6)
    for cut in cuts:
        img, guard, err = _decode(ctx, [good, s[:cut], good], 3, len(out) // 2, 1, 1, 1)
        if D.truncation_is_tolerated(cut):
            assert err is None and img[1].astype("<u2").tobytes() == out, cut
        else:
            assert err is not None and "strip 1" in str(err) and ("stream ends inside a block" in str(err) or "bad zlib header" in str(err)), (cut, err)
        assert img[0].astype("<u2").tobytes() == out[::-1] and img[2].astype("<u2").tobytes() == out[::-1] and (guard == PATTERN).all(), cut


def test_predictor_2_of_a_refused_strip_leaves_the_neighbours_right(ctx):
    rows, width, spp = 6, 257, 4
    img = np.random.default_rng(11).integers(0, 65536, (rows, width * spp), dtype=np.uint16)
    streams = T.streams_of(img, spp, 2, rps=2)
    got, guard, err = _decode(ctx, streams, rows, width, spp, 2, 2)
    assert err is None and np.array_equal(got, img)
    streams[1] = streams[1][:-1] + bytes([streams[1][-1] ^ 0x80])
    got, guard, err = _decode(ctx, streams, rows, width, spp, 2, 2)
    assert err is not None and "Adler-32 mismatch" in str(err) and "strip 1" in str(err)
    assert np.array_equal(got[:2], img[:2]) and np.array_equal(got[4:], img[4:]) and (guard == PATTERN).all()


def test_other_sample_counts_and_a_one_pixel_row(ctx):
    for rows, width, spp, rps in ((5, 37, 3, 2), (3, 1, 4, 1), (4, 70, 2, 4), (3, 1, 1, 2)):
        img = np.random.default_rng(rows + width).integers(0, 65536, (rows, width * spp), dtype=np.uint16)
        for pred in (1, 2):
            got, guard, err = _decode(ctx, T.streams_of(img, spp, pred, rps=rps), rows, width, spp, rps, pred)
            assert err is None and np.array_equal(got, img) and (guard == PATTERN).all(), (rows, width, spp, pred)


def test_bad_arguments(ctx):
    rows, width, spp = 2, 64, 1
    img = _image("ramp", rows, width, spp, seed=1)
    streams = T.streams_of(img, spp, 2, rps=1)
    blob, off, ln = D.pack(streams)
    d_file = torch.from_numpy(blob).cuda()
    d_img = torch.zeros((rows, width), dtype=torch.int16, device="cuda")
    with pytest.raises(ValueError):
        ctx.tiff_deflate_decode(d_file, off, [ln[0], len(blob)], rows, width, spp, 1, 2, d_img)      # strip outside the buffer
    with pytest.raises(ValueError):
        ctx.tiff_deflate_decode(d_file, off, ln, rows, width, spp, 2, 2, d_img)                      # strip count against RowsPerStrip
    with pytest.raises(ValueError):
        ctx.tiff_deflate_decode(d_file, off, ln, rows, width, spp, 1, 3, d_img)                      # predictor
    with pytest.raises(ValueError):
        ctx.tiff_deflate_decode(d_file, off, ln, rows, 0, spp, 1, 2, d_img)
    ctx.tiff_deflate_decode(d_file, off, ln, rows, width, spp, 1, 2, d_img)
    assert np.array_equal(d_img.cpu().numpy().view(np.uint16), img)
