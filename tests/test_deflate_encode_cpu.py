"""CPU: the Deflate encoder of csrc/oip_deflate.h in its host instantiation and the Deflate branch of the two TIFF writers
(csrc/oip_tiff.hpp, csrc/oip_tifftiled.hpp), as a stand-alone program under ASan + UBSan (tests/cpp/deflate_encode_test.cpp).
The program encodes the inputs this file writes into exact-size heap blocks and decodes every stream again with the project's own
decoder; this file inflates every stream with Python's zlib, compares it with the input, holds its size against the stored bound
n + 5 ceil(n / 65535) + 6, and asks the bit-level tracer of tests/_deflate_cases.py what the short ones are made of.  The device
runs of the same coder are GPU tests (tests/test_gpu_deflate_encode.py, tests/test_gpu_deflate_encode_cli.py)."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import _deflate_cases as D
import _deflate_write_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("deflate_encode")
    src = os.path.join(ROOT, "tests", "cpp", "deflate_encode_test.cpp")
    inc = os.path.join(ROOT, "opticalimageprocessor_amd", "csrc")
    exe = d / "deflate_encode_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread", "-I" + inc,
                    src, "-o", str(exe)], check=True)
    return str(exe)


def _fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


def _inputs():
    rng = np.random.default_rng(5)
    x = {}
    for n in list(range(301)) + [65535, 65536, 65537]:
        x["zero_%d" % n] = bytes(n)
    x["random_100000"] = rng.integers(0, 256, 100000, dtype=np.uint8).tobytes()
    x["one_value"] = b"\x11" * 3000
    x["one_value_and_another_once"] = b"\x11" * 1500 + b"\x93" + b"\x11" * 1499
    x["two_bytes"] = b"\x07\x08"
    # 24 byte values: 19 with the frequencies 1, 1, 2, 3, 5 .. 4181 and five more that occur once, in random order (10950 bytes, one
    # block): the unlimited Huffman tree of the 19 alone is 18 deep
    vals = rng.permutation(256)[:24]
    fib = np.repeat(vals, _fib(19) + [1] * 5)
    x["fibonacci_24"] = rng.permutation(fib).astype(np.uint8).tobytes()
    # many code lengths and zero runs of many sizes in the header: byte values at growing gaps, frequencies 1, 1, 2, 3, 5 ..
    vals = np.cumsum(np.arange(1, 20)) % 256
    x["header_mix"] = rng.permutation(np.repeat(vals, _fib(19))).astype(np.uint8).tobytes()
    r = rng.integers(0, 256, 16384, dtype=np.uint8).tobytes()
    x["random_16384_twice"] = r + r
    x["blocky_tile_8MiB"] = R.strip_bytes(R.blocks(1024, 1024, 4, 9, 28), 4, tile=(1024, 1024))[0]
    return x


@pytest.fixture(scope="module")
def encoded(program, tmp_path_factory):
    """{name: (input, stream)} of _inputs() and of every stream of the ratio fixtures, encoded by the program in one run"""
    d = str(tmp_path_factory.mktemp("streams"))
    x = _inputs()
    for name, (streams, _) in R.ratio_fixtures().items():
        for k, s in enumerate(streams):
            x["%s.%d" % (name, k)] = s
    for name, data in x.items():
        with open(os.path.join(d, name + ".bin"), "wb") as f:
            f.write(data)
    with open(os.path.join(d, "list.txt"), "w") as f:
        f.write("\n".join(x) + "\n")
    r = subprocess.run([program, "streams", d], capture_output=True, text=True)
    assert r.returncode == 0 and "%d streams, 0 bad" % len(x) in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    out = {}
    for name, data in x.items():
        with open(os.path.join(d, name + ".z"), "rb") as f:
            out[name] = (data, f.read())
    return out


def test_every_stream_inflates_with_zlib_and_stays_under_the_stored_bound(encoded):
    for name, (data, z) in encoded.items():
        o = zlib.decompressobj()
        assert o.decompress(z) == data and o.eof and not o.unused_data, name
        assert len(z) <= R.stored_bound(len(data)), (name, len(z))
        assert z[0] == 0x78 and (z[0] * 256 + z[1]) % 31 == 0 and not z[1] & 0x20, name           # CM 8, CINFO 7, FCHECK, no FDICT
        assert z[-4:] == zlib.adler32(data).to_bytes(4, "big"), name


def test_short_streams_hold_what_the_contract_says(encoded):
    """the tracer (which refuses what include/oip_c.h refuses: incomplete and over-subscribed sets, distances before the start)
    on every input but the 8 MiB one and the ratio fixtures"""
    for name, (data, z) in encoded.items():
        if "." in name or name == "blocky_tile_8MiB":
            continue
        t = D.trace(z)
        assert bytes(t.out) == data and t.cinfo == 7 and t.trailer is True and t.trailing == 0, name
        assert all(3 <= ln <= 258 and 1 <= dist <= 32768 and dist <= off for off, ln, dist in t.matches), name
        assert t.max_lit_len <= 15 and t.max_dist_len <= 15, name
    # runs: a literal, then matches at distance 1 of 258 and what is left (3 at n = 4, 262, ...)
    for n, want in ((3, []), (4, [3]), (259, [258]), (260, [258]), (261, [258]), (262, [258, 3]), (300, [258, 41])):
        t = D.trace(encoded["zero_%d" % n][1])
        assert [m[1] for m in t.matches] == want and all(m[2] == 1 for m in t.matches), (n, t.matches)
    for n in range(4, 301):
        assert len(encoded["zero_%d" % n][1]) <= 14, n
    # random bytes: stored blocks, merged to 65535
    t = D.trace(encoded["random_100000"][1])
    assert t.blocks == [0, 0] and t.stored_lens == [65535, 34465]
    assert len(encoded["random_100000"][1]) == R.stored_bound(100000)
    # one and two symbols: a few bytes, and sets the tracer takes for complete
    assert len(encoded["one_value"][1]) < 40 and len(encoded["one_value_and_another_once"][1]) < 48
    assert len(encoded["two_bytes"][1]) == 2 + 4 + 4 and D.trace(encoded["two_bytes"][1]).blocks == [1]      # a fixed block is the smallest
    # Fibonacci frequencies: dynamic blocks within the limit.  (Bytes this skewed repeat themselves, the matcher takes the frequent
    # values out of the literal histogram and the tree that is left is not 18 deep: that the limit ACTS is shown on the builder
    # itself, test_the_code_builder_under_both_limits.)
    for name in ("fibonacci_24", "header_mix"):
        t = D.trace(encoded[name][1])
        assert set(t.blocks) == {2} and t.max_lit_len <= 15 and {17, 18} & t.repeats, (name, t.blocks, t.max_lit_len, t.repeats)
    # the second half is found in the first: one candidate per position, 4096 slots, 16384 positions entered since -- a position's
    # candidate is still the one 16384 back with probability e^-4 = 1.8 %, so 2 rounds of 64 in 3 begin a match, which then runs to
    # 258 bytes: well over half of the second half goes out as matches at distance 16384
    data, z = encoded["random_16384_twice"]
    t = D.trace(z)
    far = sum(ln for _, ln, dist in t.matches if dist == 16384)
    assert t.max_dist == 16384 and far > 8192, (t.max_dist, far)
    assert len(z) < 16384 + 8192 + 1024


def test_the_code_builder_under_both_limits(program):
    r = subprocess.run([program, "codes"], capture_output=True, text=True)
    assert r.returncode == 0 and "codes, 0 bad" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "fibonacci 24 / 15 bits: 24 codes, longest 15" in r.stdout and "fibonacci 19 / 7 bits: 19 codes, longest 7" in r.stdout


@pytest.mark.parametrize("name", list(R.ratio_fixtures()))
def test_ratio_conditions(encoded, name):
    """conditions that keep a cop-out from passing, not quality targets: noise within 2 % of zlib's Z_HUFFMAN_ONLY streams (fixed
    codes are at 1.185 of them, stored blocks at 1.124: dynamic codes on blocks of 16 KiB or more), blocky images at half of
    them or less (zlib level 1 is at 0.09 .. 0.17; a coder without matches at 1.0)"""
    streams, factor = R.ratio_fixtures()[name]
    ours = sum(len(encoded["%s.%d" % (name, k)][1]) for k in range(len(streams)))
    ref = sum(R.huffman_only(s) for s in streams)
    print("%s: %d bytes, Z_HUFFMAN_ONLY %d, ratio %.4f (at most %.2f)" % (name, ours, ref, ours / ref, factor))
    assert ours <= factor * ref, (name, ours, ref)


def _image(h, w, spp, seed):
    rng = np.random.default_rng(seed)
    a = (1800 + 600 * np.sin(np.arange(h * w * spp) / 37.0) + rng.integers(0, 40, h * w * spp)).astype(np.uint16)
    a[::13] = 65535
    a[::17] = 0
    return a.reshape(h, w * spp)


def _halve(img, spp):
    h = img.shape[0]
    return np.ascontiguousarray(img.reshape(h, -1, spp)[::2, ::2]).reshape((h + 1) // 2, -1)


@pytest.mark.parametrize("big", [False, True])
def test_the_writers_write_deflate_files(program, tmp_path, big):
    """TiffWriterU16 (strips of 64 KiB of rows; an overview file of three levels) and TiffTiledWriterU16 (write_tiles, two levels)
    with TIFF_DEFLATE, 1 and 4 samples, classic and BigTIFF: the Python reader recovers the pixels from zlib streams behind tags
    259 = 8 and 317 = 2, and Pillow's libtiff reads the 1-sample files"""
    d = str(tmp_path)
    lines, want = [], {}
    for spp in (1, 4):
        img = _image(300, 257, spp, spp)                                       # 300 rows of 514 / 2056 bytes: 127 / 31 rows a strip
        img.astype("<u2").tofile(os.path.join(d, "in%d.raw" % spp))
        for kind, a, b in (("strips", 0, 0), ("ovr", 3, 0), ("tiles", 64, 1)):
            out = os.path.join(d, "%s%d.tiff" % (kind, spp))
            lines.append("%s %s %s 257 300 %d %d %d" % (kind, out, os.path.join(d, "in%d.raw" % spp), spp, a, b))
            if kind == "strips":
                want[out] = (spp, [img])
            elif kind == "ovr":
                l1 = _halve(img, spp)
                l2 = _halve(l1, spp)
                want[out] = (spp, [l1, l2, _halve(l2, spp)])
            else:
                want[out] = (spp, [img, _halve(img, spp)])
    with open(os.path.join(d, "list.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    env = dict(os.environ, OIP_TIFF_FORCE_BIG="1" if big else "0")
    r = subprocess.run([program, "tiff", os.path.join(d, "list.txt")], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "%d files, 0 bad" % len(lines) in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    for out, (spp, levels) in want.items():
        dirs, is_big = R.read_dirs(out)
        assert is_big == big and len(dirs) == len(levels), out
        for k, (e, lv) in enumerate(zip(dirs, levels)):
            R.assert_deflate_tags(e, spp)
            assert np.array_equal(e["img"], lv), (out, k)
            assert (e["next"] == 0) == (k == len(dirs) - 1)
            if not e["tiled"]:
                rowbytes = lv.shape[1] * 2
                assert e["tags"][278] == [min(max(65536 // rowbytes, 1), lv.shape[0])], (out, k)      # the LZW rule
            for s, c in zip(e["streams"], e["chunks"]):
                assert len(s) <= R.stored_bound(c.nbytes)
        if "tiles" in out:
            R.assert_is_deflate_cog(out, levels, spp, 64, big=big)
    if not big:                                                                # (the Pillow build at hand reads classic files)
        from PIL import Image
        for kind in ("strips", "tiles"):
            with Image.open(os.path.join(d, "%s1.tiff" % kind)) as im:
                assert im.mode in ("I;16", "I;16L") and np.array_equal(np.asarray(im).astype(np.uint16), want[os.path.join(d, "%s1.tiff" % kind)][1][0]), kind
