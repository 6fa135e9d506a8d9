"""CPU: the Deflate decoder of csrc/oip_inflate.h in its host instantiation and the Deflate branch of read_tiff_u16
(csrc/oip_tiff.hpp), as a stand-alone program under ASan + UBSan (tests/cpp/inflate_test.cpp).  The streams are those of
tests/_deflate_cases.py: every one is first shown, by that module's own bit-level tracer, to hold what it is named for, and zlib is
asked what it makes of it.  The `oip` tools open the device before they read an input, so their Deflate runs are GPU tests
(tests/test_gpu_deflate_cli.py)."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import _deflate_cases as D
import _deflate_tiff as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = {**D.accepted(), **D.rejected(), **D.size_cases()}


@pytest.mark.parametrize("name", list(ALL))
def test_case_holds_its_event_and_zlib_agrees(name):
    D.check_event(name)
    D.check_against_zlib(name)


def test_every_rule_has_a_rejected_case():
    rules = {c.event for c in D.rejected().values()}
    assert rules == set(D.CAUSE) - {"truncated", "no code: literal/length"}      # (truncation: every prefix, below; a literal/length
    # set that leaves bits without a code is a single end-of-block code, whose other bit is the same refusal as symbol 286)
    assert {c.event for c in D.size_cases().values()} == {"size"}


def test_truncations_by_the_tracer_and_zlib():
    """every prefix of a stored + fixed + dynamic stream: the tracer refuses it, or -- from the last four bytes on -- reports the
    image and a missing trailer; zlib never returns other bytes than a prefix of the image"""
    s, out = D.truncation_stream()
    for cut in range(len(s)):
        try:
            t = D.trace(s[:cut])
            assert D.truncation_is_tolerated(cut) and t.out == out and t.trailer is False, cut
        except D.Reject as e:
            assert not D.truncation_is_tolerated(cut) and e.args[0] == "truncated", (cut, e)
        z = zlib.decompressobj()
        got = z.decompress(s[:cut])
        assert out.startswith(got) and not z.eof and (got == out) >= D.truncation_is_tolerated(cut), cut


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("inflate")
    src = os.path.join(ROOT, "tests", "cpp", "inflate_test.cpp")
    inc = os.path.join(ROOT, "opticalimageprocessor_amd", "csrc")
    exe = d / "inflate_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread", "-I" + inc,
                    src, "-o", str(exe)], check=True)
    return str(exe)


def test_host_decoder_on_cases_truncations_and_bit_flips(program, tmp_path):
    """exact-size heap buffers at every alignment: an overrun is a sanitizer report.  Accepted cases give their bytes, rejected ones the
    status of their rule; every truncation is an error or the tolerated trailer; every single-bit flip of three short streams gives a
    refusal or the bytes of the program's second, bit-by-bit decoder -- and the two decoders accept the same flips."""
    n = D.write_case_files(str(tmp_path))
    s, _ = D.truncation_stream()
    flips = 8 * (len(s) + len(D.accepted()["writer_single_distance_code"].stream) + len(T.deflate(D._text(120, 23), 6, zlib.Z_FIXED)))
    r = subprocess.run([program, "cases", str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "%d cases, %d truncations, %d flips" % (n, len(s), flips) in r.stdout and ", 0 bad" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    got = {l.split()[1]: int(l.split()[2]) for l in r.stdout.splitlines() if l.startswith("case ")}
    for name, case in D.rejected().items():
        assert got[name] == D.CAUSE[case.event][0], name


def _image(h, w, spp, seed):
    rng = np.random.default_rng(seed)
    a = (1800 + 600 * np.sin(np.arange(h * w * spp) / 37.0) + rng.integers(0, 40, h * w * spp)).astype(np.uint16)
    a[::13] = 65535
    a[::17] = 0
    return a.reshape(h, w * spp)


def test_read_tiff_u16_reads_and_refuses_deflate_files(program, tmp_path):
    d = str(tmp_path)
    lines = []

    def keep(name, img, expect=None, **kw):
        T.write(os.path.join(d, name + ".tiff"), img, **kw)
        if expect is None:
            np.ascontiguousarray(img, "<u2").tofile(os.path.join(d, name + ".raw"))
        lines.append("%s %s %s" % (os.path.join(d, name + ".tiff"), os.path.join(d, name + ".raw") if expect is None else "-",
                                   (expect or "x").replace(" ", "_")))

    k = 0
    for spp in (1, 3, 4):
        for pred in (1, 2):
            img = _image(40, 65, spp, k)
            keep("strips_%d_%d" % (spp, pred), img, spp=spp, predictor=pred, rps=11, level=(0, 1, 6, 9)[k % 4])     # a short last strip
            keep("tiles_%d_%d" % (spp, pred), img, spp=spp, predictor=pred, tile=(32, 16))
            k += 1
    keep("odd_33x1", _image(1, 33, 1, 50), spp=1, predictor=2, rps=1)                     # 66 bytes: streams of odd lengths follow
    keep("odd_33x5", _image(5, 33, 1, 51), spp=1, predictor=1, rps=2)
    keep("one_strip", _image(9, 20, 4, 52), spp=4, predictor=2)
    keep("old_number", _image(9, 20, 4, 53), spp=4, predictor=2, rps=4, compression=32946)
    keep("old_number_tiled", _image(20, 20, 1, 54), spp=1, predictor=2, tile=(16, 16), compression=32946)
    keep("fixed_blocks", _image(12, 40, 4, 55), spp=4, predictor=2, rps=5, strategy=zlib.Z_FIXED)
    for T_ in (16, 32):
        for w in (1, 15, 16, 17, 257):
            for h in (1, 15, 16, 17, 257):
                spp = 4 if (w + h + T_) % 3 == 0 else 1
                keep("t%d_%dx%d" % (T_, w, h), _image(h, w, spp, w * 1000 + h), spp=spp, predictor=1 + (w + h) % 2, tile=(T_, T_))
    # refusals
    img = _image(40, 64, 4, 60)
    keep("compression_7", img, "compression 7 is not supported (none, LZW and Deflate are)", spp=4, compression=7, rps=8)
    keep("compression_50000", img, "compression 50000 is not supported (none, LZW and Deflate are)", spp=4, compression=50000, tile=(16, 16))
    keep("predictor_3", img, "predictor 3 is not supported", spp=4, predictor=3, rps=8)
    s = T.streams_of(img, 4, 2, rps=8)
    bad = list(s)
    bad[2] = bad[2][:2] + bytes([bad[2][2] | 6]) + bad[2][3:]                             # BTYPE 3 in the first block header
    keep("corrupt_strip", img, "corrupt Deflate stream (invalid block type) in strip 2", spp=4, rps=8, streams=bad)
    bad = list(s)
    bad[4] = bad[4][:len(bad[4]) // 2]
    keep("cut_strip", img, "corrupt Deflate stream (stream ends inside a block) in strip 4", spp=4, rps=8, streams=bad)
    bad = list(s)
    bad[1] = T.deflate(T.predict2(img.reshape(40, 64, 4)[8:15]).tobytes())               # seven rows where eight belong
    keep("short_strip", img, "strip 1 decodes to 3584 bytes, 4096 expected", spp=4, rps=8, streams=bad)
    bad[1] = T.deflate(T.predict2(img.reshape(40, 64, 4)[8:17]).tobytes())
    keep("long_strip", img, "corrupt Deflate stream (more bytes than expected) in strip 1", spp=4, rps=8, streams=bad)
    bad = list(s)
    bad[3] = bad[3][:-1] + bytes([bad[3][-1] ^ 1])
    keep("adler_strip", img, "corrupt Deflate stream (Adler-32 mismatch) in strip 3", spp=4, rps=8, streams=bad)
    t = T.streams_of(img, 4, 2, tile=(32, 16))
    bad = list(t)
    bad[5] = bad[5][:len(bad[5]) // 2]
    keep("corrupt_tile", img, "corrupt Deflate stream (stream ends inside a block) in tile 5", spp=4, tile=(32, 16), streams=bad)
    # a header that promises far more than its streams can hold: refused before anything is allocated
    keep("implausible_strips", img, "image size is implausible for its compressed strips", spp=4, rps=8, streams=s[:1],
         tags_override={257: (4, 1, 3000000), 278: (4, 1, 3000000)})
    keep("implausible_tiles", img, "image size is implausible for its compressed tiles", spp=4, tile=(32, 16), streams=[t[0]] * 2,
         tags_override={322: (4, 1, 8192), 323: (4, 1, 8192), 256: (4, 1, 8192), 257: (4, 1, 16384)})
    # ... while a constant image, Deflate's best case, is far inside the bound (1032 : 1 is a match of 258 bytes for 2 bits)
    const = np.full((2000, 1000), 7, np.uint16)
    keep("constant", const, spp=1, predictor=1, rps=500)
    assert os.path.getsize(os.path.join(d, "constant.tiff")) < const.nbytes // 500
    open(os.path.join(d, "list.txt"), "w").write("\n".join(lines) + "\n")
    r = subprocess.run([program, "tiff", os.path.join(d, "list.txt")], capture_output=True, text=True)
    assert r.returncode == 0 and "%d files, 0 bad" % len(lines) in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
