"""The host LZW pair of the product (csrc/oip_tiff.hpp: tiffdetail::lzw_encode_to / lzw_decode) and the reference of every LZW test
(tests/_tiff.py) at the coder states tests/_lzw_cases.py names: the end of a strip at every code-width boundary and at the table
clear, a width change or a clear on the strip's last byte, KwKwK codes around the decoder's early width change, and streams
that are legal but that libtiff's encoder never writes.  The C++ side runs in a stand-alone driver built with AddressSanitizer and
UBSan; libtiff (through Pillow) anchors the reference itself at the same states."""
import os
import subprocess

import numpy as np
import pytest

import _lzw_cases as L
import _tiff

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = L.distinct_inputs()

DRIVER = r'''
#include "oip_tiff.hpp"
#include <fstream>
#include <iostream>
#include <sstream>
// one job per line of the manifest: "enc IN OUT" or "dec IN OUT CAP"; one answer per line: the byte count, or "ERR what"
static std::vector<uint8_t> slurp(const std::string &p)
{
    std::ifstream f(p, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
int main(int, char **v)
{
    std::ifstream jobs(v[1]);
    std::string line;
    while (std::getline(jobs, line)) {
        std::istringstream s(line);
        std::string op, in, out;
        size_t cap = 0;
        s >> op >> in >> out >> cap;
        const std::vector<uint8_t> src = slurp(in);
        try {
            size_t n;
            std::unique_ptr<uint8_t[]> dst;                                   // exactly as large as promised: one byte more is an ASan report
            if (op == "enc") {
                dst.reset(new uint8_t[OIPGPU::tiffdetail::lzw_worst(src.size())]);
                n = OIPGPU::tiffdetail::lzw_encode_to(src.data(), src.size(), dst.get());
                if (n > OIPGPU::tiffdetail::lzw_worst(src.size())) { printf("ERR overrun\n"); continue; }
                std::ofstream(out, std::ios::binary).write((const char *)dst.get(), (std::streamsize)n);
            } else {
                dst.reset(new uint8_t[cap ? cap : 1]);
                n = OIPGPU::tiffdetail::lzw_decode(src.data(), src.size(), dst.get(), cap);
                std::ofstream(out, std::ios::binary).write((const char *)dst.get(), (std::streamsize)std::min(n, cap));
            }
            printf("%zu\n", n);
        } catch (const std::exception &e) { printf("ERR %s\n", e.what()); }
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """every job the tests below ask about, run once through the sanitizer build of the host coders:
    host["enc"][input key] = strip; host["dec"][(stream key, cap delta)] = (count returned, bytes written)"""
    d = tmp_path_factory.mktemp("lzw")
    (d / "t.cpp").write_text(DRIVER)
    exe = d / "t"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
                    "-I", os.path.join(ROOT, "opticalimageprocessor_amd", "csrc"), str(d / "t.cpp"), "-o", str(exe)], check=True)
    jobs, names = [], []

    def job(op, key, payload, cap=0):
        i = len(jobs)
        (d / ("in%d" % i)).write_bytes(payload)
        jobs.append("%s %s %s %d" % (op, d / ("in%d" % i), d / ("out%d" % i), cap))
        names.append((op, key))

    for c in INPUTS:
        data = L.case_bytes(c)
        job("enc", L.input_key(c), data)
        for delta in (0, -1, 1):
            job("dec", (L.input_key(c), delta), _tiff.lzw_encode(data), len(data) + delta)
    for spp in L.SPPS:
        data = L.predict2(L.variant_row(spp), spp)
        for name, knobs in L.VARIANTS.items():
            for delta in (0, -1, 1):
                job("dec", ((name, spp), delta), _tiff.lzw_encode_variant(data, **knobs), len(data) + delta)
    for n in (0, 1, 2):                                        # the shortest strips there are
        job("enc", "tiny%d" % n, bytes([7, 7][:n]))
    (d / "jobs").write_text("\n".join(jobs) + "\n")
    r = subprocess.run([str(exe), str(d / "jobs")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]                # the sanitizers report nothing
    answers = r.stdout.split("\n")[:-1]
    assert len(answers) == len(jobs)
    res = {"enc": {}, "dec": {}}
    for i, ((op, key), a) in enumerate(zip(names, answers)):
        res[op][key] = (a, b"") if a.startswith("ERR") else (int(a), (d / ("out%d" % i)).read_bytes())   # an ERR fails the test that asks
    return res


def test_the_table_has_a_case_for_every_target():
    assert {(c[4], c[2]) for c in L.CASES} == {(e, s) for e in L.EVENTS for s in L.SPPS} and len(L.CASES) == len(L.EVENTS) * len(L.SPPS)


@pytest.mark.parametrize("case", L.CASES, ids=L.case_id)
def test_case_produces_its_event_and_the_trace_is_the_encoder(case):
    data = L.case_bytes(case)
    t = _tiff.lzw_trace(data)
    assert L.has_event(t, case[4])
    assert t.stream == _tiff.lzw_encode(data) and _tiff.lzw_decode(t.stream) == data
    # the trace's own bookkeeping: the code widths are what a decoder, one entry behind, reads them with
    assert [c[0] for c in t.codes].count(256) == len(t.clears) and t.codes[-1][:2] == (257, t.eoi_width)


@pytest.mark.parametrize("case", L.CASES, ids=L.case_id)
def test_host_encoder_equals_the_independent_coder(host, case):
    data = L.case_bytes(case)
    assert L.has_event(_tiff.lzw_trace(data), case[4])
    n, strip = host["enc"][L.input_key(case)]
    assert n == len(strip) and strip == _tiff.lzw_encode(data)


def test_host_encoder_on_the_shortest_strips(host):
    for n in (0, 1, 2):
        assert host["enc"]["tiny%d" % n][1] == _tiff.lzw_encode(bytes([7, 7][:n]))


def _check_decode(host, key, data):
    for delta in (0, -1, 1):                                   # cap exact, one byte short (the count still says so), one byte long
        n, got = host["dec"][(key, delta)]
        assert n == len(data), (key, delta, n)
        assert got == data[:len(data) + min(delta, 0)], (key, delta)


@pytest.mark.parametrize("case", L.CASES, ids=L.case_id)
def test_host_decoder_returns_the_input(host, case):
    data = L.case_bytes(case)
    assert L.has_event(_tiff.lzw_trace(data), case[4])
    _check_decode(host, L.input_key(case), data)


@pytest.mark.parametrize("spp", L.SPPS)
@pytest.mark.parametrize("name", list(L.VARIANTS))
def test_foreign_variant_is_legal_and_the_host_decoder_reads_it(host, tmp_path, name, spp):
    """a variant is in the table only if the reference decoder and libtiff read it; then the host decoder must"""
    Image = pytest.importorskip("PIL.Image")
    knobs = L.VARIANTS[name]
    data = L.predict2(L.variant_row(spp), spp)
    t = _tiff.lzw_trace(data, **knobs)
    assert L.variant_reaches_its_state(t, knobs) and t.stream != _tiff.lzw_encode(data)
    assert _tiff.lzw_decode(t.stream) == data
    p = str(tmp_path / "v.tiff")                               # the bytes as one row of 16-bit gray, no predictor
    _tiff.write_tiff_lzw_strips(p, [t.stream], (1, len(data) // 2, 1), 1, 1)
    with Image.open(p) as im:
        assert np.asarray(im).astype("<u2").tobytes() == data
    _check_decode(host, (name, spp), data)


@pytest.mark.parametrize("case", [c for c in L.CASES if c[2] == 1], ids=L.case_id)
def test_libtiff_writes_what_the_reference_writes(host, tmp_path, case):
    """The anchor: at every state of the table libtiff's own encoder (Pillow, compression tiff_lzw) writes the strip
    _tiff.lzw_encode writes, with predictor 2 on the row and with predictor 1 on the row's differences -- the same bytes into the
    coder either way -- and libtiff reads a file around the host encoder's strip."""
    Image = pytest.importorskip("PIL.Image")
    row = L.case_row(case).reshape(1, -1)
    data = L.case_bytes(case)
    assert L.has_event(_tiff.lzw_trace(data), case[4])
    want = _tiff.lzw_encode(data)
    diff = np.frombuffer(data, dtype="<u2").reshape(1, -1)
    for pred, img in ((2, row), (1, diff)):
        p = str(tmp_path / ("pil%d.tiff" % pred))
        Image.fromarray(img.astype(np.uint16)).save(p, compression="tiff_lzw", tiffinfo={317: pred})
        tags = _tiff.read_tags(p)
        assert tags[259] == [5] and tags.get(317, [1]) == [pred] and len(tags[273]) == 1
        with open(p, "rb") as f:
            buf = f.read()
        assert buf[tags[273][0]:tags[273][0] + tags[279][0]] == want, pred
    key = L.input_key(case)
    p = str(tmp_path / "ours.tiff")
    _tiff.write_tiff_lzw_strips(p, [host["enc"][key][1]], (1, row.shape[1], 1), 2, 1)
    with Image.open(p) as im:
        assert np.array_equal(np.asarray(im), row)
