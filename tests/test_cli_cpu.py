"""CPU suite, part 4: the `oip` command line -- flag validation and exit codes of main.cpp:92-343
(no GPU is touched before the arguments are accepted)."""
import os
import platform
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OIP = os.path.join(ROOT, "opticalimageprocessor_amd", "lib", "oip")


def run(args, cwd):
    env = dict(os.environ, LOGFILE=os.path.join(cwd, "oip.log"))
    return subprocess.run([OIP] + args, cwd=cwd, env=env, capture_output=True, text=True)


@pytest.fixture()
def files(tmp_path):
    for n in ("a.raw", "b.raw", "c.tiff", "k.csv"):
        (tmp_path / n).write_bytes(b"\0" * 64)
    return str(tmp_path)


def test_cli_is_built():
    assert os.path.exists(OIP), "run __graft_entry__.build()"


def test_version_and_help(files):
    r = run(["--version"], files)
    assert r.stdout.strip() == "1.1" and r.returncode == 255            # CLI::Success + 255 (main.cpp:262-263)
    assert run(["-h"], files).returncode == 255


def test_required_and_validation_errors(files):
    assert run(["stitch", "--image1", "a.raw"], files).returncode == 106                        # RequiredError
    assert run(["stitch", "--image1", "a.raw", "--image2", "b.raw", "-c", "1"], files).returncode == 105   # fold-cols >= 2
    assert run(["prestitch", "--pan1", "a.raw", "--pan2", "missing.raw"], files).returncode == 105          # ExistingFile
    assert run(["prestitch", "--pan1", "a.raw", "--pan2", "b.raw", "--stitch-overlap", "200", "-e", "101"], files).returncode == 105
    assert run(["--pan", "a.raw", "--mss", "b.raw", "--ibc-threshold", "1.0", "--no-rrc4mss"], files).returncode == 105
    assert run(["stitch", "--bogus"], files).returncode == 109                                  # ExtrasError
    assert run(["prestitch", "--pan1", "a.raw", "--pan2", "b.raw", "-s", "x"], files).returncode == 104     # ConversionError


def test_usage_errors_exit_254(files):
    r = run(["--pan", "a.raw", "--mss", "b.raw", "--do-rrc4pan"], files)
    assert r.returncode == 254 and "USAGE ERROR: RRC parameter file of PAN needed." in r.stdout           # main.cpp:290-292
    r = run(["--pan", "a.raw", "--mss", "b.raw", "--rrc-msb1", "k.csv"], files)
    assert r.returncode == 254 and "all MSS Bands" in r.stdout                                             # main.cpp:293-299


def test_runtime_errors_exit_2(files):
    r = run(["stitch", "--image1", "a.raw", "--image2", "c.tiff", "-c", "100"], files)
    assert r.returncode == 2 and "two images should be same type" in r.stdout                              # stitcher.h:31-33
    r = run(["prestitch", "--pan1", "a.raw", "--pan2", "b.raw"], files)
    assert r.returncode == 2 and "too small for SECTION" in r.stdout                                       # stitcher.h:61-63
    # PAN must be 4x the MSS size (preproc.h:565-567)
    r = run(["--pan", "a.raw", "--mss", "b.raw", "--no-rrc4mss"], files)
    assert r.returncode == 2 and "PAN file size does not match MSS file size" in r.stdout


def _tiff_tool(tmp_path):
    """tiny driver around csrc/oip_tiff.hpp: `t write OUT W H SPP COMP` (deterministic content) and
    `t read IN RAWOUT [REWRITE COMP]`"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "t.cpp"
    src.write_text('#include "oip_tiff.hpp"\n#include <cstdlib>\n#include <cstring>\n#include <vector>\n'
                   'int main(int c, char** v){try{if(!strcmp(v[1],"write")){int w=atoi(v[3]);long h=atol(v[4]);int s=atoi(v[5]);int comp=atoi(v[6]);'
                   'std::vector<uint16_t> d((size_t)w*h*s);for(size_t i=0;i<d.size();++i)d[i]=(uint16_t)((i*2654435761u>>7)&(comp==5?0x0fff:0xffff));'
                   'OIPGPU::write_tiff_u16(v[2],d.data(),w,h,s,s==4,comp);return 0;}'
                   'int w,s;long h;std::vector<uint16_t> d;OIPGPU::read_tiff_u16(v[2],&w,&h,&s,&d);'
                   'if(c>5){OIPGPU::write_tiff_u16(v[4],d.data(),w,h,s,false,atoi(v[5]));}'
                   'FILE*f=fopen(v[3],"wb");fwrite(d.data(),2,d.size(),f);fclose(f);printf("%d %ld %d\\n",w,h,s);return 0;}'
                   'catch(std::exception&e){printf("ERR %s\\n",e.what());return 3;}}\n')
    exe = tmp_path / "t"
    # AddressSanitizer + UBSan on the CPU build (sanitizers are not available on the GPU pool): every malformed-input
    # case below must end in a clean ERR, not in an out-of-bounds access
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
                    "-I", os.path.join(root, "opticalimageprocessor_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    return exe


@pytest.mark.parametrize("comp", [1, 5])
def test_tiff_writer_roundtrip(tmp_path, comp):
    """csrc/oip_tiff.hpp writer: classic TIFF, 1 and 4 samples, odd sizes, many strips; uncompressed and LZW with the
    horizontal predictor (what cv::imwrite and the reference's GDAL call produce).  Checked by the independent
    Python decoder of tests/_tiff.py and, for 1-band files, by Pillow (libtiff)."""
    import numpy as np
    import _tiff
    exe = _tiff_tool(tmp_path)
    for w, h, spp in [(7, 5, 1), (1001, 333, 4), (3000, 3000, 1), (7500, 700, 4)]:
        if comp == 5 and w * h * spp > 300_000:
            h = max(1, 300_000 // (w * spp))                # the Python LZW decoder is slow
        out = tmp_path / ("o_%d_%d_%d.tiff" % (w, h, spp))
        subprocess.run([str(exe), "write", str(out), str(w), str(h), str(spp), str(comp)], check=True)
        img, tags, big = _tiff.read_tiff_u16(str(out))
        assert tags[259] == [comp] and tags.get(317, [1]) == ([2] if comp == 5 else [1])
        n = w * h * spp
        want = (((np.arange(n, dtype=np.uint64) * 2654435761 % (1 << 32)) >> 7) & (0x0fff if comp == 5 else 0xffff)).astype(np.uint16)
        want = want.reshape(h, w, spp) if spp > 1 else want.reshape(h, w)
        if spp == 4:
            want = want[:, :, [2, 1, 0, 3]]
        assert not big and np.array_equal(img, want), (w, h, spp)
        if comp == 5 and n > 100000:
            assert os.path.getsize(out) < n * 2                     # it did compress the 12-bit data
        if spp == 1:
            from PIL import Image
            with Image.open(str(out)) as im:
                assert np.array_equal(np.asarray(im), want)


def test_tiff_writer_bigtiff_hook(tmp_path):
    """BigTIFF layout (what products past 4 GiB get) at a small size through the OIP_TIFF_FORCE_BIG test hook: both encodings, read
    by the independent Python reader and by the product's own reader"""
    import numpy as np
    import _tiff
    exe = _tiff_tool(tmp_path)
    env = dict(os.environ, OIP_TIFF_FORCE_BIG="1")
    for comp in (1, 5):
        w, h, spp = 301, 97, 4
        out = tmp_path / ("big_%d.tiff" % comp)
        subprocess.run([str(exe), "write", str(out), str(w), str(h), str(spp), str(comp)], check=True, env=env)
        img, tags, big = _tiff.read_tiff_u16(str(out))
        n = w * h * spp
        want = (((np.arange(n, dtype=np.uint64) * 2654435761 % (1 << 32)) >> 7) & (0x0fff if comp == 5 else 0xffff)).astype(np.uint16)
        want = want.reshape(h, w, spp)[:, :, [2, 1, 0, 3]]
        assert big and tags[259] == [comp] and np.array_equal(img, want)
        raw = tmp_path / "back.raw"
        r = subprocess.run([str(exe), "read", str(out), str(raw)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.split() == [str(w), str(h), str(spp)]
        assert np.array_equal(np.fromfile(str(raw), np.uint16).reshape(h, w, spp), want)


def test_tiff_reader(tmp_path):
    """oip_tiff.hpp reader: its own files (both compressions), foreign uncompressed files, LZW files written by Pillow
    (libtiff; predictor 1 and 2) and by the independent Python encoder (4 samples, predictor 2, one row per strip
    like cv::imwrite writes wide images); malformed headers fail cleanly."""
    import numpy as np
    import _tiff
    from PIL import Image
    exe = _tiff_tool(tmp_path)
    rng = np.random.default_rng(3)
    for shape in [(5, 7), (333, 1001, 4), (900, 7500, 4)]:
        a = rng.integers(0, 65536, shape).astype(np.uint16)
        p = tmp_path / "in.tiff"
        _tiff.write_tiff_u16(str(p), a)
        for comp in (1, 5):
            r = subprocess.run([str(exe), "read", str(p), str(tmp_path / "o.raw"), str(tmp_path / "rt.tiff"), str(comp)], capture_output=True, text=True)
            assert r.returncode == 0, r.stdout
            w, h, s = map(int, r.stdout.split())
            assert (h, w) == shape[:2] and s == (shape[2] if len(shape) == 3 else 1)
            assert np.array_equal(np.fromfile(tmp_path / "o.raw", np.uint16).reshape(shape), a)
            # written again by the C++ writer (many strips for the large case) and read back by the C++ reader
            r = subprocess.run([str(exe), "read", str(tmp_path / "rt.tiff"), str(tmp_path / "o2.raw")], capture_output=True, text=True)
            assert r.returncode == 0 and np.array_equal(np.fromfile(tmp_path / "o2.raw", np.uint16).reshape(shape), a)
            if comp == 1 or a.size < 200000:
                back, _, _ = _tiff.read_tiff_u16(str(tmp_path / "rt.tiff"))
                assert np.array_equal(back.reshape(shape), a)
    # Pillow (libtiff) writes 16-bit gray: uncompressed, LZW, LZW + horizontal predictor
    g = (rng.integers(0, 4096, (240, 500)) + np.arange(500) * 3).astype(np.uint16)
    for name, kw in (("pil.tiff", {}), ("lzw.tiff", {"compression": "tiff_lzw"}),
                     ("lzwp.tiff", {"compression": "tiff_lzw", "tiffinfo": {317: 2}})):
        Image.fromarray(g).save(str(tmp_path / name), **kw)
        r = subprocess.run([str(exe), "read", str(tmp_path / name), str(tmp_path / "o3.raw")], capture_output=True, text=True)
        assert r.returncode == 0, (name, r.stdout)
        assert np.array_equal(np.fromfile(tmp_path / "o3.raw", np.uint16).reshape(g.shape), g), name
    # what cv::imwrite produces for an ALIGNED image: 4 samples, LZW, predictor 2, a handful of rows per strip
    a4 = (rng.integers(0, 4096, (37, 411, 4)) + np.arange(411)[None, :, None]).astype(np.uint16)
    for pred, rps in ((2, 1), (2, 5), (1, 37)):
        _tiff.write_tiff_u16(str(tmp_path / "cv.tiff"), a4, lzw=True, predictor=pred, rows_per_strip=rps)
        r = subprocess.run([str(exe), "read", str(tmp_path / "cv.tiff"), str(tmp_path / "o4.raw")], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout
        assert np.array_equal(np.fromfile(tmp_path / "o4.raw", np.uint16).reshape(a4.shape), a4), (pred, rps)
    # long runs force the 12-bit table to fill and clear several times
    flat = np.zeros((24, 4096), np.uint16); flat[::7] = 4095; flat[:, ::501] = 17
    _tiff.write_tiff_u16(str(tmp_path / "runs.tiff"), flat, lzw=True, predictor=1, rows_per_strip=24)
    r = subprocess.run([str(exe), "read", str(tmp_path / "runs.tiff"), str(tmp_path / "o5.raw"), str(tmp_path / "runs2.tiff"), "5"], capture_output=True, text=True)
    assert r.returncode == 0 and np.array_equal(np.fromfile(tmp_path / "o5.raw", np.uint16).reshape(flat.shape), flat)
    with Image.open(str(tmp_path / "runs2.tiff")) as im:           # the C++ LZW stream through libtiff
        assert np.array_equal(np.asarray(im), flat)
    # malformed input: clean failures, no crash
    (tmp_path / "bad.tiff").write_bytes(b"not a tiff at all")
    good = (tmp_path / "pil.tiff").read_bytes()
    import struct
    ifd = struct.unpack_from("<I", good, 4)[0]
    nent = struct.unpack_from("<H", good, ifd)[0]

    def patched(tag, field_off, fmt, value):
        b = bytearray(good)
        for i in range(nent):
            o = ifd + 2 + 12 * i
            if struct.unpack_from("<H", b, o)[0] == tag:
                struct.pack_into(fmt, b, o + field_off, value)
        return bytes(b)

    cases = {"bad.tiff": b"not a tiff at all",
             "hugecount.tiff": patched(279, 4, "<I", 0xFFFFFFFF),         # StripByteCounts count
             "hugelen.tiff": patched(279, 8, "<I", 0xFFFFFFF0),           # a strip longer than the file
             "hugew.tiff": patched(256, 8, "<I", 0xFFFFFFFF),             # width that overflows the image size
             "zerocount.tiff": patched(273, 4, "<I", 0),                  # tag with count 0
             "trunc.tiff": good[: len(good) // 2]}
    # corrupt LZW payloads behind a valid header (one strip, 64 x 64 gray): a stream that fills the code table without ever
    # sending ClearCode (Clear, then 6000 literal 9..12-bit codes -- used to write past the decoder's 4096-entry tables),
    # random bytes, a truncated stream, and a tiny file whose header claims a 2^40-byte image
    def lzw_file(payload, w=64, h=64):
        tags = [(256, 4, 1, w), (257, 4, 1, h), (258, 3, 1, 16), (259, 3, 1, 5), (262, 3, 1, 1), (273, 4, 1, 8 + 2 + 12 * 10 + 4),
                (277, 3, 1, 1), (278, 4, 1, h), (279, 4, 1, len(payload)), (339, 3, 1, 1)]
        b = struct.pack("<2sHI", b"II", 42, 8) + struct.pack("<H", len(tags))
        for t in tags:
            b += struct.pack("<HHII", *t)
        return b + struct.pack("<I", 0) + payload

    def pack_codes(codes):
        acc = nb = 0
        out = bytearray()
        width, nxt, first = 9, 258, True
        for c in codes:
            acc = (acc << width) | c; nb += width
            while nb >= 8:
                out.append((acc >> (nb - 8)) & 0xFF); nb -= 8
            if c == 256:
                width, nxt, first = 9, 258, True
            elif first:
                first = False                        # the first code after Clear adds no table entry
            else:
                nxt += 1
                if nxt >= (1 << width) - 1 and width < 12:
                    width += 1
        if nb:
            out.append((acc << (8 - nb)) & 0xFF)
        return bytes(out)
    noclear = pack_codes([256] + [(i * 37) % 256 for i in range(6000)])
    good_payload = _tiff.lzw_encode((np.arange(4096) % 700).astype("<u2").tobytes())
    cases.update({"noclear.tiff": lzw_file(noclear),
                  "garbage.tiff": lzw_file(bytes(rng.integers(0, 256, 5000, dtype=np.uint8))),
                  "lzwtrunc.tiff": lzw_file(good_payload[: len(good_payload) // 2]),
                  "claims_huge.tiff": lzw_file(b"\x80\x00\x20\x20", w=1 << 20, h=1 << 19)})
    # the healthy payload behind the same hand-made header decodes (the header builder itself is sound)
    (tmp_path / "ok64.tiff").write_bytes(lzw_file(good_payload))
    r = subprocess.run([str(exe), "read", str(tmp_path / "ok64.tiff"), str(tmp_path / "o7.raw")], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    assert np.array_equal(np.fromfile(tmp_path / "o7.raw", np.uint16), (np.arange(4096) % 700).astype(np.uint16))
    for name, data in cases.items():
        (tmp_path / name).write_bytes(data)
        r = subprocess.run([str(exe), "read", str(tmp_path / name), str(tmp_path / "o6.raw")], capture_output=True, text=True)
        assert r.returncode == 3 and r.stdout.startswith("ERR"), (name, r.returncode, r.stdout, r.stderr[-2000:])


def test_task_subcommand_argument_errors(files):
    """`oip task` (fused flow of DOC/sample-task.sh): argument checking happens before any device use"""
    r = run(["task", "--pan1", "a.raw"], files)
    assert r.returncode == 106 and "is required" in r.stderr
    base = ["task", "--pan1", "a.raw", "--pan2", "b.raw", "--rrc1", "k.csv", "--rrc2", "k.csv", "--mss1", "a.raw", "--mss2", "b.raw",
            "--out-pan", "p.TIFF", "--out-mss", "m.TIFF"]
    for c in (1, 2):
        for b in range(1, 5):
            base += ["--rrc-mss%d-b%d" % (c, b), "k.csv"]
    r = run(base + ["--fold-cols-pan", "1", "--fold-cols-mss", "12"], files)
    assert r.returncode == 105 and "fold column value too small" in r.stderr
    r = run(base + ["--fold-cols-pan", "40", "--fold-cols-mss", "12", "-m", "1,2,3,4"], files)
    assert r.returncode == 107                                       # --band-map needs --GDAL
    r = run(base + ["--fold-cols-pan", "40", "--fold-cols-mss", "12", "--bogus"], files)
    assert r.returncode == 109


def test_tiff_external_strips_equal_write_rows(tmp_path):
    """TiffWriterU16::begin_external_strips / end_external_strips (what the device LZW encoder feeds, csrc/tifflzw.hip): strips
    encoded outside the writer and packed as oip_tiff_lzw_strips_u16 packs them give the file write_rows() gives, byte for byte
    (seven geometries; ASan + UBSan); misuse is refused."""
    src = os.path.join(ROOT, "tests", "cpp", "tiff_external_strips_test.cpp")
    inc = os.path.join(ROOT, "opticalimageprocessor_amd", "csrc")
    exe = tmp_path / "tiff_external"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + inc, src,
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "7 cases, 0 bad" in r.stdout, r.stdout + r.stderr


def test_rank_failure_protocol_under_thread_sanitizer(tmp_path):
    """csrc/oip_rankguard.hpp (HostBarrier + CommGuard of the N-GPU host): a rank that fails right behind the pre-exchange barrier
    aborts every communicator while its peers are posting grouped sends / receives -- no peer may touch a communicator after
    ncclCommAbort has freed it, every peer leaves with PeerFailed, the culprit with its own error.  Sanitizers are not
    available on the GPU pool, so the protocol is exercised here on fake communicators under TSan and ASan + UBSan.
    Every second round the peers sit in a call that blocks until it is aborted (an abort that waits for the calls in
    flight never returns then -- the binary runs under a time limit), and every round must report the culprit's own message,
    whatever its rank index, not the error of a peer's call that the abort released."""
    src = os.path.join(ROOT, "tests", "cpp", "rankguard_test.cpp")
    inc = os.path.join(ROOT, "opticalimageprocessor_amd", "csrc")
    # TSan's fixed shadow layout does not fit every randomised address space (kernels with more mmap entropy place the
    # executable or its libraries outside it: "FATAL: ThreadSanitizer: unexpected memory mapping"), so its binary runs with
    # address-space randomisation off for that one process
    no_aslr = ["setarch", platform.machine(), "-R"]
    for name, flags, launch in (("tsan", ["-fsanitize=thread"], no_aslr),
                                ("asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], [])):
        exe = tmp_path / ("rankguard_" + name)
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-I" + inc] + flags + [src, "-o", str(exe)], check=True)
        r = subprocess.run(launch + [str(exe), "4", "150"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "150 rounds, 0 bad" in r.stdout, r.stdout + r.stderr
        assert "75 rounds with a blocking call" in r.stdout, r.stdout


def test_loopback_communicator_protocol_under_sanitizers(tmp_path):
    """csrc/oip_loopcomm.hpp, the in-process communicator behind OIP_COMM=loopback (tests/test_gpu_multigpu_loopback.py runs the
    N-GPU host over it), on host memory with a fake stream that copies at once, under TSan and under ASan + UBSan: random
    exchange plans on 2, 3 and 4 rank threads (groups some ranks skip, one-way groups, a halo-style group, an all-gather; every
    received byte and the accounting checked), a size mismatch that both ranks are told, an abort that releases a blocking group
    end, a blocking send and an all-gather, and the rendezvous deadline's message for send, recv and allgather."""
    src = os.path.join(ROOT, "tests", "cpp", "loopcomm_test.cpp")
    inc = os.path.join(ROOT, "opticalimageprocessor_amd", "csrc")
    no_aslr = ["setarch", platform.machine(), "-R"]                 # (as above: TSan's shadow layout)
    for name, flags, launch in (("tsan", ["-fsanitize=thread"], no_aslr),
                                ("asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], [])):
        exe = tmp_path / ("loopcomm_" + name)
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-I" + inc] + flags + [src, "-o", str(exe)], check=True)
        r = subprocess.run(launch + [str(exe), "200"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "6 cases, 200 rounds per plan case" in r.stdout and ", 0 bad" in r.stdout, r.stdout + r.stderr


def test_node_plan_invariants_under_sanitizers(tmp_path):
    """csrc/oip_nodeplan.hpp, the plans of the N-GPU host, on the CPU under ASan + UBSan (tests/cpp/nodeplan_test.cpp; no HIP, the two
    *_src_range calls are stand-ins): for the strips of tests/test_gpu_multigpu_loopback.py (8 x 1 and 9 x 2 inter-band units, five CCD
    sections) at N = 2, 3, 4 all units of a group have one owner; the local groups and exchange_groups() together cover every unit
    exactly once in ascending order, so the host's exchange-and-correlate driver computes every unit once; a group is exchanged
    exactly when one of its units has a piece that changes rank; the mixed pair (8, 9) of 9 x 2 at N = 2 is one exchange group of
    rank 0; halo transfers never name src == dst, lie inside the source rank's block and leave no rank lacking a line."""
    src = os.path.join(ROOT, "tests", "cpp", "nodeplan_test.cpp")
    inc = [os.path.join(ROOT, "opticalimageprocessor_amd", "csrc"), os.path.join(ROOT, "include")]
    exe = tmp_path / "nodeplan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + ["-I" + i for i in inc] +
                   [src, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and " checks, 0 bad" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
    assert int(r.stdout.split()[-4]) > 1000, r.stdout[-200:]                 # the checks ran
