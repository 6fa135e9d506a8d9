"""CPU: the baseline JPEG coder of include/oip_c.h (oip_jpeg_scan_u8) without a device.
1. The restatement (tests/_jpeg_ref.py) is a JPEG writer: Pillow's libjpeg opens its files, finds our quantisation tables, and the
   Huffman tables are those of a file libjpeg itself writes without optimising them.
2. Its arithmetic is as good as libjpeg's: both files decoded by Pillow, on a smooth scene with noise, our PSNR is within 0.1 dB of
   that of Pillow's own save(quality=Q, subsampling=0).
3. The host instantiation of csrc/oip_jpeg.h, the code the device runs as well, as a stand-alone program under ASan + UBSan
   (tests/cpp/jpeg_encode_test.cpp): every interval's bytes are the restatement's, and so is the file its writer makes.
The device runs of the same coder are GPU tests (tests/test_gpu_jpeg.py, tests/test_gpu_jpeg_beyond_2g.py, tests/test_gpu_jpeg_cli.py)."""
import io
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

import _jpeg_ref as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _decode(data):
    with Image.open(io.BytesIO(data)) as im:
        im.load()
        return im.mode, im.size, {k: list(v) for k, v in im.quantization.items()}, np.asarray(im)


def _pillow(img, quality, **kw):
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", quality=quality, subsampling=0, **kw)
    return b.getvalue()


def _psnr(a, b):
    return 10.0 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


@pytest.mark.parametrize("nch", [1, 3], ids=["grey", "rgb"])
@pytest.mark.parametrize("quality", [1, 50, 75, 90, 100])
def test_the_restatement_writes_files_libjpeg_reads(nch, quality):
    img = J.scene(67, 93, nch, 11)
    e = J.encode(img, quality)
    mode, size, qt, _ = _decode(e.file)
    assert mode == ("L" if nch == 1 else "RGB") and size == (93, 67)
    assert qt == {i: t for i, t in enumerate(e.qtables)}                       # (Pillow 12: natural order)
    ours, theirs = J.parse_segments(e.file), J.parse_segments(_pillow(img, quality))
    assert ours["dht"] == theirs["dht"] and len(ours["dht"]) == (2 if nch == 1 else 4)
    assert ours["dqt"] == theirs["dqt"]                                        # the IJG rule is libjpeg's
    assert ours["sof0"] == (8, 67, 93, [(c + 1, 0x11, min(c, 1)) for c in range(nch)])
    assert ours["dri"] == 12 and ours["sos"] == ([(c + 1, 0x11 * min(c, 1)) for c in range(nch)], 0, 63, 0)
    assert ours["app0"] == b"JFIF\0\1\1\0\0\1\0\1\0\0"
    assert e.file.endswith(b"\xff\xd9") and len(e.intervals) == 9
    # RST0..7 cycling between the intervals, none before EOI
    scan = e.file[ours["scan"]:-2]
    assert scan == b"".join(iv + (bytes([0xff, 0xd0 + k % 8]) if k < 8 else b"") for k, iv in enumerate(e.intervals))


@pytest.mark.parametrize("nch", [1, 3], ids=["grey", "rgb"])
@pytest.mark.parametrize("quality", [50, 75, 90])
def test_fidelity_against_libjpeg(nch, quality):
    """Measured with Pillow 12.2 on this 320 x 256 scene, PSNR ours - theirs in dB and
    file size against Pillow's with restart_marker_rows=1: grey Q50 -0.011 / 1.022, Q75 -0.013 / 1.018, Q90 -0.045 / 1.025; RGB
    Q50 -0.034 / 1.012, Q75 -0.031 / 1.012, Q90 -0.075 / 1.020 (grey Q100: +0.31 dB).  The margin is 0.1 dB; a larger gap is a
    defect of the arithmetic."""
    img = J.scene(256, 320, nch, 1)
    e = J.encode(img, quality)
    ours = _psnr(_decode(e.file)[3], img)
    theirs = _psnr(_decode(_pillow(img, quality))[3], img)
    print("nch %d Q %d: PSNR ours %.3f dB, Pillow %.3f dB, difference %+.3f dB; size %.4f of Pillow's with restart_marker_rows=1"
          % (nch, quality, ours, theirs, ours - theirs, len(e.file) / len(_pillow(img, quality, restart_marker_rows=1))))
    assert ours >= theirs - 0.1


def test_case_preconditions():
    for name, *_ in J.CASES:
        img, q = J.case_image(name)
        J.assert_case_preconditions(name, J.encode(img, q).trace)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("jpeg_encode")
    src = os.path.join(ROOT, "tests", "cpp", "jpeg_encode_test.cpp")
    inc = os.path.join(ROOT, "opticalimageprocessor_amd", "csrc")
    exe = d / "jpeg_encode_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + inc,
                    src, "-o", str(exe)], check=True)
    return str(exe)


def test_the_host_instantiation_gives_the_restatements_bytes(program, tmp_path):
    """every case of J.CASES, lines packed and (every other case) 5 bytes apart, from exact-size heap blocks; the program must end
    clean under the sanitizers"""
    d = str(tmp_path)
    lines, want = [], {}
    for k, (name, _, w, h, nch, q) in enumerate(J.CASES):
        img, _ = J.case_image(name)
        pitch = w * nch + (5 if k % 2 else 0)
        rows = np.full((h, pitch), 0xEE, dtype=np.uint8)
        rows[:, :w * nch] = img.reshape(h, w * nch)
        with open(os.path.join(d, name + ".bin"), "wb") as f:
            f.write(rows.tobytes()[:(h - 1) * pitch + w * nch])
        lines.append("%s %d %d %d %d %d" % (name, w, h, nch, q, pitch))
        want[name] = J.encode(img, q)
    with open(os.path.join(d, "list.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([program, d], capture_output=True, text=True)
    assert r.returncode == 0 and "%d images, 0 bad" % len(lines) in r.stdout and not r.stderr, r.stdout[-3000:] + r.stderr[-3000:]
    for name, e in want.items():
        with open(os.path.join(d, name + ".iv"), "rb") as f:
            data = f.read()
        got, p = [], 0
        while p < len(data):
            n = int.from_bytes(data[p:p + 4], "little")
            got.append(data[p + 4:p + 4 + n])
            p += 4 + n
        assert len(got) == len(e.intervals), name
        for k, (a, b) in enumerate(zip(got, e.intervals)):
            assert a == b, "%s: interval %d differs" % (name, k)
        with open(os.path.join(d, name + ".jpg"), "rb") as f:
            assert f.read() == e.file, name
