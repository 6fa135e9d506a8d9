"""CPU: the arithmetic the device TIFF codecs share (csrc/oip_tiffstreams.h) -- the encode plan, the even-offset rule, the decode
scratch and the device-or-host route rule -- as a stand-alone program under ASan + UBSan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tiff_stream_plans_offsets_and_routes(tmp_path):
    """tests/cpp/tiffstreams_test.cpp: for both codecs and every image of 1..40 rows, 1..9 pixels, 1 or 4 samples and strips of 1..7
    rows the payload's worst case and the scratch equal the formulas the encoders had, the regions [tables | slots | len | off] tile
    the scratch from multiples of 256 bytes, a slot is a multiple of 4 that holds the worst stream; the same at a product's size, at
    70000 strips and at strips of 1 GiB against 128-bit arithmetic, with the refusals; every mix of six odd and even streams is
    placed at even offsets at most a byte apart, the same whether placed in one go or in two at any split; the route table."""
    src = os.path.join(ROOT, "tests", "cpp", "tiffstreams_test.cpp")
    inc = os.path.join(ROOT, "opticalimageprocessor_amd", "csrc")
    exe = tmp_path / "tiffstreams"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + inc, src, "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and " cases, 0 bad" in r.stdout, r.stdout + r.stderr
    assert int(r.stdout.split()[-4]) > 10000, r.stdout               # the exhaustive part ran
