"""CPU: the tile arithmetic of the neighbourhood filters (csrc/oip_tileplan.h), which convolve.hip, despike.hip and denoise.hip
share, as a stand-alone program under ASan + UBSan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tile_plan_fill_border_partition_and_refusals(tmp_path):
    """tests/cpp/tileplan_test.cpp: for 1 and 4 samples per pixel, horizontal and vertical radii 0..4, widths 1..1025 pixels,
    1..33 lines, output ranges and resident windows cut at every line, aligned and odd bases, and four column groups of 1..512
    pixels, the header's own fill indexing puts into every LDS sample a lane reads the replicate-border sample of the line or the
    group, no index leaves the resident window (a heap block of exactly its size) or the LDS image, and the tiles partition the
    output once; the plan refuses exactly what oip_convolve_u16, oip_despike_u16 and oip_sigma_filter_u16 refuse of their common
    arguments, a window one line short at either end and 2^31 tiles included."""
    src = os.path.join(ROOT, "tests", "cpp", "tileplan_test.cpp")
    inc = os.path.join(ROOT, "opticalimageprocessor_amd", "csrc")
    exe = tmp_path / "tileplan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + inc, src, "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and " cases, 0 bad" in r.stdout, r.stdout + r.stderr
    assert int(r.stdout.split()[-4]) > 7000, r.stdout                # the exhaustive part ran
