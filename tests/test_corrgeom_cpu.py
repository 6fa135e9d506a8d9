"""CPU: the correlation-window geometry (csrc/oip_corrgeom.h) that the C ABI's whole-strip correlation calls, the single-GPU hosts
and the multi-GPU plans share, as a stand-alone program under ASan + UBSan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_correlation_geometry_values_properties_arrival_order_and_table(tmp_path):
    """tests/cpp/corrgeom_test.cpp: the hand-worked values of the 30000 x 100000 strip and the 262144-line CCD pair; for strips of
    16..4000 lines, 1..6 sections, 2..11 slices and windows of 64..1200 lines either maker refuses in the reference's words or
    its windows are in order, disjoint, inside both rasters and evenly spaced, the division's remainder in the last gap; the
    arrival order of the pipelined default action reads every line once, a section's lines before its units, everything before
    the fit, PAN in blocks no longer than asked; the shift table puts [unit][band] results at [band][unit] with the slice's
    centre column."""
    src = os.path.join(ROOT, "tests", "cpp", "corrgeom_test.cpp")
    inc = [os.path.join(ROOT, "opticalimageprocessor_amd", "csrc"), os.path.join(ROOT, "include")]
    exe = tmp_path / "corrgeom"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + ["-I" + i for i in inc] +
                   [src, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and " cases, 0 bad" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
    assert int(r.stdout.split()[-4]) > 150000, r.stdout[-200:]               # the sweeps ran
