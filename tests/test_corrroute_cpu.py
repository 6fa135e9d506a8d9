"""CPU: the planner of the correlation drivers (csrc/oip_corrroute.h) -- the switches, the route of an inter-band geometry, the
FFT plans of its arrays and its workspace -- as a stand-alone program under ASan + UBSan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_correlation_route_table_refusals_and_workspace_properties(tmp_path):
    """tests/cpp/corrroute_test.cpp: the route and stored-window radius of the product's geometries under every switch that
    moves them, worked out by hand from the planner's conditions; the refusal of more than 65535 correlation lines in its own
    words; and for every 2^a 3^b 5^c line count from 8 to 16000 x {3000, 1228, 320, 200} columns x every combination of
    OIP_SPECTRAL_UP, OIP_SPECTRAL_V and OIP_PEAK_PRUNE either a refusal with a text or a plan whose regions are 256-byte aligned,
    in order, disjoint and sum to its total, whose arrays inside a slot fit it, whose window radius is -1 or fits the tile
    lists, and whose description is JSON naming its route."""
    src = os.path.join(ROOT, "tests", "cpp", "corrroute_test.cpp")
    inc = [os.path.join(ROOT, "opticalimageprocessor_amd", "csrc"), os.path.join(ROOT, "include")]
    exe = tmp_path / "corrroute"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + ["-I" + i for i in inc] +
                   [src, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and " cases, 0 bad" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
    # 193 line counts x 4 widths x 12 switch settings = 9264 plans of the sweep, and the table
    assert int(r.stdout.split()[-4]) > 9264, r.stdout[-200:]               # the sweep ran
