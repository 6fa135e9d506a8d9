"""CPU: the definition of `oip regfix` on its numpy restatement (_regfix_ref.py) -- a zero field is the identity, a constant
field is the constant-shift resampler, and on seeded textures warped by a smooth field the report of regcheck's restatement,
turned into a field and applied, brings regcheck's RMS down to a quarter or less --, the host entry points
oip_regfix_load_report / oip_regfix_fill / oip_regfix_smooth through capi against the restatement, the report parser
(csrc/oip_warpfield.hpp) as a stand-alone program under ASan + UBSan, and what the command refuses before a device is touched."""
import os
import subprocess

import numpy as np
import pytest

import _regcheck_ref as rc
import _regfix_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _image(W, L, seed=5):
    return np.random.default_rng(seed).integers(0, 65536, (L, W), dtype=np.uint16)


def test_zero_field_is_the_identity(oracle_mod):
    for W, L in ((1, 1), (7, 4), (67, 37)):
        img = _image(W, L)
        for nx, ny, sx, sy, g0 in ((1, 1, 1, 1, 0), (2, 3, 64, 5, -9), (4, 2, 7, 100, 30)):
            Z = np.zeros((ny, nx), np.int32)
            assert np.array_equal(ref.warp(img, Z, Z, g0, g0 - 1, sx, sy), img)
    # ... and so is every value that rounds to 0/32 px: -16 .. 15 of 1/1024
    img = _image(20, 9)
    for v in (-16, 15):
        assert np.array_equal(ref.warp(img, np.full((2, 2), v), np.full((2, 2), v), 0, 0, 8, 8), img)
    assert not np.array_equal(ref.warp(img, np.full((2, 2), 16), np.zeros((2, 2), int), 0, 0, 8, 8), img)


def test_constant_field_is_prestitch_with_one_section(oracle_mod):
    W, L = 96, 120
    img = _image(W, L, 6)
    NX, NY = np.full((3, 4), 13 * 32), np.full((3, 4), -42 * 32)
    want, _ = oracle_mod.prestitch(img, 13 / 32, -42 / 32, section_rows=L, row_guard=0)
    assert np.array_equal(ref.warp(img, NX, NY, -5, 7, 40, 50), want)
    assert not np.array_equal(want, img)


def _regcheck(A, B, T, S, step):
    """(dx, dy, score, flags) as (ny, nx) arrays, the grid, and the RMS of the summary"""
    h, w = A.shape
    x0, y0, nx, ny = rc.grid(w, h, T, S, step)
    recs, _, _ = rc.match_tiles(A, B, T, S, x0, y0, step, step, nx, ny)
    pk = np.array([rc.peak(r, T, S) for r in recs]).reshape(ny, nx, 4)
    dx, dy, sc, fl = pk[..., 0], pk[..., 1], pk[..., 2], pk[..., 3].astype(int)
    return (dx, dy, sc, fl), (x0, y0, nx, ny), rc.summary(dx, dy, fl)[5]


LOOP_CASES = [(160, 208, 16, 3, 16), (200, 260, 32, 4, 16), (120, 150, 16, 3, 8), (96, 130, 16, 3, 12)]


@pytest.mark.parametrize("h,w,T,S,step", LOOP_CASES)
@pytest.mark.parametrize("smooth", [0, 1])
def test_the_loop_closes(oracle_mod, h, w, T, S, step, smooth):
    """A, B0: a _regcheck_ref.pair texture without shift, 8 pixels larger on every side.  B is B0 warped so that A's content at
    (y, x) is found in B near (y + dy, x + dx), dx = 1.2 sin(2 pi y / h) + 0.3, dy = 0.6 cos(2 pi x / w) - 0.5; both are then
    cropped, so no border value enters.  regcheck -> report -> field -> warp -> regcheck: the RMS falls to a quarter or less (the
    condition; the restatement itself stays under 0.15 of it)"""
    m = 8
    A0, B0 = rc.pair(h + 2 * m, w + 2 * m, (0, 0), 1000 + h)
    yy, xx = np.mgrid[0:h + 2 * m, 0:w + 2 * m]
    dx = 1.2 * np.sin(2 * np.pi * (yy - m) / h) + 0.3
    dy = 0.6 * np.cos(2 * np.pi * (xx - m) / w) - 0.5
    Bw = ref.warp(B0, np.rint(-dx * 1024).astype(np.int64), np.rint(-dy * 1024).astype(np.int64), 0, 0, 1, 1)      # a node per pixel
    A, B = A0[m:-m, m:-m], Bw[m:-m, m:-m]
    (mx, my, sc, fl), (x0, y0, nx, ny), before = _regcheck(A, B, T, S, step)
    assert (fl == 0).all() and 1.0 < before < 1.3, before
    NX, NY, g = ref.parse_report(ref.report_text(mx, my, sc, fl, x0, y0, step, T), w, h, smooth)
    assert NX.shape == (ny, nx) and (g["gx0"], g["gy0"], g["sx"], g["sy"]) == (x0 + T // 2, y0 + T // 2, step, step)
    fixed = ref.warp(B, NX, NY, g["gx0"], g["gy0"], g["sx"], g["sy"])
    _, _, after = _regcheck(A, fixed, T, S, step)
    print("\nregfix loop %s smooth %d: rms %.4f -> %.4f (ratio %.3f)" % ((h, w, T, S, step), smooth, before, after, after / before))
    assert after <= 0.25 * before, (before, after)


# ---- the host entry points against the restatement ---------------------------------------------------------------------------
def _masks(ny, nx, rng):
    hole = np.ones((ny, nx), bool)
    hole[ny // 2, nx // 2] = False                               # an isolated hole
    border = np.zeros((ny, nx), bool)
    border[1:-1, 1:-1] = True                                    # a flagged border: corners need two passes
    one = np.zeros((ny, nx), bool)
    one[ny - 1, 0] = True                                        # all but one flagged
    return [hole, border, one, rng.random((ny, nx)) < 0.3, np.ones((ny, nx), bool)]


def test_fill_against_the_restatement():
    import opticalimageprocessor_amd as oip
    rng = np.random.default_rng(11)
    for ny, nx in ((5, 7), (1, 9), (6, 1), (3, 3)):
        X, Y = rng.integers(-65536, 65537, (ny, nx)).astype(np.int32), rng.integers(-3000, 3001, (ny, nx)).astype(np.int32)
        for m in _masks(ny, nx, rng):
            if not m.any():
                continue
            gx, gy = oip.regfix_fill(X, Y, m)
            wx, wy = ref.fill(X, Y, m)
            assert np.array_equal(gx, wx) and np.array_equal(gy, wy), (ny, nx, m)
            assert np.array_equal(gx[m], X[m]) and gx.min() >= X[m].min() and gx.max() <= X[m].max()
    # known answers: the hole is the rounded mean of its four neighbours, negative means round to the nearest too (ties up)
    X = np.array([[0, -7, 0], [-2, 99, -4], [0, -6, 0]], np.int32)
    m = np.ones((3, 3), bool)
    m[1, 1] = False
    assert oip.regfix_fill(X, -X, m)[0][1, 1] == -5 and oip.regfix_fill(X, -X, m)[1][1, 1] == 5        # -19 / 4 = -4.75, 4.75
    X[0, 1] = -5
    assert oip.regfix_fill(X, -X, m)[0][1, 1] == -4 and oip.regfix_fill(X, -X, m)[1][1, 1] == 4        # -17 / 4 = -4.25
    X[0, 1] = -4
    assert oip.regfix_fill(X, -X, m)[0][1, 1] == -4 and oip.regfix_fill(X, -X, m)[1][1, 1] == 4        # -4 exactly
    X[0, 1] = -6
    assert oip.regfix_fill(X, -X, m)[0][1, 1] == -4 and oip.regfix_fill(X, -X, m)[1][1, 1] == 5        # -4.5 -> -4, 4.5 -> 5
    with pytest.raises(ValueError):
        oip.regfix_fill(X, X, np.zeros((3, 3), bool))


def test_smooth_against_the_restatement():
    import opticalimageprocessor_amd as oip
    rng = np.random.default_rng(12)
    for ny, nx in ((5, 7), (1, 9), (6, 1), (1, 1), (2, 2)):
        X, Y = rng.integers(-65536, 65537, (ny, nx)).astype(np.int32), rng.integers(-9, 10, (ny, nx)).astype(np.int32)
        for p in (0, 1, 2, 3, 16):
            gx, gy = oip.regfix_smooth(X, Y, p)
            assert np.array_equal(gx, ref.smooth(X, p)) and np.array_equal(gy, ref.smooth(Y, p)), (ny, nx, p)
        assert np.array_equal(oip.regfix_smooth(X, Y, 0)[0], X)
    # negative values: the shift floors, (a + 2 b + c + 2) >> 2 of (-1, -1, -2) is (-5 + 2) >> 2 = -1, of (-2, -2, -3) is -2
    gx, _ = oip.regfix_smooth(np.array([[-1, -1, -2, -2, -3]], np.int32), np.zeros((1, 5), np.int32), 1)
    assert gx.tolist() == [[-1, -1, -2, -2, -3]]
    gx, _ = oip.regfix_smooth(np.array([[-8, 0, 0]], np.int32), np.zeros((1, 3), np.int32), 1)
    assert gx.tolist() == [[-6, -2, 0]]
    for bad in (-1, 17):
        with pytest.raises(ValueError):
            oip.regfix_smooth(X, Y, bad)


def _report(rng, ny, nx, share, scale=1, shift=(0, 0), band2=1):
    dx, dy = rng.normal(0.3, 1.5, (ny, nx)), rng.normal(-0.2, 0.8, (ny, nx))
    fl = np.where(rng.random((ny, nx)) < share, rng.integers(1, 16, (ny, nx)), 0)
    fl[0, 0] = 0
    return ref.report_text(dx, dy, rng.random((ny, nx)), fl, 4, 4, 24, 16, scale, shift, band2)


def test_load_report_against_the_restatement(tmp_path):
    import opticalimageprocessor_amd as oip
    rng = np.random.default_rng(13)
    path = str(tmp_path / "R.CSV")
    for ny, nx, share, scale, shift, band2 in ((6, 9, 0.3, 1, (0, 0), 1), (1, 4, 0.0, 4, (-3, 2), 3), (5, 1, 0.5, 2, (100, 0), 4), (1, 1, 0.0, 1, (0, 0), 2),
                                               (7, 7, 0.95, 1, (5, -5), 1)):
        text = _report(rng, ny, nx, share, scale, shift, band2)
        open(path, "w").write(text)
        X, Y, g = oip.regfix_load_report(path)
        for p in (0, 1, 2, 3):
            wx, wy, wg = ref.parse_report(text, smooth_passes=p)
            sx, sy = oip.regfix_smooth(X, Y, p)
            assert np.array_equal(sx, wx) and np.array_equal(sy, wy) and g == wg, (ny, nx, p, g, wg)
        assert g["band2"] == band2 and g["gx0"] == 4 + 8 - shift[0] and g["gy0"] == 4 + 8 - shift[1] and g["sx"] == (24 if nx > 1 else 1)
        # the image the field is for: its last node must lie inside
        lx, ly = g["gx0"] + (nx - 1) * g["sx"], g["gy0"] + (ny - 1) * g["sy"]
        if g["gx0"] >= 0 and g["gy0"] >= 0:
            oip.regfix_load_report(path, lx + 1, ly + 1)
            with pytest.raises(ValueError, match="outside the image"):
                oip.regfix_load_report(path, lx, ly + 1)
        else:
            with pytest.raises(ValueError, match="outside the image"):
                oip.regfix_load_report(path, 10000, 10000)
    with pytest.raises(ValueError, match="room for"):
        oip.regfix_load_report(path, cap=48)
    with pytest.raises(OSError):
        oip.regfix_load_report(str(tmp_path / "missing.csv"))
    # rint of d * 1024 in fp64, ties to even: 0.00048828125 * 1024 = 0.5 -> 0, 0.00146484375 * 1024 = 1.5 -> 2
    open(path, "w").write("# oip regcheck band2=1 scale=1 shift-x=0 shift-y=0\n8,8,0.00048828125,0.00146484375,0.9,0\n")
    X, Y, _ = oip.regfix_load_report(path)
    assert X.tolist() == [[0]] and Y.tolist() == [[2]]


def test_report_parser_under_sanitizers(tmp_path):
    """tests/cpp/warpfield_test.cpp: minimal and malformed reports through oip_regfix_load_report with node buffers of exactly
    the stated size, fill and smoothing on lattices of one node, line and column -- under ASan + UBSan"""
    src = [os.path.join(ROOT, "tests", "cpp", "warpfield_test.cpp"), os.path.join(ROOT, "opticalimageprocessor_amd", "csrc", "host.cpp")]
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "opticalimageprocessor_amd", "csrc")]
    exe = tmp_path / "warpfield"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + inc + src +
                   ["-o", str(exe)], check=True)
    r = subprocess.run([str(exe), str(tmp_path / "report.csv")], capture_output=True, text=True)
    assert r.returncode == 0 and " checks, 0 bad" in r.stdout and "FAILED" not in r.stdout, r.stdout + r.stderr
    assert int(r.stdout.split()[-4]) > 300, r.stdout                  # every part ran


def test_cli_refusals_need_no_device(tmp_path):
    oip = os.path.join(ROOT, "opticalimageprocessor_amd", "lib", "oip")
    d = str(tmp_path)
    np.zeros((100, 80), np.uint16).tofile(os.path.join(d, "B.RAW"))
    open(os.path.join(d, "B.PNG"), "wb").write(b"x" * 80)
    open(os.path.join(d, "there.RAW"), "wb").write(b"kept")
    rng = np.random.default_rng(14)
    open(os.path.join(d, "R.CSV"), "w").write(_report(rng, 3, 2, 0.0))             # nodes at 12 + 24 i: inside 80 x 100
    open(os.path.join(d, "WIDE.CSV"), "w").write(_report(rng, 3, 4, 0.0))          # a node at column 84
    open(os.path.join(d, "FLAGGED.CSV"), "w").write(_report(rng, 2, 2, 0.0).replace(",0\n", ",4\n"))
    open(os.path.join(d, "NOHEAD.CSV"), "w").write(_report(rng, 2, 2, 0.0).replace(" scale=1", ""))
    open(os.path.join(d, "RAGGED.CSV"), "w").write(_report(rng, 2, 2, 0.0) + "60,60,0,0,0.9,0\n")
    open(os.path.join(d, "NAN.CSV"), "w").write(_report(rng, 1, 1, 0.0).replace("\n12,12,", "\n12,12,nan,"))
    open(os.path.join(d, "BAND3.CSV"), "w").write(_report(rng, 3, 2, 0.0, band2=3))

    def run(args):
        env = dict(os.environ, LOGFILE=os.path.join(d, "oip.log"))
        return subprocess.run([oip, "regfix"] + args, cwd=d, env=env, capture_output=True, text=True)
    ok = ["--report", "R.CSV", "--image", "B.RAW", "--width", "80"]
    for args, code, text in (([], 106, "--report is required"), (ok[:2], 106, "--image is required"), (ok[2:], 106, "--report is required"),
                             (["--report", "missing.CSV"] + ok[2:], 105, "does not exist"), (ok[:2] + ["--image", "missing.RAW"], 105, "does not exist"),
                             (ok + ["--smooth", "-1"], 105, "--smooth"), (ok + ["--smooth", "17"], 105, "--smooth"), (ok + ["--smooth", "x"], 104, "Could not convert"),
                             (ok + ["--bands", "0"], 105, "--bands"), (ok + ["--bands", "5"], 105, "--bands"), (ok + ["--bands", "1,,2"], 105, "--bands"),
                             (ok + ["--bands", ""], 105, "--bands"), (ok + ["--bands", "ALL"], 105, "--bands"), (ok + ["--width", "0"], 105, "--width"),
                             (ok + ["--bil"], 2, "BIL RAW"), (ok + ["--bands", "2"], 254, "--bands: band index out of range (1..1)"),
                             (ok[:2] + ["--image", "B.PNG"], 2, "only RAW and TIFF image supported"), (ok[:4] + ["--width", "81"], 2, "file size invalid"),
                             (["--report", "WIDE.CSV"] + ok[2:], 2, "outside the image"), (["--report", "FLAGGED.CSV"] + ok[2:], 2, "no usable tile"),
                             (["--report", "NOHEAD.CSV"] + ok[2:], 2, "the header lacks scale="), (["--report", "RAGGED.CSV"] + ok[2:], 2, "lattice"),
                             (["--report", "NAN.CSV"] + ok[2:], 2, "not finite"), (["--report", "B.RAW"] + ok[2:], 2, "regcheck report invalid"),
                             (["--report", "BAND3.CSV"] + ok[2:], 254, "--bands: band index out of range (1..1)"),
                             (ok + ["-o", "there.RAW"], 2, "--force"), (ok + ["-o", "B.RAW", "--force"], 2, "is the input image"),
                             (ok + ["-o", "out.TIFF"], 2, "container of the input"), (ok + ["--tile", "16"], 109, "--tile")):
        r = run(args)
        assert r.returncode == code and text in r.stdout + r.stderr, (args, r.returncode, r.stdout + r.stderr)
    assert open(os.path.join(d, "there.RAW"), "rb").read() == b"kept" and not os.path.exists(os.path.join(d, "B.REGFIX.RAW"))
