"""GPU: `oip regcheck` -> `oip regfix` -> `oip regcheck` end to end.  The product's bytes are those of the restatement
(_regfix_ref.py) fed the same report file, the bands that are not resampled are the input's, and the second report's RMS is a
quarter of the first's or less (the condition of tests/test_regfix_cpu.py, whose textures and field these are)."""
import os
import subprocess

import numpy as np
import pytest

import _regcheck_ref as rc
import _regfix_ref as ref
from _tiff import read_tiff_u16, write_tiff_u16

pytestmark = pytest.mark.gpu
OIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "opticalimageprocessor_amd", "lib", "oip")
TILE = ["--tile", "16", "--search", "3", "--step", "8"]


def _run(tool, args, cwd, **env):
    env = dict(os.environ, LOGFILE=os.path.join(cwd, "oip.log"), **env)
    return subprocess.run([OIP, tool] + args, cwd=cwd, env=env, capture_output=True, text=True)


def _ok(r):
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def _pair(h, w, seed):
    """A and B of tests/test_regfix_cpu.py: A's content at (y, x) is found in B near (y + dy, x + dx),
    dx = 1.2 sin(2 pi y / h) + 0.3, dy = 0.6 cos(2 pi x / w) - 0.5"""
    m = 8
    A0, B0 = rc.pair(h + 2 * m, w + 2 * m, (0, 0), seed)
    yy, xx = np.mgrid[0:h + 2 * m, 0:w + 2 * m]
    dx = 1.2 * np.sin(2 * np.pi * (yy - m) / h) + 0.3
    dy = 0.6 * np.cos(2 * np.pi * (xx - m) / w) - 0.5
    Bw = ref.warp(B0, np.rint(-dx * 1024).astype(np.int64), np.rint(-dy * 1024).astype(np.int64), 0, 0, 1, 1)
    return np.ascontiguousarray(A0[m:-m, m:-m]), np.ascontiguousarray(Bw[m:-m, m:-m])


def _rms(path):
    """(tiles used, rms) of a report's summary"""
    tail = [l for l in open(path).read().splitlines() if l.startswith("#")]
    v = [float(x) for x in tail[-1][2:].split(",")]
    return v[0], v[5]


def _want(report, img, band_mask=None, smooth=0):
    lines, w = img.shape[0], img.shape[1]
    NX, NY, g = ref.parse_report(open(report).read(), w, lines, smooth)
    return ref.warp(img, NX, NY, g["gx0"], g["gy0"], g["sx"], g["sy"], band_mask), g


def test_band_of_a_tiff(tmp_path, oracle_mod):
    """a 4-sample TIFF whose band 3 is warped against band 2: the default band is the report's band2, the other bands pass
    through; --bands all, --smooth 1, -o, --force"""
    d = str(tmp_path)
    h, w = 120, 150
    A, B = _pair(h, w, 1120)
    C1, C2 = rc.pair(h, w, (0, 0), 77)
    img = np.stack([C1, A, B, C2], axis=2)
    write_tiff_u16(os.path.join(d, "M.TIFF"), img)
    pair = ["--band1", "2", "--band2", "3"] + TILE
    _ok(_run("regcheck", ["--image1", "M.TIFF"] + pair, d))
    used, before = _rms(os.path.join(d, "M.REG.CSV"))
    assert used > 100 and 0.9 < before < 1.4
    r = _ok(_run("regfix", ["--report", "M.REG.CSV", "--image", "M.TIFF"], d))
    assert "regfix: " in r.stdout and "tiles used" in r.stdout
    got, _, _ = read_tiff_u16(os.path.join(d, "M.REGFIX.TIFF"))
    want, g = _want(os.path.join(d, "M.REG.CSV"), img, 4)
    assert g["band2"] == 3 and np.array_equal(got, want)
    for b in (0, 1, 3):
        assert np.array_equal(got[:, :, b], img[:, :, b])
    assert not np.array_equal(got[:, :, 2], img[:, :, 2])
    _ok(_run("regcheck", ["--image1", "M.REGFIX.TIFF", "-o", "after.csv"] + pair, d))
    used2, after = _rms(os.path.join(d, "after.csv"))
    print("\nregfix cli: rms %.4f -> %.4f" % (before, after))
    # (the tiles whose search window meets the zeros that the resampling leaves at the raster's edge carry the no-data flag)
    assert used2 >= 0.9 * used and after <= 0.25 * before, (before, after, used, used2)
    # the product exists: kept without --force, replaced with it
    keep = open(os.path.join(d, "M.REGFIX.TIFF"), "rb").read()
    r = _run("regfix", ["--report", "M.REG.CSV", "--image", "M.TIFF", "--bands", "1,3"], d)
    assert r.returncode == 2 and "--force" in r.stdout and open(os.path.join(d, "M.REGFIX.TIFF"), "rb").read() == keep
    _ok(_run("regfix", ["--report", "M.REG.CSV", "--image", "M.TIFF", "--bands", "1,3", "--force"], d))
    got, _, _ = read_tiff_u16(os.path.join(d, "M.REGFIX.TIFF"))
    assert np.array_equal(got, _want(os.path.join(d, "M.REG.CSV"), img, 5)[0])
    # --bands all --smooth 1 -o
    _ok(_run("regfix", ["--report", "M.REG.CSV", "--image", "M.TIFF", "--bands", "all", "--smooth", "1", "-o", "all.TIFF"], d))
    got, _, _ = read_tiff_u16(os.path.join(d, "all.TIFF"))
    want1 = _want(os.path.join(d, "M.REG.CSV"), img, 15, 1)[0]
    assert np.array_equal(got, want1) and not np.array_equal(want1[:, :, 2], want[:, :, 2])
    # a single-sample TIFF does not have the report's band 3
    write_tiff_u16(os.path.join(d, "P.TIFF"), B[:, :, None])
    r = _run("regfix", ["--report", "M.REG.CSV", "--image", "P.TIFF"], d)
    assert r.returncode == 254 and "--bands: band index out of range (1..1)" in r.stdout
    _ok(_run("regfix", ["--report", "M.REG.CSV", "--image", "P.TIFF", "--bands", "1"], d))
    got, _, _ = read_tiff_u16(os.path.join(d, "P.REGFIX.TIFF"))
    assert np.array_equal(got, want[:, :, 2])


def test_raw_strip_in_blocks(tmp_path, oracle_mod):
    """two single-band RAW images; the strip streamed in blocks of 16 lines (OIP_REGFIX_BLOCK_LINES) equals the one-block run"""
    d = str(tmp_path)
    h, w = 96, 130
    A, B = _pair(h, w, 1096)
    A.tofile(os.path.join(d, "A.RAW"))
    B.tofile(os.path.join(d, "B.RAW"))
    _ok(_run("regcheck", ["--image1", "A.RAW", "--image2", "B.RAW", "--width", str(w), "--step", "12"] + TILE[:4], d))
    _, before = _rms(os.path.join(d, "A.REG.CSV"))
    _ok(_run("regfix", ["--report", "A.REG.CSV", "--image", "B.RAW", "--width", str(w)], d))
    one = np.fromfile(os.path.join(d, "B.REGFIX.RAW"), np.uint16).reshape(h, w)
    assert np.array_equal(one, _want(os.path.join(d, "A.REG.CSV"), B)[0])
    _ok(_run("regfix", ["--report", "A.REG.CSV", "--image", "B.RAW", "--width", str(w), "-o", "blocks.RAW"], d, OIP_REGFIX_BLOCK_LINES="16"))
    assert np.array_equal(np.fromfile(os.path.join(d, "blocks.RAW"), np.uint16).reshape(h, w), one)
    _ok(_run("regcheck", ["--image1", "A.RAW", "--image2", "B.REGFIX.RAW", "--width", str(w), "--step", "12", "-o", "after.csv"] + TILE[:4], d))
    _, after = _rms(os.path.join(d, "after.csv"))
    assert after <= 0.25 * before, (before, after)
    # the report is about another image size: refused before anything is written
    B[:, :100].copy().tofile(os.path.join(d, "N.RAW"))
    r = _run("regfix", ["--report", "A.REG.CSV", "--image", "N.RAW", "--width", "100"], d)
    assert r.returncode == 2 and "outside the image" in r.stdout and not os.path.exists(os.path.join(d, "N.REGFIX.RAW"))


def test_report_with_scale_4_and_shift_x(tmp_path, oracle_mod):
    """PAN against an MSS band: image 1 at four times the size, image 2 beginning at column 20 of its decimation.  The report
    counts in image-1 pixels; a node lies at (x / 4 - 20, y / 4) of image 2"""
    d = str(tmp_path)
    h, w, off = 120, 150, 20
    A, B = _pair(h, w, 1120)
    np.kron(A, np.ones((4, 4), np.uint16)).tofile(os.path.join(d, "PAN.RAW"))
    B2 = np.ascontiguousarray(B[:, off:])
    B2.tofile(os.path.join(d, "MSS.RAW"))
    both = ["--image1", "PAN.RAW", "--width", str(4 * w), "--width2", str(w - off), "--scale", "4", "--shift-x", str(off)] + TILE
    _ok(_run("regcheck", both + ["--image2", "MSS.RAW"], d))
    _, before = _rms(os.path.join(d, "PAN.REG.CSV"))
    head = open(os.path.join(d, "PAN.REG.CSV")).readline()
    assert "scale=4" in head and "shift-x=20" in head
    _ok(_run("regfix", ["--report", "PAN.REG.CSV", "--image", "MSS.RAW", "--width", str(w - off)], d))
    got = np.fromfile(os.path.join(d, "MSS.REGFIX.RAW"), np.uint16).reshape(h, w - off)
    want, g = _want(os.path.join(d, "PAN.REG.CSV"), B2)
    assert (g["gx0"], g["gy0"], g["sx"], g["sy"]) == (3 + 8, 3 + 8, 8, 8) and np.array_equal(got, want)
    _ok(_run("regcheck", both + ["--image2", "MSS.REGFIX.RAW", "-o", "after.csv"], d))
    _, after = _rms(os.path.join(d, "after.csv"))
    assert 0.9 < before < 1.4 and after <= 0.25 * before, (before, after)
