"""GPU: `oip wallis` end to end -- the product's bytes are restatement(moments -> wallis_fit -> apply) (_wallis_ref.py) on a RAW
strip streamed in several blocks and on a 4-sample TIFF; the CSV holds the report's values; --mean / --std are honoured; an
existing output is refused without --force."""
import os
import subprocess

import numpy as np
import pytest

from opticalimageprocessor_amd import capi
import _wallis_ref as ref
from _tiff import read_tiff_u16, write_tiff_u16

pytestmark = pytest.mark.gpu
OIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "opticalimageprocessor_amd", "lib", "oip")


def _run(args, cwd, **env):
    env = dict(os.environ, LOGFILE=os.path.join(cwd, "oip.log"), **env)
    return subprocess.run([OIP, "wallis"] + args, cwd=cwd, env=env, capture_output=True, text=True)


def _ok(r):
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def _want(img, spp, B, cmax=65535, **kw):
    """restatement(moments) -> the library's fit -> restatement(apply)"""
    G, O, _, report = capi.wallis_fit(ref.moments(img, spp, B), **kw)
    out, counts = ref.apply(img, spp, G, O, B, 1, 65535, cmax)
    return out, counts, report


def _read_report(path, spp):
    lines = open(path).read().splitlines()
    assert lines[0].startswith("# oip wallis image=") and lines[1] == "channel," + ",".join(capi.WALLIS_REPORT)
    rows = [[float(v) for v in ln.split(",")[1:]] for ln in lines[2:2 + spp]]
    counters = dict(ln.split(",") for ln in lines[2 + spp:])
    return lines[0], np.array(rows), [int(counters[k]) for k in ("transformed_samples", "clamped_low", "clamped_high")]


def _strip(L, w, seed):
    """texture under a brightness ramp along and across the strip, a zero-filled border and a block of zeros"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:L, 0:w]
    img = np.clip((1200 + 250 * rng.standard_normal((L, w))) * (0.6 + 0.5 * yy / L + 0.3 * xx / w), 1, 4095).astype(np.uint16)
    img[:, :3] = 0
    img[96:128, 32:64] = 0
    return img


def test_raw_strip_in_several_blocks(tmp_path):
    """64 columns x 400 lines, B 32; OIP_WALLIS_BLOCK_LINES 70 cuts pass 1 into blocks of 64 lines and pass 2 into blocks of 70"""
    d = str(tmp_path)
    L, w, B = 400, 64, 32
    img = _strip(L, w, 2)
    img.tofile(os.path.join(d, "P.RAW"))
    r = _ok(_run(["P.RAW", "--width", str(w), "--block", str(B), "--max-value", "2000"], d, OIP_WALLIS_BLOCK_LINES="70"))
    want, wc, report = _want(img, 1, B, 2000)
    assert report[0, 6] >= 1 and wc[2] > 0                             # a substituted node; results cut at 2000
    got = np.fromfile(os.path.join(d, "P.WAL.RAW"), np.uint16).reshape(L, w)
    assert np.array_equal(got, want), "%d samples differ" % int((got != want).sum())
    head, rows, counts = _read_report(os.path.join(d, "P.WAL.CSV"), 1)
    assert np.array_equal(rows, report) and counts == [int(v) for v in wc]
    assert " width=64 line-offset=0 lines=400 samples=1 block=32 contrast=0.80000000000000004 " in head and "max-value=2000" in head and "MBps" in r.stdout
    # one block per pass: the same files
    _ok(_run(["P.RAW", "--width", str(w), "--block", str(B), "--max-value", "2000", "-o", "one.RAW", "--report", "one.csv"], d))
    assert open(os.path.join(d, "one.RAW"), "rb").read() == open(os.path.join(d, "P.WAL.RAW"), "rb").read()
    assert open(os.path.join(d, "one.csv")).read() == open(os.path.join(d, "P.WAL.CSV")).read()
    # an existing output: refused, then replaced with --force; targets and other options, other bytes
    before = open(os.path.join(d, "P.WAL.RAW"), "rb").read()
    args = ["P.RAW", "--width", str(w), "--block", "64", "--mean", "2000", "--std", "150.5", "--contrast", "1", "--brightness", "0.9", "--max-gain", "2"]
    r = _run(args, d)
    assert r.returncode == 2 and "--force" in r.stdout and open(os.path.join(d, "P.WAL.RAW"), "rb").read() == before
    _ok(_run(args + ["--force"], d, OIP_WALLIS_BLOCK_LINES="130"))
    want, wc, report = _want(img, 1, 64, contrast=1.0, brightness=0.9, g_max=2.0, target_mean=[2000.0], target_std=[150.5])
    assert np.array_equal(np.fromfile(os.path.join(d, "P.WAL.RAW"), np.uint16).reshape(L, w), want)
    _, rows, counts = _read_report(os.path.join(d, "P.WAL.CSV"), 1)
    assert np.array_equal(rows, report) and rows[0, 3] == 2000.0 and rows[0, 4] == 150.5 and counts == [int(v) for v in wc]
    # a line range is the raster
    _ok(_run(["P.RAW", "--width", str(w), "--block", str(B), "--line-offset", "37", "--lines", "200", "-o", "part.RAW", "--report", "part.csv"], d,
             OIP_WALLIS_BLOCK_LINES="70"))
    want, wc, report = _want(img[37:237], 1, B)
    assert np.array_equal(np.fromfile(os.path.join(d, "part.RAW"), np.uint16).reshape(200, w), want)
    assert " line-offset=37 lines=200 " in open(os.path.join(d, "part.csv")).readline()


def test_four_band_tiff(tmp_path):
    d = str(tmp_path)
    H, W, B = 150, 200, 64
    dn = np.stack([_strip(H, W, 10 + c) for c in range(4)], axis=2)
    write_tiff_u16(os.path.join(d, "S.TIFF"), dn)
    img = dn.reshape(H, W * 4)
    _ok(_run(["S.TIFF", "--block", str(B)], d))
    want, wc, report = _want(img, 4, B)
    got = read_tiff_u16(os.path.join(d, "S.WAL.TIFF"))[0].reshape(H, W * 4)
    assert np.array_equal(got, want), "%d samples differ" % int((got != want).sum())
    _, rows, counts = _read_report(os.path.join(d, "S.WAL.CSV"), 4)
    assert np.array_equal(rows, report) and counts == [int(v) for v in wc]
    # a target per channel; a constant channel without --std is refused by name and leaves nothing behind
    _ok(_run(["S.TIFF", "--block", str(B), "--mean", "1000,1500,2000,2500", "--std", "100,200,300,400", "-o", "t.TIFF", "--report", "t.csv"], d))
    want, wc, report = _want(img, 4, B, target_mean=[1000.0, 1500.0, 2000.0, 2500.0], target_std=[100.0, 200.0, 300.0, 400.0])
    assert np.array_equal(read_tiff_u16(os.path.join(d, "t.TIFF"))[0].reshape(H, W * 4), want)
    assert np.array_equal(_read_report(os.path.join(d, "t.csv"), 4)[1], report)
    flat = dn.copy()
    flat[:, :, 3] = 4095
    write_tiff_u16(os.path.join(d, "A.TIFF"), flat)
    r = _run(["A.TIFF", "--block", str(B)], d)
    assert r.returncode == 2 and "channel 3" in r.stdout and not os.path.exists(os.path.join(d, "A.WAL.TIFF")) and not os.path.exists(os.path.join(d, "A.WAL.CSV"))
    _ok(_run(["A.TIFF", "--block", str(B), "--std", "200"], d))
    got = read_tiff_u16(os.path.join(d, "A.WAL.TIFF"))[0].reshape(H, W, 4)
    assert (got[:, :, 3] == 4095).all()
