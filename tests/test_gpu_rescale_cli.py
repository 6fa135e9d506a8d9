"""GPU: `oip rescale` end to end -- a TIFF product of 4 samples a pixel and a RAW strip through --scale 0.8, --scale-y 3/4 and
--to-width; the outputs, read back with tests/_tiff.py, are the restatement's bytes (_rescale_ref.py); -o switches the container;
the log states the output size (a RAW output needs it as --width of the next tool); --force; the exit codes."""
import os
import subprocess

import numpy as np
import pytest

import _rescale_ref as ref
from _tiff import read_tiff_u16, write_tiff_u16

pytestmark = pytest.mark.gpu
OIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "opticalimageprocessor_amd", "lib", "oip")


def _run(args, cwd):
    env = dict(os.environ, LOGFILE=os.path.join(cwd, "oip.log"))
    return subprocess.run([OIP, "rescale"] + args, cwd=cwd, env=env, capture_output=True, text=True)


def _ok(r):
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def _scene(L, w, seed, border=True):
    """texture over a ramp with 0 and 65535 among it, and a zero-filled border (no data)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:L, 0:w]
    img = np.clip(1500 + 400 * rng.standard_normal((L, w)) + 3 * yy + 2 * xx, 1, 65535).astype(np.uint16)
    img[rng.random(img.shape) < 0.003] = 65535
    img[rng.random(img.shape) < 0.003] = 0
    if border:
        img[:, :5] = 0
        img[-4:] = 0
    return img


def test_four_band_tiff(tmp_path):
    d = str(tmp_path)
    H, W = 150, 200
    dn = np.stack([_scene(H, W, 30 + c) for c in range(4)], axis=2)
    write_tiff_u16(os.path.join(d, "S.TIFF"), dn)
    img = dn.reshape(H, W * 4)
    r = _ok(_run(["S.TIFF", "--scale", "0.8"], d))
    assert "200 x 150 -> 160 x 120 pixels of 4 samples, kernel lanczos, 8 x 8 taps, valid-min 1" in r.stdout and "MBps" in r.stdout
    got = read_tiff_u16(os.path.join(d, "S.RSC.TIFF"))[0]
    assert got.shape == (120, 160, 4)
    want = ref.rescale_kind(img, 4, 160, 120, "lanczos", valid_min=1)
    assert np.array_equal(got.reshape(120, 160 * 4), want), "%d samples differ" % int((got.reshape(120, -1) != want).sum())
    assert (got[:, :4] == 0).all() and (got[-3:] == 0).all()            # no data stays no data
    # an existing output: refused, then replaced with --force; other options, other bytes
    before = open(os.path.join(d, "S.RSC.TIFF"), "rb").read()
    args = ["S.TIFF", "--scale-x", "3/2", "--to-lines", "61", "--kernel", "linear", "--valid-min", "0"]
    r = _run(args, d)
    assert r.returncode == 2 and "--force" in r.stdout + r.stderr and open(os.path.join(d, "S.RSC.TIFF"), "rb").read() == before
    r = _ok(_run(args + ["--force"], d))
    assert "-> 300 x 61 pixels of 4 samples, kernel linear" in r.stdout
    got = read_tiff_u16(os.path.join(d, "S.RSC.TIFF"))[0].reshape(61, 300 * 4)
    assert np.array_equal(got, ref.rescale_kind(img, 4, 300, 61, "linear"))
    # a RAW file holds one sample per pixel; a ratio outside 1/4 .. 16: refused with 2, nothing written
    for extra, text in ((["--scale", "2", "-o", "S4.RAW"], "one sample per pixel"), (["--scale", "0.2", "-o", "tiny.TIFF"], "1/4 .. 16"),
                        (["--to-width", "3201", "-o", "wide.TIFF"], "beyond 16")):
        r = _run(["S.TIFF"] + extra, d)
        assert r.returncode == 2 and text in r.stdout + r.stderr and not os.path.exists(os.path.join(d, extra[-1])), r.stdout + r.stderr


def test_raw_strip_and_container_switch(tmp_path):
    d = str(tmp_path)
    L, w = 300, 96
    img = _scene(L, w, 7)
    img.tofile(os.path.join(d, "P.RAW"))
    # the line-rate correction: lines only
    r = _ok(_run(["P.RAW", "--width", str(w), "--scale-y", "3/4"], d))
    assert "96 x 300 -> 96 x 225 pixels of 1 samples" in r.stdout and "strip of 96 x 225 samples (--width 96)" in r.stdout
    got = np.fromfile(os.path.join(d, "P.RSC.RAW"), np.uint16)
    assert got.size == 225 * 96
    want = ref.rescale_kind(img, 1, 96, 225, "lanczos", valid_min=1)
    assert np.array_equal(got.reshape(225, 96), want)
    # the output is a strip like any other: --width as logged
    r = _ok(_run(["P.RSC.RAW", "--width", "96", "--to-width", "131", "--kernel", "cubic", "-o", "Q.RAW"], d))
    assert "96 x 225 -> 131 x 225 pixels" in r.stdout and "(--width 131)" in r.stdout
    assert np.array_equal(np.fromfile(os.path.join(d, "Q.RAW"), np.uint16).reshape(225, 131), ref.rescale_kind(want, 1, 131, 225, "cubic", valid_min=1))
    # -o with the other extension changes the container, both ways, the same samples
    _ok(_run(["P.RAW", "--width", str(w), "--scale-y", "3/4", "-o", "P.TIFF"], d))
    t = read_tiff_u16(os.path.join(d, "P.TIFF"))[0]
    assert np.array_equal(t.reshape(225, 96), want)
    _ok(_run(["P.TIFF", "--scale", "4", "--valid-min", "0", "-o", "back.RAW"], d))
    assert np.array_equal(np.fromfile(os.path.join(d, "back.RAW"), np.uint16).reshape(900, 384), ref.rescale_kind(want, 1, 384, 900))
    # equal sizes: the input's bytes
    _ok(_run(["P.RAW", "--width", str(w), "--scale", "1", "-o", "same.RAW"], d))
    assert open(os.path.join(d, "same.RAW"), "rb").read() == open(os.path.join(d, "P.RAW"), "rb").read()
    # the input as the output, with or without --force
    r = _run(["P.RAW", "--width", str(w), "--scale", "1", "-o", "P.RAW", "--force"], d)
    assert r.returncode == 2 and "is the input image" in r.stdout + r.stderr
    assert np.array_equal(np.fromfile(os.path.join(d, "P.RAW"), np.uint16).reshape(L, w), img)
