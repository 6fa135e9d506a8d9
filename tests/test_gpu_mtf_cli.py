"""GPU: `oip mtf` end to end -- the report's rows, status counts and order statistics are those assembled from the restatement
(_mtf_ref.py) of the input file's samples, on a RAW strip streamed in line blocks of two sizes and in one, on a line range and on
a 4-band TIFF; `--noise REPORT` sets the slack of every band; an image without a usable edge writes no report; and
`oip mtfc --mtf REPORT` writes the bytes of `oip mtfc --mtf-x M --mtf-y M` for the numbers the report holds."""
import os
import subprocess

import numpy as np
import pytest

import _mtf_ref as ref
import opticalimageprocessor_amd as oip
from _tiff import write_tiff_u16

pytestmark = pytest.mark.gpu
OIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "opticalimageprocessor_amd", "lib", "oip")
KW = dict(contrast_min=200, valid_min=1, valid_max=60000)
OPTS = ["--valid-max", "60000", "--tv-slack", str(ref.FIELD_SLACK)]


def _run(tool, args, cwd, **env):
    env = dict(os.environ, LOGFILE=os.path.join(cwd, "oip.log"), **env)
    return subprocess.run([OIP, tool] + args, cwd=cwd, env=env, capture_output=True, text=True)


def _scene(rows, w, seed, spp=1):
    """x cells in the left half of every line, y cells in the right half"""
    h = w // 2
    left, right = ref.field(rows, h, 0, seed, spp), ref.field(rows, w - h, 1, seed + 1, spp)
    return np.concatenate([left.reshape(rows, h, spp), right.reshape(rows, w - h, spp)], axis=1).reshape(rows, w * spp)


def _compare(path, img, spp, axes, slacks, stdout):
    want = ref.report_body(img, spp, axes, slacks, tile_value=oip.mtf_tile, **KW)
    lines = open(path).read().split("\n")
    assert lines[0].startswith("# oip mtf image=") and lines[0].endswith("columns=band,axis,ty,tx,polarity,slope_q,contrast,mtf") and lines[-1] == ""
    assert lines[1:-1] == want
    logged = [ln.split("mtf: ", 1)[1] for ln in stdout.splitlines() if "mtf: band " in ln]
    assert logged == [ln[2:] for ln in want if ln.startswith("# band ")]          # the log carries the same lines
    return want


def _all(path):
    """{axis: {name: text}} of the `# all` lines"""
    out = {}
    for ln in open(path):
        if ln.startswith("# all axis "):
            f = ln.split()
            out[f[3][0]] = dict(zip(f[4::2], f[5::2]))
    return out


def test_raw_strip_in_line_blocks_of_two_sizes_and_mtfc(tmp_path):
    d = str(tmp_path)
    W, L = 512, 400
    img = _scene(L, W, 5)
    img.tofile(os.path.join(d, "P.RAW"))
    base = ["P.RAW", "--width", str(W)] + OPTS
    r = _run("mtf", base, d, OIP_MTF_BLOCK_LINES="70")                  # rounded down to 64: a multiple of 32
    assert r.returncode == 0, r.stdout + r.stderr
    want = _compare(os.path.join(d, "P.MTF.CSV"), img, 1, (0, 1), [ref.FIELD_SLACK], r.stdout)
    assert sum(1 for ln in want if ln[0] != "#") >= 20 and " emptybin 0 " not in want[-1] and " emptybin 0 " not in want[-2]
    for k, hook in enumerate(("96", None)):                             # another block size, and the tool's own (one block)
        r = _run("mtf", base + ["-o", "b%d.csv" % k], d, **({"OIP_MTF_BLOCK_LINES": hook} if hook else {}))
        assert r.returncode == 0, r.stdout + r.stderr
        assert open(os.path.join(d, "b%d.csv" % k)).read() == open(os.path.join(d, "P.MTF.CSV")).read()
    # an existing report: refused, then replaced with --force (one axis, a line range that ends inside a tile)
    r = _run("mtf", base + ["-o", "b0.csv", "--axis", "y"], d)
    assert r.returncode == 2 and "--force" in r.stdout
    r = _run("mtf", base + ["-o", "b0.csv", "--axis", "y", "--line-offset", "64", "--lines", "300", "--force"], d, OIP_MTF_BLOCK_LINES="128")
    assert r.returncode == 0, r.stdout + r.stderr
    _compare(os.path.join(d, "b0.csv"), img[64:364], 1, (1,), [ref.FIELD_SLACK], r.stdout)
    r = _run("mtf", base + ["-o", "x.csv", "--axis", "x"], d)
    assert r.returncode == 0, r.stdout + r.stderr
    _compare(os.path.join(d, "x.csv"), img, 1, (0,), [ref.FIELD_SLACK], r.stdout)
    assert set(_all(os.path.join(d, "x.csv"))) == {"x"}

    # mtfc --mtf: the numbers are the report's, the product is that of --mtf-x / --mtf-y
    al = _all(os.path.join(d, "P.MTF.CSV"))
    for stat in ("median", "p90"):
        mx, my = al["x"][stat], al["y"][stat]
        assert float(mx) == float("%.17g" % float(mx)) and 0 < float(mx) < 1 and 0 < float(my) < 1
        r = _run("mtfc", ["P.RAW", "--width", str(W), "--mtf", "P.MTF.CSV", "-o", "r.RAW", "--force"] + (["--mtf-stat", stat] if stat != "median" else []), d)
        assert r.returncode == 0 and "mtf-x %s, mtf-y %s" % (mx, my) in r.stdout, r.stdout + r.stderr
        r = _run("mtfc", ["P.RAW", "--width", str(W), "--mtf-x", mx, "--mtf-y", my, "-o", "m.RAW", "--force"], d)
        assert r.returncode == 0, r.stdout + r.stderr
        got = open(os.path.join(d, "r.RAW"), "rb").read()
        assert got == open(os.path.join(d, "m.RAW"), "rb").read() and len(got) == img.nbytes
        assert got != img.tobytes()
    # --max-gain still applies: with the gain cut to 1 the filter is the identity
    r = _run("mtfc", ["P.RAW", "--width", str(W), "--mtf", "P.MTF.CSV", "--max-gain", "1", "-o", "g.RAW"], d)
    assert r.returncode == 0 and open(os.path.join(d, "g.RAW"), "rb").read() == img.tobytes(), r.stdout + r.stderr
    # a report of one axis has no value for the other
    r = _run("mtfc", ["P.RAW", "--width", str(W), "--mtf", "x.csv", "-o", "n.RAW"], d)
    assert r.returncode == 105 and "no value for axis y" in r.stdout + r.stderr and not os.path.exists(os.path.join(d, "n.RAW"))


def test_contrast_min_reaches_the_report(tmp_path):
    d = str(tmp_path)
    img = _scene(200, 512, 9)
    img.tofile(os.path.join(d, "P.RAW"))
    r = _run("mtf", ["P.RAW", "--width", "512", "--contrast-min", "1000", "--axis", "x"] + OPTS, d)
    assert r.returncode == 0, r.stdout + r.stderr
    want = ref.report_body(img, 1, (0,), [ref.FIELD_SLACK], tile_value=oip.mtf_tile, **dict(KW, contrast_min=1000))
    assert open(os.path.join(d, "P.MTF.CSV")).read().split("\n")[1:-1] == want
    assert want != ref.report_body(img, 1, (0,), [ref.FIELD_SLACK], tile_value=oip.mtf_tile, **KW)


NOISE_LINE = "# band %d: blocks 9 nodata 0 structured 0 levels 1 a %s b 0 mu_ref 1000 sigma_ref 1 snr_ref 1\n"


def test_tiff_product_and_noise_report(tmp_path):
    """a 4-band LZW TIFF, every channel a scene of its own; then the slack of every band from a noise report: sigma_ref 5 DN gives
    240, at which the tiles planted for a slack of 3200 are TEXTURED, 66.5 DN gives 3192"""
    d = str(tmp_path)
    w, rows, spp = 256, 300, 4
    img = _scene(rows, w, 31, spp)
    write_tiff_u16(os.path.join(d, "A.TIFF"), img.reshape(rows, w, spp), lzw=True, predictor=2, rows_per_strip=16)
    r = _run("mtf", ["A.TIFF"] + OPTS, d)
    assert r.returncode == 0, r.stdout + r.stderr
    want = _compare(os.path.join(d, "A.MTF.CSV"), img, spp, (0, 1), [ref.FIELD_SLACK] * 4, r.stdout)
    assert len({ln.split(":", 1)[1] for ln in want if ln.startswith("# band ") and " axis x" in ln}) == 4          # the channels differ
    r = _run("mtf", ["A.TIFF", "-o", "b.csv"] + OPTS, d, OIP_MTF_BLOCK_LINES="64")
    assert r.returncode == 0 and open(os.path.join(d, "b.csv")).read() == open(os.path.join(d, "A.MTF.CSV")).read(), r.stdout + r.stderr
    sig = (5.0, 66.5, 5.0, 20.0)
    open(os.path.join(d, "n.csv"), "w").write("".join(NOISE_LINE % (b + 1, repr(s * s)) for b, s in enumerate(sig)))
    slacks = [oip.mtf_tv_slack(np.sqrt(s * s + 0.0 * 1000.0)) for s in sig]
    assert slacks == [240, 3192, 240, 960]
    r = _run("mtf", ["A.TIFF", "--valid-max", "60000", "--noise", "n.csv", "-o", "n.mtf.csv"], d)
    assert r.returncode == 0, r.stdout + r.stderr
    got = _compare(os.path.join(d, "n.mtf.csv"), img, spp, (0, 1), slacks, r.stdout)
    assert "tv-slack=noise" in open(os.path.join(d, "n.mtf.csv")).readline()
    assert got != want
    # a report with fewer bands than the image
    open(os.path.join(d, "n1.csv"), "w").write(NOISE_LINE % (1, "25"))
    r = _run("mtf", ["A.TIFF", "--noise", "n1.csv", "-o", "n1.mtf.csv"], d)
    assert r.returncode == 2 and "holds 1 band" in r.stdout and not os.path.exists(os.path.join(d, "n1.mtf.csv")), r.stdout + r.stderr


def test_an_axis_without_a_value_writes_no_report(tmp_path):
    d = str(tmp_path)
    rng = np.random.default_rng(1)
    rng.integers(1, 4096, (96, 256)).astype(np.uint16).tofile(os.path.join(d, "N.RAW"))
    r = _run("mtf", ["N.RAW", "--width", "256"], d)
    assert r.returncode == 2 and "no tile with a value on axis x" in r.stdout and "tiles 45 " in r.stdout, r.stdout + r.stderr
    assert not os.path.exists(os.path.join(d, "N.MTF.CSV"))
    # x cells alone: axis x has values, axis y has none
    ref.field(96, 256, 0, 3).tofile(os.path.join(d, "X.RAW"))
    r = _run("mtf", ["X.RAW", "--width", "256"] + OPTS, d)
    assert r.returncode == 2 and "no tile with a value on axis y" in r.stdout and not os.path.exists(os.path.join(d, "X.MTF.CSV")), r.stdout + r.stderr
    r = _run("mtf", ["X.RAW", "--width", "256", "--axis", "x"] + OPTS, d)
    assert r.returncode == 0 and os.path.exists(os.path.join(d, "X.MTF.CSV")), r.stdout + r.stderr
