"""GPU: `oip overviews` and `oip stitch --overviews` end to end -- the overview file holds the restatement's pyramid
(_overview_ref.py) of the image's samples, level for level, in chained reduced-resolution directories; it is the same file
however the strip was cut into blocks and whoever encoded its strips; and a stitch with --overviews writes the product it
writes without."""
import os
import subprocess

import numpy as np
import pytest

import _overview_ref as ref
import _seam_ref
from _tiff import read_tiff_u16, write_tiff_u16

pytestmark = pytest.mark.gpu
OIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "opticalimageprocessor_amd", "lib", "oip")


def _run(args, cwd, tool="overviews", **env):
    env = dict(os.environ, LOGFILE=os.path.join(cwd, "oip.log"), **env)
    return subprocess.run([OIP, tool] + args, cwd=cwd, env=env, capture_output=True, text=True)


def _noise(h, n, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(1, 4096, (h, n)).astype(np.uint16)
    x[rng.random(x.shape) < 0.30] = 0
    x[rng.random(x.shape) < 0.02] = 65535
    return x


def _bytes(path):
    with open(path, "rb") as f:
        return f.read()


def test_raw_strip_levels_blocks_and_refusals(tmp_path):
    """40 x 70 RAW, --levels 3: every level is the restatement's, under the default name beside the image; line blocks of 6
    lines (OIP_OVERVIEWS_BLOCK_LINES; the tool's own are 64 MiB) give the identical file, an odd hook is rounded down; BigTIFF;
    an existing output is kept without --force and replaced with it; what OverviewsCheck refuses"""
    d = str(tmp_path)
    W, L = 40, 70
    img = _noise(L, W, 1)
    img.tofile(os.path.join(d, "P.RAW"))
    base = ["P.RAW", "--width", str(W), "--levels", "3"]
    r = _run(base, d)
    assert r.returncode == 0, r.stdout + r.stderr
    out = os.path.join(d, "P.RAW.ovr")
    want = ref.pyramid(img, 3, 1)
    ref.assert_is_pyramid(out, want, 1, big=False, compression=1)
    for k, lv in enumerate(want):
        assert "level %d: %d x %d x 1" % (k + 1, lv.shape[1], lv.shape[0]) in r.stdout
    assert "%d bytes in " % img.nbytes in r.stdout
    for lines in ("6", "7", "2"):
        r = _run(base + ["-o", "b%s.ovr" % lines], d, OIP_OVERVIEWS_BLOCK_LINES=lines)
        assert r.returncode == 0, r.stdout + r.stderr
        assert _bytes(os.path.join(d, "b%s.ovr" % lines)) == _bytes(out), lines
    # the default level count: a level that fits 256 x 256 is the first already
    r = _run(["P.RAW", "--width", str(W), "-o", "default.ovr", "--valid-min", "0"], d)
    assert r.returncode == 0, r.stdout + r.stderr
    ref.assert_is_pyramid(os.path.join(d, "default.ovr"), ref.pyramid(img, 1, 0), 1)
    # BigTIFF
    r = _run(base + ["-o", "big.ovr"], d, OIP_TIFF_FORCE_BIG="1")
    assert r.returncode == 0, r.stdout + r.stderr
    ref.assert_is_pyramid(os.path.join(d, "big.ovr"), want, 1, big=True)
    # an existing output: refused and untouched, then replaced with --force (valid-min 300: another result)
    r = _run(base + ["--valid-min", "300"], d)
    assert r.returncode == 2 and "--force" in r.stdout
    assert _bytes(out) == _bytes(os.path.join(d, "b6.ovr"))
    with open(out, "ab") as f:
        f.write(b"longer than the pyramid")
    r = _run(base + ["--valid-min", "300", "--force"], d)
    assert r.returncode == 0, r.stdout + r.stderr
    want300 = ref.pyramid(img, 3, 300)
    ref.assert_is_pyramid(out, want300, 1)
    assert not np.array_equal(want300[0], want[0])
    # refusals, before a device is touched: the container, a RAW that is not whole lines, the ranges, an output that is the input
    open(os.path.join(d, "P.PNG"), "wb").write(b"x" * 80)
    r = _run(["P.PNG"], d)
    assert r.returncode == 2 and "only RAW and TIFF image supported" in r.stdout
    r = _run(["P.RAW", "--width", "41"], d)
    assert r.returncode == 2 and "file size invalid" in r.stdout
    for bad in (["--levels", "0"], ["--levels", "17"], ["--valid-min", "-1"], ["--valid-min", "65536"]):
        r = _run(base[:3] + bad + ["-o", "never.ovr"], d)
        assert r.returncode == 105, (bad, r.stdout + r.stderr)
    r = _run(base + ["-o", "P.RAW", "--force"], d)
    assert r.returncode == 2 and "is the input image" in r.stdout
    assert _bytes(os.path.join(d, "P.RAW")) == img.tobytes() and not os.path.exists(os.path.join(d, "never.ovr"))
    r = _run(["missing.RAW"], d)
    assert r.returncode == 105
    r = _run(base + ["--bil"], d)
    assert r.returncode == 109                                     # there is no BIL mode: a BIL line would mix bands


def test_four_sample_tiff_device_and_host_lzw(tmp_path):
    """a 36 x 50 LZW TIFF of 4 samples: the levels are LZW with predictor 2 as the product is; the device encoder and the host's
    (OIP_TIFF_GPU_LZW=0) write the same file; --tiff-compress none writes the levels uncompressed"""
    d = str(tmp_path)
    w, h = 36, 50
    img = _noise(h, w * 4, 2)
    write_tiff_u16(os.path.join(d, "M.TIFF"), img.reshape(h, w, 4), lzw=True, predictor=2, rows_per_strip=7)
    want = ref.pyramid(img, 3, 1, 4)
    r = _run(["M.TIFF", "--levels", "3"], d)
    assert r.returncode == 0, r.stdout + r.stderr
    out = os.path.join(d, "M.TIFF.ovr")
    dirs = ref.assert_is_pyramid(out, want, 4, big=False, compression=5)
    assert all(e["tags"][317] == [2] and e["tags"][338] == [2] for e in dirs)
    r = _run(["M.TIFF", "--levels", "3", "-o", "host.ovr"], d, OIP_TIFF_GPU_LZW="0")
    assert r.returncode == 0, r.stdout + r.stderr
    ref.assert_is_pyramid(os.path.join(d, "host.ovr"), want, 4, compression=5)
    assert _bytes(os.path.join(d, "host.ovr")) == _bytes(out)
    r = _run(["M.TIFF", "--levels", "3", "-o", "big.ovr"], d, OIP_TIFF_FORCE_BIG="1")
    assert r.returncode == 0, r.stdout + r.stderr
    ref.assert_is_pyramid(os.path.join(d, "big.ovr"), want, 4, big=True, compression=5)
    r = _run(["M.TIFF", "--levels", "2", "-o", "plain.ovr", "--tiff-compress", "none"], d)
    assert r.returncode == 0, r.stdout + r.stderr
    ref.assert_is_pyramid(os.path.join(d, "plain.ovr"), want[:2], 4, compression=1)
    # a one-sample TIFF
    write_tiff_u16(os.path.join(d, "G.TIFF"), img[:, :37])
    r = _run(["G.TIFF", "--levels", "2", "--valid-min", "0"], d)
    assert r.returncode == 0, r.stdout + r.stderr
    ref.assert_is_pyramid(os.path.join(d, "G.TIFF.ovr"), ref.pyramid(img[:, :37], 2, 0), 1, compression=1)


@pytest.mark.parametrize("seam", [[], ["--balance", "moments", "--feather", "4"]])
@pytest.mark.parametrize("ext", ["RAW", "TIFF"])
def test_stitch_overviews(tmp_path, seam, ext):
    """two 64 x 40 RAW images, --overviews --levels 2: <output>.ovr is the pyramid of the product the same command wrote, and
    that product is byte for byte the one written without --overviews; an .ovr that exists is replaced with its product"""
    d = str(tmp_path)
    W, L = 64, 40
    left, right = _seam_ref.build_pair(W, L, 4, 1.1, 9.0, 3)           # one scene seen by two detectors: the overlaps show the same ground
    for img, name in ((left, "L.RAW"), (right, "R.RAW")):
        img[np.random.default_rng(4).random(img.shape) < 0.2] = 0   # no data in both, so that blocks without data occur
        img.tofile(os.path.join(d, name))
    base = ["--image1", "L.RAW", "--image2", "R.RAW", "--fold-cols", "8", "--width", str(W)] + seam
    r = _run(base + ["-o", "plain." + ext], d, tool="stitch")
    assert r.returncode == 0, r.stdout + r.stderr
    assert not os.path.exists(os.path.join(d, "plain.%s.ovr" % ext))
    open(os.path.join(d, "S.%s.ovr" % ext), "wb").write(b"stale")
    r = _run(base + ["-o", "S." + ext, "--overviews", "--levels", "2"], d, tool="stitch")
    assert r.returncode == 0, r.stdout + r.stderr
    assert _bytes(os.path.join(d, "S." + ext)) == _bytes(os.path.join(d, "plain." + ext))
    ow = 2 * (W - 4)
    if ext == "RAW":
        product = np.fromfile(os.path.join(d, "S.RAW"), np.uint16).reshape(L, ow)
    else:
        product = read_tiff_u16(os.path.join(d, "S.TIFF"))[0]
    assert product.shape == (L, ow)
    ref.assert_is_pyramid(os.path.join(d, "S.%s.ovr" % ext), ref.pyramid(product, 2, 1), 1, compression=1)
    # --levels belongs to --overviews; the seam options' --valid-min is the pyramid's
    r = _run(base + ["-o", "T." + ext, "--levels", "2"], d, tool="stitch")
    assert r.returncode == 107
    r = _run(base + ["-o", "T." + ext, "--overviews", "--valid-min", "300"], d, tool="stitch")
    assert r.returncode == 0, r.stdout + r.stderr
    if ext == "RAW":
        product = np.fromfile(os.path.join(d, "T.RAW"), np.uint16).reshape(L, ow)
    else:
        product = read_tiff_u16(os.path.join(d, "T.TIFF"))[0]
    ref.assert_is_pyramid(os.path.join(d, "T.%s.ovr" % ext), ref.pyramid(product, 1, 300), 1)


def test_stitch_overviews_of_four_sample_tiffs(tmp_path):
    """two 4-sample TIFFs with a band map: the levels are in the product's on-disk sample order"""
    d = str(tmp_path)
    w, h = 24, 30
    for name, seed in (("A.TIFF", 5), ("B.TIFF", 6)):
        write_tiff_u16(os.path.join(d, name), _noise(h, w * 4, seed).reshape(h, w, 4), lzw=True, predictor=2, rows_per_strip=5)
    for tag, extra in (("n", []), ("g", ["--GDAL", "--band-map", "4,1,3,2"])):
        r = _run(["--image1", "A.TIFF", "--image2", "B.TIFF", "--fold-cols", "4", "-o", tag + ".TIFF", "--overviews", "--levels", "2"] + extra, d,
                 tool="stitch")
        assert r.returncode == 0, r.stdout + r.stderr
        product = read_tiff_u16(os.path.join(d, tag + ".TIFF"))[0]
        assert product.shape == (h, 2 * (w - 2), 4)
        ref.assert_is_pyramid(os.path.join(d, tag + ".TIFF.ovr"), ref.pyramid(product.reshape(h, -1), 2, 1, 4), 4, compression=5)
