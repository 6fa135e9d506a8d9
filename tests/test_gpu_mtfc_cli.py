"""GPU: `oip mtfc` end to end -- the product is the restatement's (_mtfc_ref.py) of the input file's samples, sample for
sample, in the container of the input."""
import os
import re
import subprocess

import numpy as np
import pytest

import _mtfc_ref as ref
from _tiff import read_tags, read_tiff_u16, write_tiff_u16

pytestmark = pytest.mark.gpu
OIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "opticalimageprocessor_amd", "lib", "oip")


def _run(args, cwd, **env):
    env = dict(os.environ, LOGFILE=os.path.join(cwd, "oip.log"), **env)
    return subprocess.run([OIP, "mtfc"] + args, cwd=cwd, env=env, capture_output=True, text=True)


def _strip(W, L, seed, spp=1):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 65536, (L, W * spp), dtype=np.uint16)
    img[rng.random(img.shape) < 0.03] = 0
    img[:, :3 * spp] = 0                                            # a black border as prestitch leaves it
    return img


def test_raw_strip_in_several_line_blocks(tmp_path):
    """96 x 500 through --mtf-x / --mtf-y.  OIP_MTFC_BLOCK_LINES forces line blocks of 64 lines (the tool's own are 64 MiB):
    eight blocks, so both device blocks of either kind are reused, the halo line above and below a block comes from the
    file, and the last block is short.  The default name, then -o, --force and another valid-min."""
    d = str(tmp_path)
    W, L = 96, 500
    img = _strip(W, L, 1)
    img.tofile(os.path.join(d, "P.RRC.RAW"))
    taps = ref.quantise(ref.design3(0.3, 0.45, 2.0))
    base = ["P.RRC.RAW", "--width", str(W), "--mtf-x", "0.3", "--mtf-y", "0.45"]
    r = _run(base, d, OIP_MTFC_BLOCK_LINES="64")
    assert r.returncode == 0, r.stdout + r.stderr
    out = os.path.join(d, "P.RRC.MTFC.RAW")
    want = ref.convolve(img, taps, 1)
    assert np.array_equal(np.fromfile(out, np.uint16).reshape(L, W), want)
    assert not np.array_equal(want, img) and (want[img == 0] == 0).all()
    # the log shows the taps and their sum
    rows = re.findall(r"^ {4}(-?\d+(?: -?\d+)*)$", r.stdout, re.M)
    assert [[int(v) for v in row.split()] for row in rows] == taps.tolist()
    assert "sum |t| = %d" % np.abs(taps).sum() in r.stdout
    # one block gives the same bytes
    r = _run(base + ["-o", "one.RAW"], d)
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(os.path.join(d, "one.RAW"), "rb").read() == open(out, "rb").read()
    # an existing output: refused, then replaced with --force (valid-min 0: another result)
    r = _run(base + ["-o", "one.RAW", "--valid-min", "0"], d)
    assert r.returncode == 2 and "--force" in r.stdout
    assert open(os.path.join(d, "one.RAW"), "rb").read() == want.tobytes()
    with open(os.path.join(d, "one.RAW"), "ab") as f:
        f.write(b"longer than the product")
    r = _run(base + ["-o", "one.RAW", "--valid-min", "0", "--force"], d, OIP_MTFC_BLOCK_LINES="7")
    assert r.returncode == 0, r.stdout + r.stderr
    want0 = ref.convolve(img, taps, 0)
    assert open(os.path.join(d, "one.RAW"), "rb").read() == want0.tobytes() and not np.array_equal(want0, want)


@pytest.mark.parametrize("compress", ["none", "lzw"])
def test_four_sample_tiff_through_a_kernel_file(tmp_path, compress):
    d = str(tmp_path)
    w, rows = 131, 100
    img = _strip(w, rows, 2, 4)
    write_tiff_u16(os.path.join(d, "A.TIFF"), img.reshape(rows, w, 4), lzw=compress == "lzw", predictor=2 if compress == "lzw" else 1,
                   rows_per_strip=16 if compress == "lzw" else None)
    c = np.random.default_rng(5).normal(0, 0.02, (5, 7))
    c[2, 3] += 1.0 - sum(float(v) for v in c.ravel())
    c[2, 3] += 1.0 - sum(float(v) for v in c.ravel())
    ref.write_kernel(os.path.join(d, "k.txt"), c)
    r = _run(["A.TIFF", "--kernel", "k.txt", "--tiff-compress", compress], d)
    assert r.returncode == 0, r.stdout + r.stderr
    out = os.path.join(d, "A.MTFC.TIFF")
    got = read_tiff_u16(out)[0]
    assert got.shape == (rows, w, 4)
    assert np.array_equal(got.reshape(rows, -1), ref.convolve(img, ref.quantise(ref.load_kernel(os.path.join(d, "k.txt"))), 1, 4))
    assert read_tags(out)[259][0] == (5 if compress == "lzw" else 1)   # Compression


def test_one_sample_tiff_and_identity_kernel(tmp_path):
    d = str(tmp_path)
    w, rows = 200, 77
    img = _strip(w, rows, 3)
    write_tiff_u16(os.path.join(d, "S.TIFF"), img)
    open(os.path.join(d, "id.txt"), "w").write("3 3\n0 0 0\n0 1 0\n0 0 0\n")
    r = _run(["S.TIFF", "--kernel", "id.txt", "-o", "same.TIFF"], d)
    assert r.returncode == 0, r.stdout + r.stderr
    assert np.array_equal(read_tiff_u16(os.path.join(d, "same.TIFF"))[0].reshape(rows, w), img)     # the payload of the input
    r = _run(["S.TIFF", "--mtf-x", "0.5", "--mtf-y", "0.5", "--max-gain", "1.5"], d)
    assert r.returncode == 0, r.stdout + r.stderr
    got = read_tiff_u16(os.path.join(d, "S.MTFC.TIFF"))[0].reshape(rows, w)
    assert np.array_equal(got, ref.convolve(img, ref.quantise(ref.design3(0.5, 0.5, 1.5)), 1))
    # a RAW strip through the identity kernel is the input's bytes
    img.tofile(os.path.join(d, "S.RAW"))
    r = _run(["S.RAW", "--width", str(w), "--kernel", "id.txt"], d)
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(os.path.join(d, "S.MTFC.RAW"), "rb").read() == img.tobytes()


def test_halo_larger_than_the_block_and_every_way_to_cut_a_small_strip(tmp_path):
    """96 x 23 through a 9 x 9 kernel file: four halo lines either side.  OIP_MTFC_BLOCK_LINES 1 and 2 make the halo larger than
    the block, reuse every device block many times and clamp the halo at both ends of the strip; 23 is exactly one block; 24 is
    larger than the strip, so no second block is allocated.  However the strip is cut, the product is the restatement's."""
    d = str(tmp_path)
    W, L = 96, 23
    img = _strip(W, L, 7)
    img.tofile(os.path.join(d, "P.RAW"))
    c = np.random.default_rng(8).normal(0, 0.01, (9, 9))
    c[4, 4] += 1.0 - sum(float(v) for v in c.ravel())
    c[4, 4] += 1.0 - sum(float(v) for v in c.ravel())
    ref.write_kernel(os.path.join(d, "k.txt"), c)
    taps = ref.quantise(ref.load_kernel(os.path.join(d, "k.txt")))
    assert taps.shape == (9, 9) and np.count_nonzero(taps[0]) and np.count_nonzero(taps[8])
    want = ref.convolve(img, taps, 1).tobytes()
    products = []
    for lines in (1, 2, 23, 24):
        r = _run(["P.RAW", "--width", str(W), "--kernel", "k.txt", "-o", "b%d.RAW" % lines], d, OIP_MTFC_BLOCK_LINES=str(lines))
        assert r.returncode == 0, r.stdout + r.stderr
        products.append(open(os.path.join(d, "b%d.RAW" % lines), "rb").read())
        assert products[-1] == want, "blocks of %d lines" % lines
    assert all(p == products[0] for p in products)
