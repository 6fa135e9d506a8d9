"""GPU: `oip stitch --balance / --feather` end to end -- the product is the restatement's (_seam_ref.py) of the files'
contents, sample for sample, the logged gains are the restatement's, and without the options the tool writes what it wrote
before."""
import os
import re
import subprocess

import numpy as np
import pytest

import _seam_ref as ref
from _tiff import read_tiff_u16, write_tiff_u16

pytestmark = pytest.mark.gpu
OIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "opticalimageprocessor_amd", "lib", "oip")
W, L, FOLD = 1280, 1000, 50                                         # --fold-cols 100


def _run(args, cwd):
    env = dict(os.environ, LOGFILE=os.path.join(cwd, "oip.log"))
    return subprocess.run([OIP, "stitch"] + args, cwd=cwd, env=env, capture_output=True, text=True)


def _logged(stdout):
    """[(channel, n, gain_q16, offset_q16, identity substituted)] of the log's per-channel lines, in order"""
    return [(int(c), int(n), int(g), int(o), bool(i)) for c, n, g, o, i in
            re.findall(r"seam channel (\d+): n (\d+), .*? gain_q16 (-?\d+), offset_q16 (-?\d+)( \(identity substituted\))?", stdout)]


@pytest.fixture(scope="module")
def raw_pair(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("seam"))
    left, right = ref.build_pair(W, L, FOLD, 1.2, 12.0, 11)
    left.tofile(os.path.join(d, "L.RAW"))
    right.tofile(os.path.join(d, "R.RAW"))
    return d, left, right


def test_raw_moments_feather(raw_pair):
    d, left, right = raw_pair
    base = ["--image1", "L.RAW", "--image2", "R.RAW", "--fold-cols", str(2 * FOLD), "--width", str(W)]
    r = _run(base + ["--balance", "moments", "--feather", "8", "-o", "balanced.RAW"], d)
    assert r.returncode == 0, r.stdout + r.stderr
    acc = ref.moments(left, right, FOLD, 1, 1, 65535)
    G, O, ident, _ = ref.fit(acc, "moments", 0)
    assert _logged(r.stdout) == [(1, int(acc[0, 0]), G[0], O[0], False)]
    assert open(os.path.join(d, "oip.log")).read().count("seam channel 1:") == 1
    got = np.fromfile(os.path.join(d, "balanced.RAW"), np.uint16).reshape(L, 2 * (W - FOLD))
    assert np.array_equal(got, ref.stitch(left, right, FOLD, 1, G, O, 4, 1))
    # what it is for: the step across the seam.  Columns just left and just right of the blend zone (h = 4)
    s, h = W - FOLD, 4
    step_in = abs(left[:, s - h - 1].mean() - right[:, s + h - (W - 2 * FOLD)].mean())
    step_out = abs(got[:, s - h - 1].mean() - got[:, s + h].mean())
    assert step_out < step_in, "column means across the seam differ by %.2f DN in the product, %.2f DN in the inputs" % (step_out, step_in)
    assert step_in > 200 and step_out < 150, (step_in, step_out)    # 352 DN by construction; the rest is the scene's own noise
    # RAW in, TIFF out takes the same path
    r = _run(base + ["--balance", "moments", "--feather", "8", "-o", "balanced.TIFF"], d)
    assert r.returncode == 0, r.stdout + r.stderr
    assert np.array_equal(read_tiff_u16(os.path.join(d, "balanced.TIFF"))[0], got)


def test_default_path_is_untouched(raw_pair):
    d, left, right = raw_pair
    base = ["--image1", "L.RAW", "--image2", "R.RAW", "--fold-cols", str(2 * FOLD), "--width", str(W)]
    r0 = _run(base + ["-o", "plain.RAW"], d)
    r1 = _run(base + ["--balance", "none", "--feather", "0", "-o", "none.RAW"], d)
    assert r0.returncode == 0 and r1.returncode == 0, r0.stdout + r1.stdout
    a = open(os.path.join(d, "plain.RAW"), "rb").read()
    assert a == open(os.path.join(d, "none.RAW"), "rb").read()
    assert a == np.concatenate([left[:, :W - FOLD], right[:, FOLD:]], 1).tobytes()
    assert not _logged(r0.stdout) and not _logged(r1.stdout)
    # feathering alone: no fit, no log line, identity gains
    r2 = _run(base + ["--feather", "20", "-o", "feather.RAW"], d)
    assert r2.returncode == 0 and not _logged(r2.stdout)
    got = np.fromfile(os.path.join(d, "feather.RAW"), np.uint16).reshape(L, 2 * (W - FOLD))
    assert np.array_equal(got, ref.stitch(left, right, FOLD, 1, [65536], [0], 10, 1))


def test_four_sample_tiffs_gain_per_channel(tmp_path):
    w, rows, fold = 96, 120, 8
    d = str(tmp_path)
    left, right = ref.build_pair(w, rows, fold, [1.07, 0.93, 1.2, 0.8], 0.0, 21, 4)
    write_tiff_u16(os.path.join(d, "A.TIFF"), left.reshape(rows, w, 4))
    write_tiff_u16(os.path.join(d, "B.TIFF"), right.reshape(rows, w, 4), lzw=True, predictor=2, rows_per_strip=16)
    r = _run(["--image1", "A.TIFF", "--image2", "B.TIFF", "--fold-cols", str(2 * fold), "--balance", "gain", "--feather", "4", "-o", "S.TIFF"], d)
    assert r.returncode == 0, r.stdout + r.stderr
    acc = ref.moments(left, right, fold, 4, 1, 65535)
    G, O, ident, _ = ref.fit(acc, "gain", 0)
    assert _logged(r.stdout) == [(c + 1, int(acc[0, c]), G[c], 0, False) for c in range(4)]
    assert len(set(G)) == 4                                         # precondition: the channels' gains differ
    got = read_tiff_u16(os.path.join(d, "S.TIFF"))[0]
    assert got.shape == (rows, 2 * (w - fold), 4)
    assert np.array_equal(got.reshape(rows, -1), ref.stitch(left, right, fold, 4, G, O, 2, 1))
