"""GPU: `oip regcheck` end to end.  The report's tiles and summary are parsed and compared with what the restatement
(_regcheck_ref.py) gives for the same planes and grid: positions and flags exactly, dx and dy within 1e-4 and the score within
1e-6 -- the resolutions they are printed at (%.4f, %.6f), not measured tolerances."""
import os
import subprocess

import numpy as np
import pytest

import _regcheck_ref as ref
from _tiff import write_tiff_u16

pytestmark = pytest.mark.gpu
OIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "opticalimageprocessor_amd", "lib", "oip")


def _run(args, cwd):
    env = dict(os.environ, LOGFILE=os.path.join(cwd, "oip.log"))
    return subprocess.run([OIP, "regcheck"] + args, cwd=cwd, env=env, capture_output=True, text=True)


def _parse(path):
    """-> (first line, tiles (n, 6) float64, summary (8,), the summary sentence)"""
    lines = open(path).read().splitlines()
    assert lines[0].startswith("# oip regcheck ") and lines[0].endswith("columns=x,y,dx,dy,score,flags")
    body = [l for l in lines[1:] if not l.startswith("#")]
    tail = [l for l in lines[1:] if l.startswith("#")]
    assert lines[1:] == body + tail and len(tail) == 3 and tail[1] == "# count,mean_dx,mean_dy,std_dx,std_dy,rms,ce90,max"
    for l in body:
        x, y, dx, dy, sc, fl = l.split(",")
        assert len(dx.split(".")[1]) == 4 and len(dy.split(".")[1]) == 4 and len(sc.split(".")[1]) == 6 and "." not in x + y + fl
    tiles = np.array([[float(v) for v in l.split(",")] for l in body])
    return lines[0], tiles, np.array([float(v) for v in tail[2][2:].split(",")]), tail[0][2:]


def _expect(A, B, T, S, step, origin=(0, 0), scale=1, min_score=0.5, valid=(1, 65535)):
    """tiles (n, 6) and summary (8,) of planes A, B (the overlap of the two images) by the restatement"""
    h, w = A.shape
    x0, y0, nx, ny = ref.grid(w, h, T, S, step)
    recs, _, gap = ref.match_tiles(A, B, T, S, x0, y0, step, step, nx, ny, *valid)
    assert gap.min() > 1e-9
    rows = []
    for t, r in enumerate(recs):
        dx, dy, sc, fl = ref.peak(r, T, S, min_score)
        j, i = divmod(t, nx)
        rows.append(((origin[0] + x0 + i * step + T // 2) * scale, (origin[1] + y0 + j * step + T // 2) * scale, dx, dy, sc, fl))
    rows = np.array(rows, np.float64)
    return rows, ref.summary(rows[:, 2], rows[:, 3], rows[:, 5].astype(int))


def _check(path, want, wsum, stdout=None):
    first, tiles, summ, sentence = _parse(path)
    assert tiles.shape == want.shape
    assert np.array_equal(tiles[:, [0, 1, 5]], want[:, [0, 1, 5]])
    assert np.abs(tiles[:, 2:4] - want[:, 2:4]).max() <= 1e-4 and np.abs(tiles[:, 4] - want[:, 4]).max() <= 1e-6
    assert summ[0] == wsum[0] and np.abs(summ[1:] - wsum[1:]).max() <= 1e-6
    assert sentence.startswith("tiles %d, used %d " % (len(want), wsum[0]))
    if stdout is not None:
        assert "regcheck: " + sentence in stdout
    return first


def test_bands_of_one_tiff(tmp_path):
    """a 4-sample TIFF whose bands are shifted copies of one texture: band 3 against band 1 with --tile 16 --search 3 --step 8, the
    shift found; the default output name, an existing report kept without --force and replaced with it; -o"""
    d = str(tmp_path)
    h, w = 90, 120
    shifts = [(0, 0), (1, -1), (2, 1), (-2, 2)]
    bands = [ref.pair(h, w, s, 40)[1] for s in shifts]
    write_tiff_u16(os.path.join(d, "M.TIFF"), np.stack(bands, axis=2))
    base = ["--image1", "M.TIFF", "--tile", "16", "--search", "3", "--step", "8"]
    r = _run(base + ["--band1", "1", "--band2", "3"], d)
    assert r.returncode == 0, r.stdout + r.stderr
    out = os.path.join(d, "M.REG.CSV")
    want, wsum = _expect(bands[0], bands[2], 16, 3, 8)
    first = _check(out, want, wsum, r.stdout)
    assert "band1=1 band2=3" in first and "tile=16 search=3 step=8" in first and "image2=M.TIFF" in first
    assert wsum[0] == len(want) and abs(wsum[1] - 2.0) < 0.3 and abs(wsum[2] - 1.0) < 0.3          # every tile used, the shift found
    # another pair: refused while the report exists, written with --force
    before = open(out).read()
    r = _run(base + ["--band1", "2", "--band2", "4"], d)
    assert r.returncode == 2 and "--force" in r.stdout and open(out).read() == before
    r = _run(base + ["--band1", "2", "--band2", "4", "--force"], d)
    assert r.returncode == 0, r.stdout + r.stderr
    want24, wsum24 = _expect(bands[1], bands[3], 16, 3, 8)
    _check(out, want24, wsum24)
    # (-3, 3) lies on the border of the search range: every tile is flagged EDGE, none enters the summary
    assert (want24[:, 2] == -3.0).all() and (want24[:, 3] == 3.0).all() and (want24[:, 5].astype(int) == ref.EDGE).all() and not wsum24.any()
    # -o, the defaults of --tile / --search / --step, --min-score
    r = _run(["--image1", "M.TIFF", "--band1", "1", "--band2", "2", "-o", "named.csv", "--min-score", "0.99"], d)
    assert r.returncode == 0, r.stdout + r.stderr
    want12, wsum12 = _expect(bands[0], bands[1], 64, 4, 64, min_score=0.99)
    _check(os.path.join(d, "named.csv"), want12, wsum12)
    assert len(want12) == 1
    # a band the file does not have, an image that holds no tile
    write_tiff_u16(os.path.join(d, "P.TIFF"), bands[0][:, :, None])
    r = _run(["--image1", "P.TIFF", "--band1", "2"], d)
    assert r.returncode == 254 and "--band1: band index out of range (1..1)" in r.stdout
    r = _run(["--image1", "P.TIFF", "--tile", "128", "-o", "none.csv"], d)
    assert r.returncode == 2 and "holds no tile" in r.stdout and not os.path.exists(os.path.join(d, "none.csv"))


def test_two_raw_strips_with_shift_x(tmp_path):
    """the CCD overlap: image 2 begins at column W - fold of image 1 and is displaced by (1, -2) on top; only the overlap is
    matched, x counts in image-1 columns; then both shifts, one of them negative; images that do not meet are refused"""
    d = str(tmp_path)
    h, w1, w2, fold = 100, 150, 140, 60
    X, Y = ref.pair(h, w1 + w2, (1, -2), 41)
    A, B = np.ascontiguousarray(X[:, :w1]), np.ascontiguousarray(Y[:, w1 - fold:w1 - fold + w2])
    A.tofile(os.path.join(d, "L.RAW"))
    B.tofile(os.path.join(d, "R.RAW"))
    args = ["--image1", "L.RAW", "--image2", "R.RAW", "--width", str(w1), "--width2", str(w2), "--tile", "24", "--search", "4", "--step", "12"]
    r = _run(args + ["--shift-x", str(w1 - fold)], d)
    assert r.returncode == 0, r.stdout + r.stderr
    want, wsum = _expect(A[:, w1 - fold:], B[:, :fold], 24, 4, 12, origin=(w1 - fold, 0))
    first = _check(os.path.join(d, "L.REG.CSV"), want, wsum, r.stdout)
    assert "shift-x=%d" % (w1 - fold) in first and wsum[0] == len(want) and abs(wsum[1] - 1.0) < 0.3 and abs(wsum[2] + 2.0) < 0.3
    assert want[:, 0].min() == w1 - fold + 4 + 12
    # both shifts, one negative (the overlap starts on line 1 of image 2); 2 columns and 1 line off, which the result shows
    r = _run(args + ["--shift-x", str(w1 - fold - 2), "--shift-y", "-1", "-o", "neg.csv"], d)
    assert r.returncode == 0, r.stdout + r.stderr
    ax = w1 - fold - 2
    want, wsum = _expect(A[:h - 1, ax:], B[1:, :w1 - ax], 24, 4, 12, origin=(ax, 0))
    _check(os.path.join(d, "neg.csv"), want, wsum)
    assert abs(wsum[1] + 1.0) < 0.3 and abs(wsum[2] + 3.0) < 0.3
    # images that do not meet
    r = _run(args + ["--shift-x", str(w1), "-o", "apart.csv"], d)
    assert r.returncode == 2 and "holds no tile" in r.stdout


def test_scale_2(tmp_path):
    """image 1 at twice the size (every sample a 2 x 2 block, whose box mean is the sample): --scale 2 matches its decimation
    against image 2; x and y count in image-1 pixels.  Image 1 as a 4-sample TIFF, whose decimation is one plane per band."""
    d = str(tmp_path)
    h, w = 80, 100
    A, B = ref.pair(h, w, (-1, 2), 42)
    C, _ = ref.pair(h, w, (0, 0), 43)
    big = [np.kron(p, np.ones((2, 2), np.uint16)) for p in (C, A, C, C)]
    write_tiff_u16(os.path.join(d, "BIG.TIFF"), np.stack(big, axis=2))
    B.tofile(os.path.join(d, "B.RAW"))
    r = _run(["--image1", "BIG.TIFF", "--band1", "2", "--image2", "B.RAW", "--width2", str(w), "--scale", "2", "--tile", "32", "--search", "3",
              "--step", "16"], d)
    assert r.returncode == 0, r.stdout + r.stderr
    want, wsum = _expect(A, B, 32, 3, 16, scale=2)
    first = _check(os.path.join(d, "BIG.REG.CSV"), want, wsum, r.stdout)
    assert "scale=2" in first and wsum[0] == len(want) and abs(wsum[1] + 1.0) < 0.3 and abs(wsum[2] - 2.0) < 0.3
    assert want[0, 0] == (3 + 16) * 2
