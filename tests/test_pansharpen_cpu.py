"""CPU: the definition of `oip pansharpen` on its numpy restatement (_pansharpen_ref.py) -- the weight table against the cubic in
exact fractions, the int32 bound, what a constant PAN, a band equal to the low-resolution PAN, a zero PAN and a gain limit of 1
give, and the quality condition on seeded scenes --, oip_pansharpen_geometry through capi against the rule, and what the command
refuses before a device is touched."""
import os
import subprocess

import numpy as np
import pytest

import _pansharpen_ref as ref
from _tiff import write_tiff_u16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _smooth12(h, w, seed):
    """12-bit smooth PAN (4h, 4w) and MSS (h, w, 4): the scene of the quality condition"""
    _, P, M = ref.scene(h, w, seed)
    return P, M


def _random16(h, w, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 65536, (4 * h, 4 * w), dtype=np.uint16), rng.integers(0, 65536, (h, w, 4), dtype=np.uint16)


def test_weights_are_the_cubic_times_2048():
    for r, t in enumerate(ref.PHASES):
        c = ref.cubic_weights(t)
        assert [x * 2048 for x in c] == [int(v) for v in ref.WEIGHTS[r]]      # exact: Fraction == int
        assert int(ref.WEIGHTS[r].sum()) == 2048
    # phase r of cell i is the cubic at the pixel centre (4 i + r + 0.5) / 4 - 0.5 = i + (2 r - 3) / 8: its floor is i - 1 for
    # r < 2 and i for r >= 2, the first tap one before it
    for r in range(4):
        pos = ref.Fraction(2 * r - 3, 8)
        fl = pos.numerator // pos.denominator
        assert pos - fl == ref.PHASES[r] and fl - 1 == (-2 if r < 2 else -1)


def test_int32_bound_on_checkerboards():
    """squares of one and of two cells of 0 / 65535: the latter puts 0, 65535, 65535, 0 under the taps, the largest |Hq| there is"""
    worst_hq = worst_acc = 0
    for k in (1, 2):
        yy, xx = np.mgrid[0:16, 0:20]
        for inv in (0, 1):
            src = ((((yy // k) + (xx // k)) & 1) ^ inv) * 65535
            u, hq, acc = ref.upsample(src, extremes=True)
            worst_hq, worst_acc = max(worst_hq, hq), max(worst_acc, acc)
            assert u.min() >= 0 and u.max() <= ref.U_MAX
    assert worst_hq == 616439 and worst_acc <= 616439 * 2768 + 1024 < 2 ** 31
    assert worst_hq < 2 ** 23 and int(np.abs(ref.WEIGHTS).max()) < 2 ** 23    # both operands of every product fit 24 signed bits


@pytest.mark.parametrize("data", [_smooth12, _random16])
def test_constant_pan_gives_the_plain_upsampling(data):
    _, M = data(9, 13, 3)
    for c in (1, 1500, 65535):
        out, (zero, cut) = ref.fuse(np.full((36, 52), c, np.uint16), M)
        assert np.array_equal(out, ref.plain(M)) and zero == 0 and cut == 0


@pytest.mark.parametrize("data", [_smooth12, _random16])
def test_band_equal_to_low_pan_returns_the_pan(data):
    P, M = data(12, 17, 4)
    M = M.copy()
    M[:, :, 2] = ref.box4(P)
    out, (zero, cut) = ref.fuse(P, M)
    UL = ref.upsample(ref.box4(P))
    q = P.astype(np.float32) / np.maximum(UL, 1).astype(np.float32)
    keep = (UL > 0) & (q <= np.float32(0.5))
    print("\npansharpen: %s zero %d cut %d of %d" % (data.__name__, zero, cut, P.size))
    assert zero == 0 and cut == 0 and keep.all()                              # nothing is cut at G = 4 on either data set
    assert np.array_equal(out[:, :, 2][keep], P[keep])


def test_zero_pan_region_has_gain_one():
    P, M = _smooth12(12, 16, 5)
    P = P.copy()
    P[8:40, 12:48] = 0                                                        # MSS cells (2 .. 9, 3 .. 11)
    out, (zero, cut) = ref.fuse(P, M)
    UL = ref.upsample(ref.box4(P))
    assert zero == int((UL == 0).sum()) > 0 and (UL[20:28, 24:36] == 0).all()
    assert np.array_equal(out[UL == 0], ref.plain(M)[UL == 0])
    assert (out[UL == 0] > 0).all()


def test_gain_limit_of_one_cuts():
    P, M = _smooth12(12, 16, 6)
    out1, (_, cut1) = ref.fuse(P, M, G=1)
    out4, (_, cut4) = ref.fuse(P, M, G=4)
    UL = ref.upsample(ref.box4(P))
    was_cut = P.astype(np.float32) / UL.astype(np.float32) > np.float32(0.125)
    assert cut4 == 0 and cut1 == int(was_cut.sum()) > P.size // 4
    assert np.array_equal(out1[was_cut], ref.plain(M)[was_cut])               # a gain of exactly 1
    assert np.array_equal(out1[~was_cut], out4[~was_cut]) and (out1 <= out4).all()


def test_windows_equal_the_whole():
    P, M = _random16(7, 5, 8)
    whole, counts = ref.fuse(P, M, off=0, G=2)
    parts, z, c = [], 0, 0
    for a, n in ((0, 1), (1, 6), (7, 13), (20, 8)):
        o, (zz, cc) = ref.fuse(P, M, G=2, out_row0=a, out_rows=n)
        parts.append(o)
        z, c = z + zz, c + cc
    assert np.array_equal(np.concatenate(parts), whole) and (z, c) == counts


QUALITY = [(24, 32, 1), (40, 28, 2), (33, 47, 3), (16, 16, 4)]


@pytest.mark.parametrize("h,w,seed", QUALITY)
def test_quality_condition(h, w, seed):
    """the fused RMSE against the scene is at most a quarter of the plain up-sampling's, 8 PAN pixels inside the border"""
    T, P, M = ref.scene(h, w, seed)
    out, (zero, cut) = ref.fuse(P, M)
    m = 8
    e_f = np.sqrt(np.mean((out.astype(np.float64) - T)[m:-m, m:-m] ** 2))
    e_p = np.sqrt(np.mean((ref.plain(M).astype(np.float64) - T)[m:-m, m:-m] ** 2))
    print("\npansharpen quality (%d, %d) seed %d: fused rmse %.3f, plain %.3f, ratio %.4f" % (h, w, seed, e_f, e_p, e_f / e_p))
    assert zero == 0 and cut == 0
    assert e_f <= 0.25 * e_p


def test_geometry_entry_point():
    import opticalimageprocessor_amd as oip
    for W, Hp, w, h, off in ((24376, 100000, 6094, 25000, 0), (24376, 100000, 6094, 25000, 7), (16, 4, 4, 1, 0), (16, 9, 4, 5, 1), (16, 9, 4, 1, 5),
                             (16, 9, 4, 5, 5), (16, 400, 4, 20, 0), (16, 9, 4, 5, 6), (20, 9, 4, 5, 0), (16, 3, 4, 5, 0), (16, 9, 4, 5, -1),
                             (0, 9, 0, 5, 0), (16, 9, 4, 0, 0), (15, 9, 4, 5, 0)):
        want = ref.geometry(W, Hp, w, h, off)
        if want is None:
            with pytest.raises(ValueError):
                oip.pansharpen_geometry(W, Hp, w, h, off)
        else:
            assert oip.pansharpen_geometry(W, Hp, w, h, off) == want
    assert ref.geometry(2 * 12288 - 200, 100000, 2 * 3072 - 50, 25000) == (24376, 100000, 25000)


def test_cli_refusals_need_no_device(tmp_path):
    oip = os.path.join(ROOT, "opticalimageprocessor_amd", "lib", "oip")
    d = str(tmp_path)
    rng = np.random.default_rng(2)
    write_tiff_u16(os.path.join(d, "P.TIFF"), rng.integers(0, 4096, (40, 32, 1), dtype=np.uint16))
    write_tiff_u16(os.path.join(d, "M.TIFF"), rng.integers(0, 4096, (10, 8, 4), dtype=np.uint16))
    write_tiff_u16(os.path.join(d, "M9.TIFF"), rng.integers(0, 4096, (10, 9, 4), dtype=np.uint16))
    write_tiff_u16(os.path.join(d, "P4.TIFF"), rng.integers(0, 4096, (40, 32, 4), dtype=np.uint16))
    rng.integers(0, 4096, (40, 32), dtype=np.uint16).tofile(os.path.join(d, "P.RAW"))
    rng.integers(0, 4096, (10, 32), dtype=np.uint16).tofile(os.path.join(d, "M.RAW"))
    open(os.path.join(d, "P.PNG"), "wb").write(b"x" * 64)
    open(os.path.join(d, "there.TIFF"), "wb").write(b"kept")

    def run(args):
        env = dict(os.environ, LOGFILE=os.path.join(d, "oip.log"))
        return subprocess.run([oip, "pansharpen"] + args, cwd=d, env=env, capture_output=True, text=True)
    ok = ["--pan", "P.TIFF", "--mss", "M.TIFF"]
    raw = ["--pan", "P.RAW", "--mss", "M.TIFF", "--width", "32"]
    for args, code, text in (([], 106, "--pan is required"), (ok[:2], 106, "--mss is required"), (ok[2:], 106, "--pan is required"),
                             (["--pan", "missing.TIFF"] + ok[2:], 105, "does not exist"), (ok[:2] + ["--mss", "missing.TIFF"], 105, "does not exist"),
                             (ok + ["--max-gain", "0"], 105, "--max-gain"), (ok + ["--max-gain", "65"], 105, "--max-gain"),
                             (ok + ["--max-gain", "x"], 104, "Could not convert"), (ok + ["--line-offset", "-1"], 105, "--line-offset"),
                             (raw[:4] + ["--width", "0"], 105, "--width"), (ok + ["--levels", "3"], 107, "--levels requires --overviews"),
                             (ok + ["--overviews", "--levels", "17"], 105, "--levels"), (ok + ["--tile", "16"], 109, "--tile"),
                             (["--pan", "P.TIFF", "--mss", "P.TIFF"], 2, "4 samples per pixel expected, not 1"),
                             (["--pan", "P4.TIFF", "--mss", "M.TIFF"], 2, "1 sample per pixel expected, not 4"),
                             (["--pan", "P.TIFF", "--mss", "M9.TIFF"], 2, "not 4 times the MSS line"),
                             (raw[:4] + ["--width", "40"], 2, "not 4 times the MSS line"), (raw[:4] + ["--width", "33"], 2, "file size invalid"),
                             (ok + ["--line-offset", "37"], 2, "fewer than 4"), (ok + ["--line-offset", "40"], 2, "fewer than 4"),
                             (["--pan", "P.TIFF", "--mss", "M.RAW"], 2, "the MSS product is a TIFF"),
                             (["--pan", "P.PNG", "--mss", "M.TIFF"], 2, "only RAW and TIFF image supported"),
                             (ok + ["-o", "there.TIFF"], 2, "--force"), (ok + ["-o", "M.TIFF", "--force"], 2, "is an input image"),
                             (ok + ["-o", "P.TIFF", "--force"], 2, "is an input image"), (ok + ["-o", "out.RAW"], 2, "the output is a TIFF")):
        r = run(args)
        assert r.returncode == code and text in r.stdout + r.stderr, (args, r.returncode, r.stdout + r.stderr)
    assert open(os.path.join(d, "there.TIFF"), "rb").read() == b"kept" and not os.path.exists(os.path.join(d, "M.PSH.TIFF"))
    assert not os.path.exists(os.path.join(d, "out.RAW"))
