"""CPU suite: the host side of `oip mtfc` -- the restatement itself on cases worked by hand, the three functions that make
the taps (oip_mtfc_design3, oip_mtfc_quantise, oip_mtfc_load_kernel) against their restatements bit for bit, and the argument
surface of the sub-command.  Nothing here touches a GPU."""
import os
import subprocess

import numpy as np
import pytest

import opticalimageprocessor_amd as oip
import _mtfc_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OIP = os.path.join(ROOT, "opticalimageprocessor_amd", "lib", "oip")


def _run(args, cwd):
    env = dict(os.environ, LOGFILE=os.path.join(cwd, "oip.log"))
    return subprocess.run([OIP, "mtfc"] + args, cwd=cwd, env=env, capture_output=True, text=True)


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def test_restatement_hand_worked_3x3():
    """out(y, x) = (-256 s(y-1, x-1) + 4864 s(y, x) - 512 s(y, x+1) + 2048) >> 12 with the border replicated, the zero in the
    middle passing through and standing in as the centre where it is a neighbour.  E.g. (0, 1): -256 * 100 + 4864 * 200
    - 512 * 300 + 2048 = 795648 = 194.25 * 4096; (1, 0): the right neighbour is no data, so -256 * 100 + 4864 * 400
    - 512 * 400 + 2048 = 1717248 = 419.25 * 4096."""
    img = np.array([[100, 200, 300], [400, 0, 600], [700, 800, 900]], np.uint16)
    taps = np.array([[-256, 0, 0], [0, 4864, -512], [0, 0, 0]])
    want = np.array([[88, 194, 306], [419, 0, 625], [706, 813, 900]], np.uint16)
    assert np.array_equal(ref.convolve(img, taps, 1), want)
    # flipped or transposed taps give something else: the case tells correlation from convolution
    assert not np.array_equal(ref.convolve(img, taps[::-1, ::-1], 1), want) and not np.array_equal(ref.convolve(img, taps.T, 1), want)
    # valid_min 0: the zero is data -- it is filtered and enters its neighbours' sums
    z = ref.convolve(img, taps, 0)
    assert z[1, 1] == 0 and z[1, 0] == (-256 * 100 + 4864 * 400 + 2048) >> 12 and z[2, 2] == (4864 * 900 - 512 * 900 + 2048) >> 12


def test_restatement_clamps_and_four_samples():
    img = np.full((4, 5), 65535, np.uint16)
    assert (ref.convolve(img, np.array([[32767]]), 1) == 65535).all()             # 32767 * 65535 + 2048 < 2^31, clamped above
    assert (ref.convolve(img, np.array([[-32767]]), 1) == 1).all()                # negative: clamped to valid_min
    assert (ref.convolve(img, np.array([[-32767]]), 0) == 0).all()
    # 4 samples per pixel: a horizontal neighbour is 4 samples away, channels never mix
    rng = np.random.default_rng(3)
    px = rng.integers(1, 65536, (6, 7, 4), dtype=np.uint16)
    taps = ref.random_taps(3, 5, 1, 9000)
    got = ref.convolve(px.reshape(6, 28), taps, 1, 4).reshape(6, 7, 4)
    for c in range(4):
        assert np.array_equal(got[:, :, c], ref.convolve(px[:, :, c], taps, 1, 1))


@pytest.mark.parametrize("shape,spp", [((5, 7), 1), ((1, 9), 1), ((9, 1), 1), ((6, 16), 4)])
def test_restatement_identity(shape, spp):
    rng = np.random.default_rng(shape[0])
    img = rng.integers(0, 65536, shape, dtype=np.uint16)
    for ky, kx in [(1, 1), (3, 3), (9, 5)]:
        taps = np.zeros((ky, kx), np.int64)
        taps[ky // 2, kx // 2] = 4096
        assert np.array_equal(ref.convolve(img, taps, 1, spp), img)


# ---- the taps -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mx,my,g", [(0.25, 0.4, 2.0), (1.0, 1.0, 1.0), (0.1, 0.1, 2.8), (0.7, 0.6, 2.0), (0.3, 0.9, 1.5)])
def test_design3_bit_for_bit(mx, my, g):
    got, want = oip.mtfc_design3(mx, my, g), ref.design3(mx, my, g)
    assert got.tobytes() == want.tobytes()
    assert np.array_equal(oip.mtfc_quantise(got), ref.quantise(want))
    assert oip.mtfc_quantise(got).sum() == 4096


def test_design3_values():
    assert np.array_equal(oip.mtfc_design3(1.0, 1.0, 1.0), [[0, 0, 0], [0, 1, 0], [0, 0, 0]])
    c = oip.mtfc_design3(0.25, 0.4, 2.0)                           # both axes limited by max_gain: a = 0.25 on either
    assert np.array_equal(c, np.outer([-0.25, 1.5, -0.25], [-0.25, 1.5, -0.25]))
    c = oip.mtfc_design3(0.5, 0.8, 4.0)                            # x: g = 2, a = 0.25; y: g = 1.25, a = 0.0625
    assert np.array_equal(c, np.outer([-0.0625, 1.125, -0.0625], [-0.25, 1.5, -0.25]))


def test_quantise_bound():
    """(0.1, 0.1, 2.8): sum |c| = 2.8^2 = 7.84, sum |t| about 7.84 * 4096 = 32113, just inside 32767; at max_gain 3 it is
    9 * 4096 = 36864 and the taps are refused"""
    t = oip.mtfc_quantise(oip.mtfc_design3(0.1, 0.1, 2.8))
    assert 32000 < np.abs(t).sum() <= 32767 and np.array_equal(t, ref.quantise(ref.design3(0.1, 0.1, 2.8)))
    with pytest.raises(ValueError, match="36864"):
        oip.mtfc_quantise(oip.mtfc_design3(0.1, 0.1, 3.0))
    with pytest.raises(ValueError):
        ref.quantise(ref.design3(0.1, 0.1, 3.0))


def test_quantise_ties_and_centre_correction():
    """0.5 / 4096 and 2.5 / 4096 are ties: to even, 0 and 2.  The taps then sum to 4095 and the centre takes the missing 1."""
    c = np.array([[0.5 / 4096, 1.0 - 3.0 / 4096, 2.5 / 4096]])
    assert c.sum() == 1.0
    t = oip.mtfc_quantise(c)
    assert t.tolist() == [[0, 4094, 2]] and np.array_equal(t, ref.quantise(c))
    c = np.array([[1.5 / 4096], [1.0 - 5.0 / 4096], [3.5 / 4096]])                 # 2 and 4: the centre gives one back
    assert oip.mtfc_quantise(c).tolist() == [[2], [4090], [4]] and np.array_equal(oip.mtfc_quantise(c), ref.quantise(c))
    # a designed filter whose rounded taps do not sum to 4096
    c = ref.design3(0.35, 0.9, 4.0)                              # rounds to a sum of 4098
    assert int(np.rint(c * 4096).sum()) != 4096
    t = oip.mtfc_quantise(c)
    assert t.sum() == 4096 and np.array_equal(t, ref.quantise(c))
    # a random 9 x 9 low-gain kernel
    rng = np.random.default_rng(9)
    c = rng.normal(0, 0.01, (9, 9))
    c[4, 4] += 1.0 - c.sum()
    c[4, 4] += 1.0 - sum(float(v) for v in c.ravel())
    assert np.array_equal(oip.mtfc_quantise(c), ref.quantise(c))


def test_refusals():
    ok = ref.design3(0.5, 0.5, 2.0)
    bad = ok.copy()
    bad[0, 0] += 1e-5                                               # the sum is off by more than 1e-6
    near = ok.copy()
    near[0, 0] += 5e-7
    assert oip.mtfc_quantise(near).sum() == 4096
    for c in (bad, np.full((3, 3), np.nan), np.ones((2, 3)) / 6, np.ones((3, 4)) / 12, np.ones((11, 1)) / 11, np.ones((1, 11)) / 11):
        with pytest.raises(ValueError):
            oip.mtfc_quantise(c)
    with pytest.raises(ValueError):
        oip.mtfc_quantise(np.ones(3) / 3)                           # not (ky, kx)
    for args in [(0.0, 0.5, 2.0), (0.5, 0.0, 2.0), (-0.1, 0.5, 2.0), (1.5, 0.5, 2.0), (0.5, 1.0001, 2.0), (0.5, 0.5, 0.99),
                 (float("nan"), 0.5, 2.0), (0.5, 0.5, float("nan"))]:
        with pytest.raises(ValueError):
            oip.mtfc_design3(*args)
        with pytest.raises(ValueError):
            ref.design3(*args)


def test_load_kernel(tmp_path):
    p = str(tmp_path / "k.txt")
    c = np.random.default_rng(4).normal(0, 1, (5, 3))
    ref.write_kernel(p, c)
    got = oip.mtfc_load_kernel(p)
    assert got.shape == (5, 3) and got.tobytes() == c.tobytes() and got.tobytes() == ref.load_kernel(p).tobytes()
    open(p, "w").write("1 3\n\t0.25   5e-1\n\n0.25\n")               # any white space
    assert oip.mtfc_load_kernel(p).tolist() == [[0.25, 0.5, 0.25]]
    with pytest.raises(OSError):
        oip.mtfc_load_kernel(str(tmp_path / "missing.txt"))
    for text in ["", "3\n", "3 3\n1 2 3\n4 5 6\n7 8\n", "3 3\n1 2 3\n4 5 6\n7 8 9 10\n", "3 3\n1 2 3\n4 x 6\n7 8 9\n", "2 3\n1 2 3\n4 5 6\n",
                 "3 4\n" + "1 " * 12, "11 1\n" + "1 " * 11, "0 1\n", "-3 3\n" + "1 " * 9, "a b\n", "1 1\n1\nend\n"]:
        open(p, "w").write(text)
        with pytest.raises(ValueError):
            oip.mtfc_load_kernel(p)


# ---- the sub-command ------------------------------------------------------------------------------------------------------------
def _no_device(r):
    """exit code 2 is also what a missing GPU gives: the refusal must have come first"""
    return r.returncode == 2 and "MI355X" not in r.stdout


def test_cli_refusals_before_the_device(tmp_path):
    d = str(tmp_path)
    np.zeros((8, 64), np.uint16).tofile(os.path.join(d, "P.RAW"))
    np.zeros((8, 64), np.uint16).tofile(os.path.join(d, "P.IMG"))
    ref.write_kernel(os.path.join(d, "k.txt"), ref.design3(0.5, 0.5))
    base = ["P.RAW", "--width", "64"]
    mtf = ["--mtf-x", "0.5", "--mtf-y", "0.5"]
    r = _run(["P.IMG", "--width", "64"] + mtf, d)                    # neither .RAW nor .TIFF
    assert _no_device(r) and "RAW and TIFF" in r.stdout
    assert _run(mtf, d).returncode == 106                           # IMAGE is required
    assert _run(["missing.RAW"] + mtf, d).returncode == 105
    assert _run(base + ["--kernel", "missing.txt"], d).returncode == 105
    assert _run(base + ["--mtf-x", "0.5"], d).returncode == 106     # the two come together
    assert _run(base + ["--mtf-y", "0.5"], d).returncode == 106
    assert _run(base + mtf + ["--frobnicate"], d).returncode == 109
    assert _run(base + mtf + ["--valid-min", "70000"], d).returncode == 105
    assert _run(base + mtf + ["--valid-min", "-1"], d).returncode == 105
    assert _run(base + ["--mtf-x", "0", "--mtf-y", "0.5"], d).returncode == 105
    assert _run(base + ["--mtf-x", "0.5", "--mtf-y", "1.5"], d).returncode == 105
    assert _run(base + mtf + ["--max-gain", "0.5"], d).returncode == 105
    for args in [base, base + ["--kernel", "k.txt"] + mtf, base + ["--kernel", "k.txt", "--max-gain", "2"]]:      # neither, both
        r = _run(args, d)
        assert r.returncode == 254 and "USAGE ERROR" in r.stdout, args
    r = _run(base + ["--mtf-x", "0.1", "--mtf-y", "0.1", "--max-gain", "3"], d)       # sum |t| = 36864
    assert _no_device(r) and "36864" in r.stdout
    open(os.path.join(d, "bad.txt"), "w").write("3 3\n1 2 3\n")
    r = _run(base + ["--kernel", "bad.txt"], d)
    assert _no_device(r) and "bad.txt" in r.stdout
    r = _run(["P.RAW", "--width", "60"] + mtf, d)                    # 1024 bytes are not lines of 120
    assert _no_device(r) and "size invalid" in r.stdout
    r = _run(base + mtf + ["-o", "out.TIFF"], d)                    # the container of the input
    assert _no_device(r) and "container" in r.stdout
    r = _run(base + mtf + ["-o", "P.RAW"], d)
    assert _no_device(r) and "is the input image" in r.stdout
    assert sorted(os.listdir(d)) == ["P.IMG", "P.RAW", "bad.txt", "k.txt", "oip.log"]


@pytest.mark.parametrize("named", [False, True])
def test_cli_existing_output_is_refused_without_force(tmp_path, named):
    d = str(tmp_path)
    np.zeros((8, 64), np.uint16).tofile(os.path.join(d, "P.RAW"))
    out = os.path.join(d, "mine.RAW" if named else "P.MTFC.RAW")
    with open(out, "wb") as f:
        f.write(b"not a filtered strip")
    r = _run(["P.RAW", "--width", "64", "--mtf-x", "0.5", "--mtf-y", "0.5"] + (["-o", "mine.RAW"] if named else []), d)
    assert _no_device(r) and os.path.basename(out) in r.stdout and "--force" in r.stdout
    assert open(out, "rb").read() == b"not a filtered strip"


def test_help_lists_the_sub_command(tmp_path):
    r = subprocess.run([OIP, "--help"], cwd=str(tmp_path), capture_output=True, text=True)
    assert r.returncode == 255 and "mtfc" in r.stdout and "--mtf-x" in r.stdout and "--kernel" in r.stdout
