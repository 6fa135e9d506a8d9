"""CPU: the tap tables of `oip rescale` against the numpy restatement (_rescale_ref.py) -- equality, no tolerance: for the pairs
below every pre-rounding value w / sum w * 16384 lies at least 5e-4 from a half-integer, so a last-bit difference between libm
and numpy cannot move a tap --, the properties of the restatement itself, the host arithmetic as a stand-alone program under
ASan + UBSan (tests/cpp/rescale_test.cpp), and what `oip rescale` refuses before a device is touched."""
import os
import subprocess

import numpy as np
import pytest

import _rescale_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("lanczos", "cubic", "linear")


@pytest.mark.parametrize("kind", KINDS)
def test_tables_equal_the_restatement(kind):
    from opticalimageprocessor_amd import capi
    for n_in, n_out in ref.PAIRS:
        margins = []
        first, taps = ref.taps(kind, n_in, n_out, margins)
        f, t = capi.rescale_taps(kind, n_in, n_out)
        assert min(margins) >= 5e-4, (n_in, n_out, min(margins))           # why equality is the right bar
        assert t.dtype == np.int16 and f.dtype == np.int32
        assert t.shape == (n_out, ref.taps_k(kind, n_in, n_out)) and t.shape[1] == 2 * -(-ref.KERNELS[kind] * max(n_in, n_out) // n_out)
        assert np.array_equal(f, first), (n_in, n_out)
        assert np.array_equal(t, taps), (n_in, n_out, np.argwhere(t != taps)[:4])
        assert (t.astype(np.int64).sum(axis=1) == 16384).all()
        assert np.abs(t.astype(np.int64)).sum(axis=1).max() <= 25300
        assert capi.rescale_taps(capi.RESCALE_KERNELS[kind], n_in, n_out)[1].shape == t.shape      # by number as well


def test_identity_rows_k_and_limits():
    from opticalimageprocessor_amd import capi
    f, t = capi.rescale_taps("lanczos", 64, 64)
    assert (t == np.array([0, 0, 16384, 0, 0, 0], np.int16)).all() and np.array_equal(f, np.arange(64) - 2)
    for kind, K in (("cubic", 4), ("linear", 2)):
        f, t = capi.rescale_taps(kind, 9, 9)
        assert t.shape[1] == K and (t[np.arange(9)[:, None] == f[:, None] + np.arange(K)[None]] == 16384).all() and (t.sum(axis=1) == 16384).all()
    assert capi.rescale_taps("lanczos", 4, 1)[1].shape == (1, 24)            # n_in = 4 n_out: K = 24, the limit
    assert capi.rescale_taps("lanczos", 800, 200)[1].shape == (200, 24)
    assert capi.rescale_taps("lanczos", 1, 16)[1].shape == (16, 6)           # n_out = 16 n_in
    assert capi.rescale_taps("linear", 1, 1)[1].tolist() == [[16384, 0]]     # n = 1
    for n_in, n_out, text in ((5, 1, "overviews"), (801, 200, "overviews"), (1, 17, "16"), (0, 4, "empty"), (4, 0, "empty"), (-3, 4, "empty")):
        with pytest.raises(ValueError, match=text):
            capi.rescale_taps("lanczos", n_in, n_out)
    with pytest.raises(ValueError):
        capi.rescale_taps(3, 8, 8)


def test_size_and_source_range():
    from opticalimageprocessor_amd import capi
    for n, p, q in ((203, 3, 4), (203, 1, 4), (10, 1, 4), (6, 1, 4), (517, 2, 1), (60000, 8, 10), (6144, 2, 3), (1, 1, 3), (7, 16, 1)):
        assert capi.rescale_size(n, p, q) == ref.size(n, p, q) == int(np.floor(n * p / q + 0.5))
    for bad in ((0, 1, 1), (5, 0, 1), (5, 1, 0), (1 << 31, 1, 1)):
        with pytest.raises(ValueError):
            capi.rescale_size(*bad)
    for kind in KINDS:
        for n_in, n_out in ref.PAIRS:
            first, taps = ref.taps(kind, n_in, n_out)
            K = taps.shape[1]
            for o, n in ((0, n_out), (0, 1), (n_out - 1, 1), (n_out // 3, max(1, n_out // 4)), (0, 0)):
                got = capi.rescale_src_range(n_in, n_out, K, o, n)
                assert got == ref.src_range(n_in, n_out, K, o, n)
                if n:
                    idx = np.clip(first[o:o + n, None] + np.arange(K)[None], 0, n_in - 1)
                    assert got == (idx.min(), idx.max() - idx.min() + 1)
    with pytest.raises(ValueError):
        capi.rescale_src_range(10, 10, 6, 5, 6)


# ---- the restatement itself ---------------------------------------------------------------------------------------------------
def test_restatement_properties():
    rng = np.random.default_rng(5)
    for spp in (1, 4):
        for kind in KINDS:
            for c in (0, 1, 777, 32768, 65535):
                x = np.full((23, 19 * spp), c, np.uint16)
                for Wo, Lo in ((19, 23), (31, 9), (5, 70), (76, 6)):
                    assert (ref.rescale_kind(x, spp, Wo, Lo, kind) == c).all(), (kind, c, Wo, Lo)          # constants are kept
            x = rng.integers(0, 65536, (23, 19 * spp)).astype(np.uint16)
            assert np.array_equal(ref.rescale_kind(x, spp, 19, 23, kind), x)                                 # equal sizes: the identity
            # no-data rule on a raster without no data: the same bytes
            y = np.maximum(x, 10)
            for Wo, Lo in ((31, 9), (5, 70), (19, 23)):
                assert np.array_equal(ref.rescale_kind(y, spp, Wo, Lo, kind, valid_min=10), ref.rescale_kind(y, spp, Wo, Lo, kind))
            # a 0 / 65535 checkerboard: every sum stays inside 32 bits (the restatement works in 64) and the result in range
            yy, xx = np.mgrid[0:23, 0:19]
            board = np.repeat(((yy + xx) % 2 * 65535).astype(np.uint16), spp, axis=1)
            for Wo, Lo in ((31, 9), (5, 70), (25, 29), (19, 23)):
                out = ref.rescale_kind(board, spp, Wo, Lo, kind)
                assert out.dtype == np.uint16 and out.shape == (Lo, Wo * spp)
    # channels do not mix: a 4-sample raster is its four planes
    x = rng.integers(0, 65536, (17, 13 * 4)).astype(np.uint16)
    out = ref.rescale_kind(x, 4, 21, 11)
    for c in range(4):
        assert np.array_equal(out[:, c::4], ref.rescale_kind(np.ascontiguousarray(x[:, c::4]), 1, 21, 11))
    # windows of output lines are slices of the whole
    fx, tx = ref.taps("lanczos", 13, 21)
    fy, ty = ref.taps("lanczos", 17, 11)
    assert np.array_equal(ref.rescale(x, 4, 21, 11, fx, tx, fy, ty, rows=(3, 5)), out[3:8])


def test_no_data_stays_no_data_and_q14_stays_near_floating_point():
    rng = np.random.default_rng(6)
    x = rng.integers(1000, 60000, (40, 36)).astype(np.uint16)
    x[:6] = 0
    x[:, :4] = 0
    x[20, 20] = 0
    for Wo, Lo in ((50, 27), (9, 10), (144, 160)):
        out = ref.rescale_kind(x, 1, Wo, Lo, valid_min=1)
        ny, nx = ref.nearest(40, Lo), ref.nearest(36, Wo)
        dead = (ny < 6)[:, None] | (nx < 4)[None]
        assert (out[dead] == 0).all()
        live = ~dead & ~((ny == 20)[:, None] & (nx == 20)[None])
        # ... and nothing rings across the edge of the fill: next to it an output sample is a source sample
        assert np.isin(out[live & np.roll(dead, 1, axis=0)], x).all()
    # The Q14 form against the same filter in floating point on a smooth image.  The bar is reasoned, not measured: a tap is off
    # by at most 1/2 unit of 2^-14, the tap that takes the residue by at most K/2, and the errors of a row sum to zero, so a pass
    # is off by at most K R / 16384 for samples within +-R of their mid value, plus 1/2 DN of rounding; the second pass carries
    # the error of the first with a gain of at most G = 25300 / 16384 (sum |t| of a row).
    yy, xx = np.mgrid[0:61, 0:64]
    smooth = (30000 + 300 * np.sin(yy / 9.0) * np.cos(xx / 7.0) + 2 * yy).astype(np.uint16)
    R = (int(smooth.max()) - int(smooth.min()) + 1) / 2
    Ky, Kx, G = ref.taps_k("lanczos", 61, 37), ref.taps_k("lanczos", 64, 100), 25300 / 16384
    bar = G * (0.5 + Ky * R / 16384) + 0.5 + Kx * R / 16384
    err = np.abs(ref.rescale_kind(smooth, 1, 100, 37) - ref.rescale_float(smooth, 100, 37)).max()
    print("Q14 against floating point: %.3f DN, bar %.3f" % (err, bar))
    assert err <= bar < 2.0


# ---- the host arithmetic under sanitizers, as a program of its own -----------------------------------------------------------
def test_host_arithmetic_under_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "rescale_test.cpp")
    exe = tmp_path / "rescale_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "opticalimageprocessor_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), src, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and " checks, 0 bad" in r.stdout, r.stdout + r.stderr


# ---- what `oip rescale` refuses before a device is touched (there is none here) -----------------------------------------------
def test_cli_refusals_need_no_device(tmp_path):
    oip = os.path.join(ROOT, "opticalimageprocessor_amd", "lib", "oip")
    d = str(tmp_path)
    np.zeros((70, 40), np.uint16).tofile(os.path.join(d, "P.RAW"))
    open(os.path.join(d, "P.PNG"), "wb").write(b"x" * 80)
    open(os.path.join(d, "there.TIFF"), "wb").write(b"kept")
    open(os.path.join(d, "P.RSC.RAW"), "wb").write(b"kept too")

    def snapshot():
        return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if f != "oip.log"}

    before = snapshot()
    env = dict(os.environ, LOGFILE=os.path.join(d, "oip.log"))
    raw = ["P.RAW", "--width", "40"]
    for args, rc, text in (
            # options that exclude each other, and none of them
            (raw + ["--scale", "0.5", "--scale-x", "2"], 107, "--scale excludes --scale-x"),
            (raw + ["--scale", "0.5", "--scale-y", "2"], 107, "--scale excludes --scale-y"),
            (raw + ["--scale", "0.5", "--to-width", "20"], 107, "--scale excludes --to-width"),
            (raw + ["--scale", "0.5", "--to-lines", "20"], 107, "--scale excludes --to-lines"),
            (raw + ["--scale-x", "0.5", "--to-width", "20"], 107, "--scale-x excludes --to-width"),
            (raw + ["--scale-y", "0.5", "--to-lines", "20"], 107, "--scale-y excludes --to-lines"),
            (raw, 106, "is required"),
            # bad values
            (raw + ["--scale", "0"], 105, "--scale"), (raw + ["--scale", "-1"], 105, "--scale"), (raw + ["--scale", "1e1"], 105, "--scale"),
            (raw + ["--scale", "2/0"], 105, "--scale"), (raw + ["--scale-x", "abc"], 105, "--scale-x"), (raw + ["--scale-y", "1/2/3"], 105, "--scale-y"),
            (raw + ["--scale", "0.12345678901"], 105, "--scale"), (raw + ["--to-width", "0"], 105, "--to-width"),
            (raw + ["--to-lines", "-4"], 105, "--to-lines"), (raw + ["--to-width", "x"], 104, "--to-width"),
            (raw + ["--scale", "2", "--kernel", "sinc"], 105, "--kernel"), (raw + ["--scale", "2", "--kernel", "Lanczos"], 105, "--kernel"),
            (raw + ["--scale", "2", "--valid-min", "65536"], 105, "--valid-min"), (["P.RAW", "--width", "0", "--scale", "2"], 105, "--width"),
            (raw + ["--scale", "2", "--bil"], 109, "--bil"), (raw + ["--scale", "2", "--levels", "3"], 109, "--levels"),
            (["missing.RAW", "--scale", "2"], 105, "does not exist"),
            # what needs the file: a ratio outside 1/4 .. 16 on either axis, an empty axis
            (raw + ["--scale", "0.24"], 2, "1/4 .. 16"), (raw + ["--scale-x", "1/5"], 2, "overviews"), (raw + ["--scale-y", "17"], 2, "1/4 .. 16"),
            (raw + ["--to-width", "9"], 2, "1/4 .. 16"), (raw + ["--to-width", "641"], 2, "1/4 .. 16"), (raw + ["--to-lines", "17"], 2, "1/4 .. 16"),
            (raw + ["--to-lines", "1121"], 2, "1/4 .. 16"), (raw + ["--scale-x", "16.5"], 2, "beyond 16"),
            (["P.PNG", "--scale", "2"], 2, "only RAW and TIFF image supported"), (["P.RAW", "--width", "41", "--scale", "2"], 2, "file size invalid"),
            # the output: the input itself, an existing file without --force, another container than RAW or TIFF
            (raw + ["--scale", "2", "-o", "P.RAW", "--force"], 2, "is the input image"), (raw + ["--scale", "2", "-o", "there.TIFF"], 2, "--force"),
            (raw + ["--scale", "2"], 2, "--force"), (raw + ["--scale", "2", "-o", "out.PNG"], 2, "RAW or a TIFF")):
        r = subprocess.run([oip, "rescale"] + args, cwd=d, env=env, capture_output=True, text=True)
        assert r.returncode == rc and text in r.stdout + r.stderr and "no usable" not in r.stdout + r.stderr, (args, r.returncode, r.stdout + r.stderr)
        assert snapshot() == before, args
