"""CPU: the overview pyramid's definition on its numpy restatement (_overview_ref.py), the host writer of the overview file
(csrc/oip_tiff.hpp: TiffWriterU16 with overview_levels) as a stand-alone program under ASan + UBSan, read back by a parser of
this suite's own, and the default level count against the library's."""
import os
import subprocess

import numpy as np
import pytest

import _overview_ref as ref
from _tiff import read_tags, read_tiff_u16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (1, 2), (2, 1), (3, 5), (8, 8), (17, 9), (64, 33), (65, 130)]


def _noise(h, w, spp, seed):
    """12-bit noise with 30 % zeros and 2 % 65535: all-no-data blocks and mixed blocks both occur"""
    rng = np.random.default_rng(seed)
    x = rng.integers(1, 4096, (h, w * spp)).astype(np.uint16)
    x[rng.random(x.shape) < 0.30] = 0
    x[rng.random(x.shape) < 0.02] = 65535
    return x


@pytest.mark.parametrize("spp", [1, 4])
@pytest.mark.parametrize("valid_min", [0, 1, 300])
def test_definition_properties(spp, valid_min):
    for i, (h, w) in enumerate(SHAPES):
        x = _noise(h, w, spp, 10 * i + spp)
        y = ref.halve(x, valid_min, spp)
        assert y.shape == ((h + 1) // 2, (w + 1) // 2 * spp) and y.dtype == np.uint16
        # cut at any even line: the same bytes
        for cut in range(2, h, 2):
            assert np.array_equal(np.concatenate([ref.halve(x[:cut], valid_min, spp), ref.halve(x[cut:], valid_min, spp)]), y)
        # a level fed back in gives the next level
        p = ref.pyramid(x, 3, valid_min, spp)
        assert np.array_equal(p[0], y) and np.array_equal(p[1], ref.halve(y, valid_min, spp)) and np.array_equal(p[2], ref.halve(p[1], valid_min, spp))
        # data never becomes no data; no data appears only where every input was no data
        for lv in p:
            assert ((lv == 0) | (lv >= valid_min)).all()
        if valid_min > 0:
            H, W = (h + 1) // 2, (w + 1) // 2
            valid = np.zeros((2 * H, 2 * W, spp), bool)
            valid[:h, :w] = x.reshape(h, w, spp) >= valid_min
            assert np.array_equal(y != 0, valid.reshape(H, 2, W, 2, spp).any(axis=(1, 3)).reshape(H, -1))


@pytest.mark.parametrize("spp", [1, 4])
def test_valid_min_0_full_blocks_divide_by_a_shift(spp):
    x = _noise(64, 48, spp, 3)
    S = x.astype(np.int64).reshape(32, 2, 24, 2, spp).sum(axis=(1, 3)).reshape(32, -1)
    assert np.array_equal(ref.halve(x, 0, spp), ((S + 2) >> 2).astype(np.uint16))


def test_single_pixel_and_edges():
    for vm in (0, 1, 300):
        assert ref.halve(np.array([[777]], np.uint16), vm).tolist() == [[777]]
        assert [lv.shape for lv in ref.pyramid(np.full((1, 1), 777, np.uint16), 4, vm)] == [(1, 1)] * 4
    assert ref.halve(np.array([[100]], np.uint16), 300).tolist() == [[0]]
    # an edge block uses its own n: 3 x 3 -> the right column and the bottom row are means of two, the corner of one
    x = np.array([[10, 20, 31], [10, 21, 32], [5, 8, 9]], np.uint16)
    assert ref.halve(x, 0).tolist() == [[(61 + 2) >> 2, (63 + 1) >> 1], [(13 + 1) >> 1, 9]]
    # three valid of four: (S + 1) // 3
    assert ref.halve(np.array([[0, 400], [401, 402]], np.uint16), 1).tolist() == [[(1203 + 1) // 3]]


def test_nested_levels_are_not_a_direct_box():
    """level 2 is defined from level 1 (as gdaladdo -r average does it), not as a 4 x 4 box of the image: on random data the two
    differ by 1 DN on a good share of the samples, so nobody swaps the definition unnoticed"""
    x = np.random.default_rng(64).integers(0, 4096, (64, 64)).astype(np.uint16)
    nested = ref.pyramid(x, 2, 0)[1].astype(np.int64)
    S = x.astype(np.int64).reshape(16, 4, 16, 4).sum(axis=(1, 3))
    direct = (S + 8) >> 4
    d = np.abs(nested - direct)
    assert d.max() == 1 and 0.05 < (d != 0).mean() < 0.5


def test_default_levels_against_the_library():
    """oip_overview_levels is a host entry point: the library loads without a device"""
    from opticalimageprocessor_amd import capi
    assert ref.default_levels(256, 256) == 1 and ref.default_levels(512, 512) == 1 and ref.default_levels(513, 2) == 2
    assert ref.default_levels(24576, 100000) == 9 and ref.default_levels(1, 1) == 1 and ref.default_levels(2 ** 31 - 1, 2 ** 31 - 1) == 16
    for w in (1, 2, 255, 256, 257, 511, 512, 513, 1024, 1025, 6144, 12288, 24576, 2 ** 31 - 1):
        for h in (1, 256, 257, 512, 513, 60000, 100000, 2 ** 31 - 1, 2 ** 40):
            assert capi.overview_levels(w, h) == ref.default_levels(w, h), (w, h)


# ---- the host writer -------------------------------------------------------------------------------------------------------
CASES = [("g1", 37, 53, 1, 1, 3), ("g1z", 37, 53, 1, 5, 3), ("c4", 21, 40, 4, 1, 4), ("c4z", 21, 40, 4, 5, 4), ("one", 5, 3, 1, 1, 1),
         ("wide", 40000, 6, 1, 5, 2), ("strips", 4100, 4200, 1, 1, 2)]      # level 1: `wide` a line per LZW strip, `strips` two strips of 8 MiB


@pytest.fixture(scope="module")
def pyramid_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("tiff_pyramid")
    src = os.path.join(ROOT, "tests", "cpp", "tiff_pyramid_test.cpp")
    inc = os.path.join(ROOT, "opticalimageprocessor_amd", "csrc")
    exe = d / "tiff_pyramid"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread", "-I" + inc,
                    src, "-o", str(exe)], check=True)
    return str(exe)


@pytest.fixture(scope="module")
def levels():
    out = {}
    for i, (name, w, h, spp, comp, n) in enumerate(CASES):
        # (`wide`: runs of 64 equal samples, so that the suite's own LZW decoder has few codes to walk through)
        x = np.repeat(_noise(h, w // 64, spp, 100 + i), 64, axis=1) if name == "wide" else _noise(h, w, spp, 100 + i)
        out[name] = [x] + ref.pyramid(x, n, 1, spp)
    return out


def _write(program, levels, d, force_big, cases=CASES):
    with open(os.path.join(d, "manifest.txt"), "w") as f:
        for name, w, h, spp, comp, n in cases:
            f.write("%s %d %d %d %d %d\n" % (name, w, h, spp, comp, n))
            for k, lv in enumerate(levels[name]):
                lv.tofile(os.path.join(d, "%s.L%d.raw" % (name, k)))
    env = dict(os.environ, OIP_TIFF_FORCE_BIG="1" if force_big else "0")
    r = subprocess.run([program, d], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "%d cases, 0 bad" % len(cases) in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("force_big", [False, True])
def test_writer_chains_reduced_resolution_directories(pyramid_program, levels, tmp_path, force_big):
    """spp 1 and 4, uncompressed and host LZW, classic and BigTIFF, through write_rows() and (the program compares the files)
    through the external interfaces: every directory parsed -- pixels, tag 254, the chain, the final 0 -- and the one-image
    file beside it"""
    d = str(tmp_path)
    _write(pyramid_program, levels, d, force_big)
    for name, w, h, spp, comp, n in CASES:
        lv = levels[name]
        dirs = ref.assert_is_pyramid(os.path.join(d, name + ".ovr"), lv[1:], spp, big=force_big, compression=comp)
        for k, e in enumerate(dirs):
            t = e["tags"]
            assert (t[256][0], t[257][0]) == ((w - 1 >> k + 1) + 1, (h - 1 >> k + 1) + 1)
            # the one-image writer's tags for a product of that geometry, and its strip rule
            assert t[262] == [2 if spp == 4 else 1] and t[284] == [1] and t[258] == [16] * spp and t[339] == [1] * spp
            assert (t.get(317) == [2]) == (comp == 5) and (t.get(338) == [2]) == (spp == 4)
            row = t[256][0] * spp * 2
            assert t[278][0] == max(1, min(t[257][0], ((64 << 10) if comp == 5 else (8 << 20)) // row))
        if name in ("wide", "strips"):
            assert len(dirs[0]["tags"][273]) == (3 if name == "wide" else 2)
        # the one-image file: a single directory without NewSubfileType, as ever
        one, big = ref.read_tiff_dirs(os.path.join(d, name + ".one.tiff"))
        assert len(one) == 1 and 254 not in one[0]["tags"] and one[0]["next"] == 0 and big == force_big
        assert np.array_equal(one[0]["img"].reshape(lv[0].shape), lv[0])
        assert read_tags(os.path.join(d, name + ".one.tiff")) == one[0]["tags"]
        # and the first level of the overview file is what a first-directory reader sees
        img, _, _ = read_tiff_u16(os.path.join(d, name + ".ovr"))
        assert np.array_equal(img.reshape(lv[1].shape), lv[1])


def test_pillow_returns_every_level(pyramid_program, levels, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    d = str(tmp_path)
    _write(pyramid_program, levels, d, False, [c for c in CASES if c[0] == "g1"])
    with Image.open(os.path.join(d, "g1.ovr")) as im:
        assert im.n_frames == 3
        for k in range(3):
            im.seek(k)
            assert np.array_equal(np.asarray(im), levels["g1"][k + 1]), k


# ---- what `oip overviews` refuses before a device is touched (there is none here) -------------------------------------------
def test_cli_refusals_need_no_device(tmp_path):
    oip = os.path.join(ROOT, "opticalimageprocessor_amd", "lib", "oip")
    d = str(tmp_path)
    np.zeros((70, 40), np.uint16).tofile(os.path.join(d, "P.RAW"))
    open(os.path.join(d, "P.PNG"), "wb").write(b"x" * 80)
    open(os.path.join(d, "there.ovr"), "wb").write(b"kept")

    def run(args, tool="overviews"):
        env = dict(os.environ, LOGFILE=os.path.join(d, "oip.log"))
        return subprocess.run([oip, tool] + args, cwd=d, env=env, capture_output=True, text=True)
    for args, rc, text in ((["P.PNG"], 2, "only RAW and TIFF image supported"), (["P.RAW", "--width", "41"], 2, "file size invalid"),
                           (["P.RAW", "--width", "40", "--levels", "0"], 105, "--levels"), (["P.RAW", "--width", "40", "--levels", "17"], 105, "--levels"),
                           (["P.RAW", "--width", "40", "--valid-min", "65536"], 105, "--valid-min"),
                           (["P.RAW", "--width", "40", "-o", "P.RAW", "--force"], 2, "is the input image"),
                           (["P.RAW", "--width", "40", "-o", "there.ovr"], 2, "--force"), (["missing.RAW"], 105, "does not exist"),
                           (["P.RAW", "--bil"], 109, "--bil")):
        r = run(args)
        assert r.returncode == rc and text in r.stdout + r.stderr and "no usable" not in r.stdout + r.stderr, (args, r.stdout + r.stderr)
    assert open(os.path.join(d, "there.ovr"), "rb").read() == b"kept" and not os.path.exists(os.path.join(d, "P.RAW.ovr"))
    r = run(["--image1", "P.RAW", "--image2", "P.RAW", "--fold-cols", "8", "--levels", "2"], tool="stitch")
    assert r.returncode == 107 and "--levels requires --overviews" in r.stderr
