"""CPU: the tile-major form on its numpy restatement (_cog_ref.py), the tiled writer and the tiled branch of the reader
(csrc/oip_tifftiled.hpp, csrc/oip_tiff.hpp) as a stand-alone program under ASan + UBSan (tests/cpp/tifftiled_test.cpp), the files
it keeps read back by a reader of this suite's own and by Pillow, and what `oip cog` refuses before a device is touched."""
import os
import subprocess

import numpy as np
import pytest

import _cog_ref as cog
import _overview_ref as ovr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_properties():
    rng = np.random.default_rng(1)
    for spp in (1, 4):
        for T in (16, 32):
            for w, h in ((1, 1), (15, 17), (16, 16), (33, 47), (70, 5)):
                x = rng.integers(0, 65536, (h, w * spp)).astype(np.uint16)
                t = cog.retile(x, spp, T)
                tx, ty = cog.grid(w, h, T)
                assert t.shape == (tx * ty, T, T * spp)
                # the definition, sample by sample, on a few samples of every tile
                p = x.reshape(h, w, spp)
                for k in range(tx * ty):
                    j, i = divmod(k, tx)
                    for r, c in ((0, 0), (T - 1, T - 1), (T // 2, T - 1), (T - 1, 3)):
                        assert np.array_equal(t[k, r, c * spp:(c + 1) * spp], p[min(j * T + r, h - 1), min(i * T + c, w - 1)])
                assert np.array_equal(cog.untile(t, w, h, spp, T), x)
                # the inverse ignores the padding; batches of tile rows are slices of the whole
                junk = t.copy().reshape(ty, tx, T, T, spp)
                junk[-1, :, (h - 1) % T + 1:] = 0xDEAD
                junk[:, -1, :, (w - 1) % T + 1:] = 0xBEEF
                assert np.array_equal(cog.untile(junk.reshape(t.shape), w, h, spp, T), x)
                for j0 in range(ty):
                    assert np.array_equal(cog.retile(x, spp, T, j0, 1), t[j0 * tx:(j0 + 1) * tx])


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("tifftiled")
    src = os.path.join(ROOT, "tests", "cpp", "tifftiled_test.cpp")
    inc = os.path.join(ROOT, "opticalimageprocessor_amd", "csrc")
    exe = d / "tifftiled"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread", "-I" + inc,
                    src, "-o", str(exe)], check=True)
    return str(exe)


def _kept(d):
    with open(os.path.join(d, "kept.txt")) as f:
        for line in f:
            name, *v = line.split()
            yield (name,) + tuple(int(x) for x in v)


@pytest.fixture(scope="module", params=[False, True], ids=["classic", "bigtiff"])
def written(program, tmp_path_factory, request):
    """the program's whole run: 1176 round trips, the refusals, the interfaces; the files it kept"""
    d = str(tmp_path_factory.mktemp("cog_files"))
    r = subprocess.run([program, d], capture_output=True, text=True, env=dict(os.environ, OIP_TIFF_FORCE_BIG="1" if request.param else "0"))
    assert r.returncode == 0 and "1176 files, 0 bad" in r.stdout, r.stdout + r.stderr
    return d, request.param


def test_round_trips_refusals_and_kept_files(written):
    """every kept file through the suite's reader: the image at level 0, _overview_ref.halve chains at the levels, replicated
    padding, every directory ahead of the first tile"""
    d, big = written
    n = 0
    for name, w, h, spp, comp, T, levels in _kept(d):
        x = np.fromfile(os.path.join(d, name + ".L0.raw"), np.uint16).reshape(h, w * spp)
        cog.assert_is_cog(os.path.join(d, name + ".tiff"), [x] + ovr.pyramid(x, levels, 1, spp), spp, T, big=big, compression=comp)
        n += 1
    assert n == 2 * 2 * 3 * 5 + 2 * 3                             # (spp, compression, levels) x (4 + 1 sizes), and 257 x 257 uncompressed


def test_pillow_returns_every_directory(written):
    features = pytest.importorskip("PIL.features")
    if not features.check("libtiff"):
        pytest.skip("Pillow without libtiff reads no tiled 16-bit LZW")
    from PIL import Image
    d, _ = written
    n = 0
    for name, w, h, spp, comp, T, levels in _kept(d):
        if spp != 1:
            continue
        x = np.fromfile(os.path.join(d, name + ".L0.raw"), np.uint16).reshape(h, w)
        want = [x] + ovr.pyramid(x, levels, 1, 1)
        with Image.open(os.path.join(d, name + ".tiff")) as im:
            assert im.n_frames == levels + 1
            for k in range(levels + 1):
                im.seek(k)
                assert np.array_equal(np.asarray(im), want[k]), (name, k)
        n += 1
    assert n > 0


# ---- what `oip cog` refuses before a device is touched (there is none here) ---------------------------------------------------
def test_cli_refusals_need_no_device(tmp_path):
    oip = os.path.join(ROOT, "opticalimageprocessor_amd", "lib", "oip")
    d = str(tmp_path)
    np.zeros((70, 40), np.uint16).tofile(os.path.join(d, "P.RAW"))
    open(os.path.join(d, "P.PNG"), "wb").write(b"x" * 80)
    open(os.path.join(d, "there.TIFF"), "wb").write(b"kept")

    def snapshot():
        return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if f != "oip.log"}

    before = snapshot()
    env = dict(os.environ, LOGFILE=os.path.join(d, "oip.log"))
    raw = ["P.RAW", "--width", "40"]
    for args, rc, text in ((raw + ["--tile", "0"], 105, "--tile"), (raw + ["--tile", "8"], 105, "--tile"), (raw + ["--tile", "24"], 105, "--tile"),
                           (raw + ["--tile", "1040"], 105, "--tile"), (raw + ["--tile", "2048"], 105, "--tile"), (raw + ["--tile", "x"], 104, "--tile"),
                           (raw + ["--levels", "-1"], 105, "--levels"), (raw + ["--levels", "17"], 105, "--levels"),
                           (raw + ["--valid-min", "65536"], 105, "--valid-min"), (["P.PNG"], 2, "only RAW and TIFF image supported"),
                           (["P.RAW", "--width", "41"], 2, "file size invalid"), (raw + ["-o", "P.RAW", "--force"], 2, "is the input image"),
                           (raw + ["-o", "there.TIFF"], 2, "--force"), (["missing.RAW"], 105, "does not exist"), (raw + ["--bil"], 109, "--bil")):
        r = subprocess.run([oip, "cog"] + args, cwd=d, env=env, capture_output=True, text=True)
        assert r.returncode == rc and text in r.stdout + r.stderr and "no usable" not in r.stdout + r.stderr, (args, r.returncode, r.stdout + r.stderr)
        assert snapshot() == before, args
