"""GPU: the tools on Deflate TIFFs.  `oip quicklook`, `oip overviews` and `oip cog` write for a Deflate strip file and for a Deflate
tiled file (written here with zlib: tests/_deflate_tiff.py) the bytes they write for the uncompressed TIFF of the same pixels --
with the streams inflated on the device, and with OIP_TIFF_GPU_DEFLATE=0 on the host's threads.  The device takes a file of at
least 256 streams of at most 2 MiB (csrc/oip_tiffstreams.h::tiff_streams_on_device), so the device files here are strips of one row and
tiles of 16; files of a few streams go to the host whatever the switch says.  A corrupt tile ends the run with exit code 2 and the
tile named -- in the words of the route that met it, which is also how these tests know the route."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import _deflate_tiff as T
from _tiff import write_tiff_u16

pytestmark = pytest.mark.gpu
OIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "opticalimageprocessor_amd", "lib", "oip")
OUTS = {"quicklook": "ql.TIFF", "overviews": "o.ovr", "cog": "c.TIFF"}


def _run(tool, args, cwd, rc=0, **env):
    env = dict(os.environ, LOGFILE=os.path.join(cwd, "oip.log"), **env)
    r = subprocess.run([OIP, tool] + args, cwd=cwd, env=env, capture_output=True, text=True)
    assert r.returncode == rc, (tool, args, r.stdout + r.stderr)
    return r


def _sha(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def _scene(h, w, spp, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    a = np.stack([1500 + 900 * np.sin(x / (11.0 + c)) * np.cos(y / (17.0 + c)) + rng.integers(0, 30, (h, w)) for c in range(spp)], axis=2)
    a = a.astype(np.uint16)
    a[:3, :5] = 0
    a[-2:, -7:] = 65535
    return np.ascontiguousarray(a).reshape(h, w * spp)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """M: 300 x 260 of 4 samples, P: 333 x 270 of 1 sample; each uncompressed (<n>.TIFF), in Deflate strips of one row with predictor
    2 (<n>.strips.TIFF: 260 and 270 streams) and in Deflate tiles of 16 (<n>.tiles.TIFF: 323 and 357 streams), which the device
    takes; in strips of 7 rows (<n>.s7.TIFF), tiles of 128 (<n>.t128.TIFF: 9 and 9 streams) and of 48 x 32 (<n>.t48.TIFF), which
    the host takes; and the SHA-256 of what the three tools write for the uncompressed one"""
    d = str(tmp_path_factory.mktemp("deflate_cli"))
    want = {}
    for name, (h, w, spp) in {"M": (260, 300, 4), "P": (270, 333, 1)}.items():
        img = _scene(h, w, spp, 1 + spp)
        write_tiff_u16(os.path.join(d, name + ".TIFF"), img.reshape(h, w, spp) if spp == 4 else img)
        _, lens = T.write(os.path.join(d, name + ".strips.TIFF"), img, spp, 2, rps=1)
        assert len(lens) >= 256
        _, lens = T.write(os.path.join(d, name + ".tiles.TIFF"), img, spp, 2, tile=(16, 16), level=9)
        assert len(lens) >= 256
        T.write(os.path.join(d, name + ".s7.TIFF"), img, spp, 2, rps=7)
        T.write(os.path.join(d, name + ".t128.TIFF"), img, spp, 2, tile=(128, 128))
        T.write(os.path.join(d, name + ".t48.TIFF"), img, spp, 1, tile=(48, 32), compression=32946)
        want[name] = {}
        for tool, out in OUTS.items():
            _run(tool, [name + ".TIFF", "-o", "want." + name + "." + out, "--force"], d)
            want[name][tool] = _sha(os.path.join(d, "want." + name + "." + out))
    return d, want


@pytest.mark.parametrize("route", ["device", "host"])
@pytest.mark.parametrize("layout", ["strips", "tiles"])
def test_deflate_input_gives_what_the_uncompressed_file_gives(files, layout, route):
    d, want = files
    env = {"OIP_TIFF_GPU_DEFLATE": "0"} if route == "host" else {}
    for tool in OUTS:
        _run(tool, ["M.%s.TIFF" % layout, "-o", "got." + OUTS[tool], "--force"], d, **env)
        assert _sha(os.path.join(d, "got." + OUTS[tool])) == want["M"][tool], (layout, route, tool)


def test_one_sample_files_tile_batches_and_tiles_of_another_shape(files):
    d, want = files
    for src, env in (("P.strips.TIFF", {}), ("P.tiles.TIFF", {}), ("P.t48.TIFF", {}), ("M.t48.TIFF", {}), ("M.tiles.TIFF", {"OIP_COG_BATCH_MB": "1"}),
                     ("M.s7.TIFF", {}), ("M.t128.TIFF", {}), ("P.s7.TIFF", {}), ("P.t128.TIFF", {})):
        _run("overviews", [src, "-o", "got1.ovr", "--force"], d, **env)
        assert _sha(os.path.join(d, "got1.ovr")) == want[src[0]]["overviews"], (src, env)


def _corrupt(d, name, T_, k):
    """300 x 260 x 4 in tiles of T_, tile k cut in half"""
    img = _scene(260, 300, 4, 5)
    streams = T.streams_of(img, 4, 2, tile=(T_, T_))
    streams[k] = streams[k][:len(streams[k]) // 2]
    T.write(os.path.join(d, name), img, 4, 2, tile=(T_, T_), streams=streams)
    return len(streams)


@pytest.mark.parametrize("route", ["device", "host"])
def test_a_corrupt_tile_ends_the_run_with_the_tile_named(files, route):
    """323 tiles of 16, tile 100 cut: the device decoder takes the tiles of a batch as strips of a 16-wide image and says "strip 100
    (tiles from 0 on)" (one batch here); the host reader says "tile 100 of [file]" """
    d, _ = files
    assert _corrupt(d, "bad.TIFF", 16, 100) == 323
    env = {"OIP_TIFF_GPU_DEFLATE": "0"} if route == "host" else {}
    r = _run("quicklook", ["bad.TIFF", "-o", "bad.ql.TIFF", "--force"], d, rc=2, **env)
    text = r.stdout + r.stderr
    want = "in strip 100 (tiles from 0 on)" if route == "device" else "in tile 100 of ["
    assert "corrupt Deflate stream (stream ends inside a block) " + want in text, text


def test_a_file_of_few_streams_is_read_on_the_host(files):
    """9 tiles of 128: below the 256 streams the device route asks for, so the refusal is in the host reader's words"""
    d, _ = files
    assert _corrupt(d, "bad9.TIFF", 128, 4) == 9
    r = _run("quicklook", ["bad9.TIFF", "-o", "bad.ql.TIFF", "--force"], d, rc=2)
    assert "corrupt Deflate stream (stream ends inside a block) in tile 4 of [" in r.stdout + r.stderr, r.stdout + r.stderr
