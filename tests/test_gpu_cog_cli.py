"""GPU: `oip cog` end to end, and tiled TIFF as the input of the other tools.  The COG holds the image and the restatement's
pyramid (_overview_ref.py) in T x T tiles with replicated edges (_cog_ref.py), every directory ahead of the pixels; its levels
are the ones `oip overviews` writes for the same input; it is the same file whoever encoded its tiles and however the tile rows
were cut into batches; and a tool fed the COG writes what it writes for the strip TIFF of the same pixels.
The images are blocks of noise (8 x 8, or 28 x 28 at 4 samples: no multiple of a tile, and 7 x 7 at level 2), so that the
suite's own LZW decoder has few codes to walk through."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import _cog_ref as cog
import _overview_ref as ovr
from _tiff import write_tiff_u16

pytestmark = pytest.mark.gpu
OIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "opticalimageprocessor_amd", "lib", "oip")


def _run(tool, args, cwd, **env):
    env = dict(os.environ, LOGFILE=os.path.join(cwd, "oip.log"), **env)
    r = subprocess.run([OIP, tool] + args, cwd=cwd, env=env, capture_output=True, text=True)
    assert r.returncode == 0, (tool, args, r.stdout + r.stderr)
    return r


def _blocks(h, w, spp, seed, b=8):
    """(h, w * spp): b x b blocks of 12-bit noise with 30 % no data and a few 65535"""
    rng = np.random.default_rng(seed)
    x = rng.integers(1, 4096, (-(-h // b), -(-w // b), spp)).astype(np.uint16)
    x[rng.random(x.shape) < 0.30] = 0
    x[rng.random(x.shape) < 0.02] = 65535
    return np.ascontiguousarray(np.repeat(np.repeat(x, b, axis=0), b, axis=1)[:h, :w]).reshape(h, w * spp)


def _sha(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


@pytest.fixture(scope="module")
def products(tmp_path_factory):
    """M.TIFF: 700 x 900 of 4 samples; P.TIFF: 1000 x 600 of 1 sample; both in strips, uncompressed"""
    d = str(tmp_path_factory.mktemp("cog"))
    m, p = _blocks(900, 700, 4, 1, 28), _blocks(600, 1000, 1, 2)
    write_tiff_u16(os.path.join(d, "M.TIFF"), m.reshape(900, 700, 4))
    write_tiff_u16(os.path.join(d, "P.TIFF"), p)
    return d, m, p


@pytest.mark.parametrize("name", ["M", "P"])
def test_cog_of_a_product(products, name):
    d, m, p = products
    img, spp, comp = (m, 4, 5) if name == "M" else (p, 1, 1)
    h, w = img.shape[0], img.shape[1] // spp
    r = _run("cog", [name + ".TIFF"], d)
    out = os.path.join(d, name + ".COG.TIFF")
    levels = ovr.default_levels(w, h)
    assert levels == 2
    want = [img] + ovr.pyramid(img, levels, 1, spp)
    T = 128 if spp == 4 else 256                                   # the default tile
    cog.assert_is_cog(out, want, spp, T, big=False, compression=comp)
    assert "%d bytes in " % img.nbytes in r.stdout
    # the levels `oip overviews` writes for the same input
    _run("overviews", [name + ".TIFF"], d)
    dirs, _ = ovr.read_tiff_dirs(os.path.join(d, name + ".TIFF.ovr"))
    assert len(dirs) == levels
    for k, e in enumerate(dirs):
        assert np.array_equal(e["img"].reshape(want[k + 1].shape), want[k + 1]), k + 1
    # the host coders, and tile rows one batch each, write the same file
    _run("cog", [name + ".TIFF", "-o", "host.COG.TIFF", "--force"], d, OIP_TIFF_GPU_LZW="0")
    _run("cog", [name + ".TIFF", "-o", "batch.COG.TIFF", "--force"], d, OIP_COG_BATCH_MB="1")
    assert _sha(os.path.join(d, "host.COG.TIFF")) == _sha(out) == _sha(os.path.join(d, "batch.COG.TIFF"))


@pytest.mark.parametrize("name", ["M", "P"])
def test_cog_options(products, name):
    """BigTIFF; no levels; another tile size with --levels and --valid-min; the other compression; an existing output"""
    d, m, p = products
    img, spp, comp = (m, 4, 5) if name == "M" else (p, 1, 1)
    want = [img] + ovr.pyramid(img, 2, 1, spp)
    T = 128 if spp == 4 else 256                                   # the default tile
    _run("cog", [name + ".TIFF", "-o", "big.COG.TIFF", "--force", "--levels", "1"], d, OIP_TIFF_FORCE_BIG="1")
    cog.assert_is_cog(os.path.join(d, "big.COG.TIFF"), want[:2], spp, T, big=True, compression=comp)
    _run("cog", [name + ".TIFF", "-o", "flat.COG.TIFF", "--force", "--levels", "0"], d)
    cog.assert_is_cog(os.path.join(d, "flat.COG.TIFF"), want[:1], spp, T, compression=comp)
    _run("cog", [name + ".TIFF", "-o", "t64.COG.TIFF", "--force", "--tile", "64", "--levels", "3", "--valid-min", "300"], d)
    cog.assert_is_cog(os.path.join(d, "t64.COG.TIFF"), [img] + ovr.pyramid(img, 3, 300, spp), spp, 64, compression=comp)
    other = "none" if comp == 5 else "lzw"
    _run("cog", [name + ".TIFF", "-o", "other.COG.TIFF", "--force", "--tile", "256", "--tiff-compress", other], d)
    cog.assert_is_cog(os.path.join(d, "other.COG.TIFF"), want, spp, 256, compression=6 - comp)
    # an existing output stays without --force
    r = subprocess.run([OIP, "cog", name + ".TIFF", "-o", "big.COG.TIFF"], cwd=d, env=dict(os.environ, LOGFILE=os.path.join(d, "oip.log")), capture_output=True, text=True)
    assert r.returncode == 2 and "--force" in r.stdout


def test_cog_of_a_raw_strip(tmp_path):
    d = str(tmp_path)
    W, L = 300, 530
    img = _blocks(L, W, 1, 3)
    img.tofile(os.path.join(d, "S.RAW"))
    _run("cog", ["S.RAW", "--width", str(W), "--tile", "32", "--levels", "2"], d)
    cog.assert_is_cog(os.path.join(d, "S.COG.TIFF"), [img] + ovr.pyramid(img, 2, 1), 1, 32, compression=1)


OUTS = {"quicklook": "ql.TIFF", "overviews": "o.ovr", "cog": "c.TIFF"}


@pytest.fixture(scope="module")
def tiled(products):
    """-> get(name): the directory and, made on first use, the product's COG with LZW tiles (<name>.lzw.TIFF) and the SHA-256 of
    what quicklook, overviews and cog write for the strip TIFF"""
    d, want = products[0], {}

    def get(name):
        if name not in want:
            _run("cog", [name + ".TIFF", "-o", name + ".lzw.TIFF", "--force", "--tiff-compress", "lzw"], d)
            want[name] = {}
            for tool, out in OUTS.items():
                _run(tool, [name + ".TIFF", "-o", "want." + out, "--force"], d)
                want[name][tool] = _sha(os.path.join(d, "want." + out))
        return d, want[name]
    return get


@pytest.mark.parametrize("name", ["M", "P"])
@pytest.mark.parametrize("path", ["device", "batches", "host", "uncompressed"])
def test_tiled_input_gives_what_the_strip_file_gives(tiled, name, path):
    """quicklook, overviews and cog itself write for a COG the bytes they write for the strip TIFF of the same pixels: LZW tiles
    decoded on the device, in one batch and in batches of one tile row, with OIP_TIFF_GPU_LZW=0 on the host, and uncompressed
    tiles of 64 (the host path)"""
    d, want = tiled(name)
    src, env, tools = {"device": (name + ".lzw.TIFF", {}, ("quicklook", "overviews", "cog")),
                       "batches": (name + ".lzw.TIFF", {"OIP_COG_BATCH_MB": "1"}, ("overviews",)),
                       "host": (name + ".lzw.TIFF", {"OIP_TIFF_GPU_LZW": "0"}, ("quicklook", "overviews")),
                       "uncompressed": ("in_none.TIFF", {}, ("overviews",))}[path]
    if path == "uncompressed":
        _run("cog", [name + ".TIFF", "-o", src, "--force", "--tiff-compress", "none", "--tile", "64", "--levels", "0"], d)
    for tool in tools:
        _run(tool, [src, "-o", "got." + OUTS[tool], "--force"], d, **env)
        assert _sha(os.path.join(d, "got." + OUTS[tool])) == want[tool], (src, env, tool)


@pytest.mark.parametrize("spp", [1, 4])
def test_tiles_of_48_x_32_read_on_the_host(tmp_path, spp):
    """a file of another writer: 48 x 32 tiles, zero padding, LZW with predictor 2 and uncompressed"""
    d = str(tmp_path)
    w, h = 130, 75
    img = _blocks(h, w, spp, 4 + spp)
    write_tiff_u16(os.path.join(d, "S.TIFF"), img.reshape(h, w, spp) if spp == 4 else img)
    _run("overviews", ["S.TIFF", "-o", "want.ovr"], d)
    for lzw in (True, False):
        cog.write_tiled_u16(os.path.join(d, "T.TIFF"), img, spp, 48, 32, lzw)
        dirs, _ = cog.read_tiled_dirs(os.path.join(d, "T.TIFF"))
        assert np.array_equal(dirs[0]["img"], img)
        _run("overviews", ["T.TIFF", "-o", "got.ovr", "--force"], d)
        assert _sha(os.path.join(d, "got.ovr")) == _sha(os.path.join(d, "want.ovr")), lzw


def _lzw_literals(data):
    """a legal LZW stream that no encoder writes and numpy packs at once: ClearCode before every 253 bytes, every byte its own
    9-bit code (the decoder's table stays below 511 entries, so no code ever widens), EndOfInformation"""
    a = np.frombuffer(data, np.uint8).astype(np.uint16)
    pad = (-len(a)) % 253
    g = np.concatenate([a, np.zeros(pad, np.uint16)]).reshape(-1, 253)
    codes = np.concatenate([np.full((len(g), 1), 256, np.uint16), g], axis=1).ravel()
    codes = np.concatenate([codes[:len(codes) - pad], [257]]).astype(np.uint16)
    bits = ((codes[:, None] >> np.arange(8, -1, -1)) & 1).astype(np.uint8)
    return np.packbits(bits.ravel()).tobytes()


def test_a_corrupt_lzw_tile_in_the_second_batch_is_named_with_its_batch(tmp_path):
    """4100 x 40 of 4 samples in LZW tiles of 16: three tile rows of 257 tiles, 514 KiB of samples each, so that OIP_COG_BATCH_MB=1
    (the smallest value the hook takes) makes a batch of every tile row -- the reader's stream helper runs three times.  Tile 262,
    the sixth of the second batch, starts with a code above 255: the device decoder counts a batch's tiles as the strips of a
    16-wide image and the reader adds where the batch began."""
    import _tiff
    d = str(tmp_path)
    w, h, T = 4100, 40, 16
    img = _blocks(h, w, 4, 11).reshape(h, w, 4)
    tx, ty = -(-w // T), -(-h // T)
    pad = np.zeros((ty * T, tx * T, 4), np.uint16)
    pad[:h, :w] = img
    tiles = pad.reshape(ty, T, tx, T, 4).transpose(0, 2, 1, 3, 4).reshape(ty * tx, T, T, 4).astype(np.int64)
    tiles[:, :, 1:] -= tiles[:, :, :-1].copy()                                            # predictor 2 along each tile row
    streams = [_lzw_literals((t & 0xFFFF).astype("<u2").tobytes()) for t in tiles]
    assert len(streams) == 771
    streams[262] = bytes([0x80, 0x4B, 0x00]) + streams[262][3:]                           # ClearCode, then code 300
    body, offs = b"", []
    for s in streams:
        body += b"\0" * (len(body) & 1)
        offs.append(8 + len(body))
        body += s
    _tiff.write_raw_tiff(os.path.join(d, "bad.TIFF"), {256: (4, [w]), 257: (4, [h]), 258: (3, [16] * 4), 259: (3, [5]), 262: (3, [2]), 277: (3, [4]),
                                                       284: (3, [1]), 317: (3, [2]), 322: (4, [T]), 323: (4, [T]), 324: (4, offs),
                                                       325: (4, [len(s) for s in streams]), 338: (3, [2]), 339: (3, [1] * 4)}, body)
    r = subprocess.run([OIP, "quicklook", "bad.TIFF", "-o", "bad.ql.TIFF"], cwd=d, env=dict(os.environ, LOGFILE=os.path.join(d, "oip.log"), OIP_COG_BATCH_MB="1"),
                       capture_output=True, text=True)
    assert r.returncode == 2 and "corrupt LZW stream (bad first code) in strip 5 (tiles from 257 on)" in r.stdout + r.stderr, r.stdout + r.stderr
