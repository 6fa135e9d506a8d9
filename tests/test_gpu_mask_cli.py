"""GPU: `oip mask` and `oip regcheck --mask` end to end -- the mask TIFF's bytes and the report's counters are the restatement's
(_mask_ref.py) on a 4-band TIFF and on a RAW strip streamed in several blocks; --no-cloud and --force do what they say; regcheck
flags exactly the tiles whose template touches a masked cell and changes nothing else; regfix loads such a report and leaves
those tiles out."""
import os
import struct
import subprocess

import numpy as np
import pytest

from opticalimageprocessor_amd import capi
import _mask_ref as ref
from _tiff import write_tiff_u16

pytestmark = pytest.mark.gpu
OIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "opticalimageprocessor_amd", "lib", "oip")
H, W = 256, 384
SCENE_KW = dict(valid_min=1, sat_level=ref.FULL10, full=ref.FULL10, band=ref.SCENE_BAND)
SCENE_ARGS = ["--bits", "10", "--bands", "1,2,3,4"]


def _run(tool, args, cwd, **env):
    env = dict(os.environ, LOGFILE=os.path.join(cwd, "oip.log"), **env)
    return subprocess.run([OIP, tool] + args, cwd=cwd, env=env, capture_output=True, text=True)


def _ok(r):
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def _read_mask(path):
    """an 8-bit, one-sample, one-strip classic TIFF as `oip mask` writes a small grid: (gh, gw) uint8"""
    b = open(path, "rb").read()
    assert b[:4] == b"II*\0"
    ifd, = struct.unpack_from("<I", b, 4)
    n, = struct.unpack_from("<H", b, ifd)
    tags = {}
    for k in range(n):
        tag, typ, cnt, val = struct.unpack_from("<HHII", b, ifd + 2 + 12 * k)
        tags[tag] = (val & 0xFFFF) if typ == 3 else val
    assert tags[258] == 8 and tags[259] == 1 and tags[277] == 1 and tags[279] == tags[256] * tags[257]
    return np.frombuffer(b, np.uint8, tags[279], tags[273]).reshape(tags[257], tags[256])


def _read_report(path):
    lines = open(path).read().splitlines()
    assert lines[0].startswith("# oip mask image=")
    vals = dict(ln.split(",") for ln in lines[1:])
    return lines[0], [int(vals[k]) for k in capi.MASK_COUNTERS], {k: vals[k] for k in vals if k.endswith("_pct")}


def _pct(counts):
    c = [float(v) for v in counts]
    return {"nodata_pct": "%.4f" % (100 * c[1] / c[0]), "saturated_pct": "%.4f" % (100 * c[2] / c[0]), "cloud_pct": "%.4f" % (100 * c[5] / c[0]),
            "cloud_or_buffer_pct": "%.4f" % (100 * (c[5] + c[6]) / c[0])}


@pytest.fixture(scope="module")
def scene():
    dn, cloud, _ = ref.scene(H, W, 0)
    return dn, cloud


def test_four_band_tiff(tmp_path, scene):
    d = str(tmp_path)
    dn, _ = scene
    write_tiff_u16(os.path.join(d, "S.TIFF"), dn)
    r = _ok(_run("mask", ["S.TIFF"] + SCENE_ARGS, d))
    want, wc = ref.mask(dn.reshape(H, -1), 4, 8, 1, 2, **SCENE_KW)
    assert (want & ref.CLOUD).any() and (want & ref.BUFFER).any() and ((want & ref.CANDIDATE != 0) & (want & ref.CLOUD == 0)).any()
    assert np.array_equal(_read_mask(os.path.join(d, "S.MASK.TIFF")), want)
    head, counts, pct = _read_report(os.path.join(d, "S.MASK.CSV"))
    assert counts == [int(v) for v in wc] and pct == _pct(wc)
    assert head == ("# oip mask image=S.TIFF cell=8 width=%d height=%d bits=10 saturation=1023 valid-min=1 bands=1,2,3,4 bright-q8=77 white-q8=38 "
                    "hot-q8=20 ndvi-q8=51 open=1 buffer=2" % (W, H))
    assert "cloud %d (%s %%)" % (wc[5], _pct(wc)["cloud_pct"]) in r.stdout and "MBps" in r.stdout
    # an existing mask or report: refused, then replaced with --force; other options, other bytes
    before = open(os.path.join(d, "S.MASK.TIFF"), "rb").read()
    r = _run("mask", ["S.TIFF"] + SCENE_ARGS + ["--cell", "16", "--open", "0", "--buffer", "5"], d)
    assert r.returncode == 2 and "--force" in r.stdout and open(os.path.join(d, "S.MASK.TIFF"), "rb").read() == before
    _ok(_run("mask", ["S.TIFF"] + SCENE_ARGS + ["--cell", "16", "--open", "0", "--buffer", "5", "--force", "--saturation", "700", "--white", "0.1"], d))
    want, wc = ref.mask(dn.reshape(H, -1), 4, 16, 0, 5, **dict(SCENE_KW, sat_level=700, q8=(77, 26, 20, 51)))
    assert np.array_equal(_read_mask(os.path.join(d, "S.MASK.TIFF")), want) and (want & ref.SATURATED).any()
    assert _read_report(os.path.join(d, "S.MASK.CSV"))[1] == [int(v) for v in wc]
    # --no-cloud: bits 1 and 2 alone, no tested cell
    _ok(_run("mask", ["S.TIFF"] + SCENE_ARGS + ["--no-cloud", "--saturation", "700", "-o", "n.TIFF", "--report", "n.csv"], d))
    want, wc = ref.cells(dn.reshape(H, -1), 4, 8, **dict(SCENE_KW, sat_level=700))
    got = _read_mask(os.path.join(d, "n.TIFF"))
    assert np.array_equal(got, want & 3) and got.any()
    head, counts, _ = _read_report(os.path.join(d, "n.csv"))
    assert counts == [int(wc[0]), int(wc[1]), int(wc[2]), 0, 0, 0, 0, int(wc[7])] and "bright-q8=-1" in head and "open=0 buffer=0" in head


def test_raw_strip_in_several_blocks(tmp_path):
    """one band, 200 lines streamed in blocks of 48 (OIP_MASK_BLOCK_LINES 50, rounded down to a multiple of the cell), a zero-filled
    32-line block inside as the de-framer leaves for lost frames; no cloud stage, and the log says so"""
    d = str(tmp_path)
    L, w = 200, 333
    img = ref.random_raster(L, w, 9)
    img[img == 0] = 7
    img[72:104] = 0
    img.tofile(os.path.join(d, "P.RAW"))
    r = _ok(_run("mask", ["P.RAW", "--width", str(w), "--cell", "16"], d, OIP_MASK_BLOCK_LINES="50"))
    assert "the cloud tests need four and are skipped" in r.stdout
    want, wc = ref.cells(img, 1, 16, valid_min=1, sat_level=4095, full=4095)
    assert (want[5] & ref.NODATA).all() and not (want[3] & ref.NODATA).any() and (want & ref.SATURATED).any()
    assert np.array_equal(_read_mask(os.path.join(d, "P.MASK.TIFF")), want)
    head, counts, pct = _read_report(os.path.join(d, "P.MASK.CSV"))
    assert counts == [int(v) for v in wc] and pct == _pct(wc) and "width=333 height=200" in head
    _ok(_run("mask", ["P.RAW", "--width", str(w), "--cell", "16", "-o", "one.TIFF", "--report", "one.csv"], d))      # one block: the same files
    assert open(os.path.join(d, "one.TIFF"), "rb").read() == open(os.path.join(d, "P.MASK.TIFF"), "rb").read()
    assert open(os.path.join(d, "one.csv")).read() == open(os.path.join(d, "P.MASK.CSV")).read()


def test_regcheck_mask_and_regfix(tmp_path, scene):
    """band 2 = band 1 moved by one pixel: every tile measures that shift, and the tiles over the discs carry flag 16"""
    d = str(tmp_path)
    dn, cloud = scene
    write_tiff_u16(os.path.join(d, "S.TIFF"), dn)
    two = dn.copy()
    two[:, :, 1] = np.roll(dn[:, :, 0], 1, axis=1)
    write_tiff_u16(os.path.join(d, "B.TIFF"), two)
    _ok(_run("mask", ["S.TIFF"] + SCENE_ARGS, d))
    T = 32
    base = ["--image1", "B.TIFF", "--band1", "1", "--band2", "2", "--tile", str(T), "--search", "2", "--min-score", "0.2"]
    _ok(_run("regcheck", base + ["-o", "plain.csv"], d))
    r = _ok(_run("regcheck", base + ["-o", "masked.csv", "--mask", "S.MASK.TIFF", "--mask-cell", "8"], d))
    plain, masked = open(os.path.join(d, "plain.csv")).read().splitlines(), open(os.path.join(d, "masked.csv")).read().splitlines()
    assert " mask-bits=12 columns=" in masked[0] and masked[0].replace(" mask-bits=12", "") == plain[0] and "mask" not in plain[0]
    mask, _ = ref.mask(dn.reshape(H, -1), 4, 8, 1, 2, **SCENE_KW)
    tiles_p = [ln for ln in plain[1:] if not ln.startswith("#")]
    tiles_m = [ln for ln in masked[1:] if not ln.startswith("#")]
    assert len(tiles_p) == len(tiles_m) > 20
    n_masked = n_over_cloud = 0
    for p, m in zip(tiles_p, tiles_m):
        fp, fm = p.split(","), m.split(",")
        assert fp[:5] == fm[:5]                                                           # x, y, dx, dy, score: byte for byte
        x, y = int(fp[0]) - T // 2, int(fp[1]) - T // 2
        hit = ref.tile_flag(mask, 8, x, y, T, T, 12)
        assert int(fm[5]) == int(fp[5]) | (16 if hit else 0)
        n_masked += hit
        if cloud[y:y + T, x:x + T].any():
            assert hit
            n_over_cloud += 1
    assert 0 < n_over_cloud <= n_masked < len(tiles_p)
    assert "masked %d" % n_masked in r.stdout and "masked" not in "".join(ln for ln in plain if ln.startswith("#"))
    # --mask-bits 4: cloud alone flags fewer tiles; a mask of another grid is refused with both sizes
    _ok(_run("regcheck", base + ["-o", "cloud.csv", "--mask", "S.MASK.TIFF", "--mask-cell", "8", "--mask-bits", "4"], d))
    n4 = sum(int(ln.split(",")[5]) & 16 != 0 for ln in open(os.path.join(d, "cloud.csv")).read().splitlines() if not ln.startswith("#"))
    assert 0 < n4 <= n_masked and " mask-bits=4 " in open(os.path.join(d, "cloud.csv")).readline()
    r = _run("regcheck", base + ["-o", "x.csv", "--mask", "S.MASK.TIFF", "--mask-cell", "16"], d)
    assert r.returncode == 2 and "48 x 32 cells" in r.stdout and "24 x 16 cells of 16" in r.stdout and not os.path.exists(os.path.join(d, "x.csv"))
    # regfix loads both reports; its node set is the tiles without a flag
    used = {}
    for name, tiles in (("plain.csv", tiles_p), ("masked.csv", tiles_m)):
        _, _, geom = capi.regfix_load_report(os.path.join(d, name), W, H)
        used[name] = geom["used"]
        assert geom["used"] == sum(int(t.split(",")[5]) == 0 for t in tiles)
    assert used["masked.csv"] < used["plain.csv"]
    _ok(_run("regfix", ["--report", "masked.csv", "--image", "B.TIFF"], d))
