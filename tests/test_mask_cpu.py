"""CPU: the mask of `oip mask` (include/oip_c.h, section "mask") as its numpy restatement (_mask_ref.py) states it -- the
properties the header claims of the opening and the buffer, strips cut into calls, the counters, every combination of disabled
tests, the crafted cells at equality of each test, and the ground truth of a synthetic scene with clouds and bright roofs --;
the two host entry points against the restatement; the stand-alone program of the report and of read_tiff_u8; and what
`oip mask` and `oip regcheck --mask` refuse before a device is touched."""
import os
import subprocess

import numpy as np
import pytest

import opticalimageprocessor_amd as oip
from opticalimageprocessor_amd import capi
import _mask_ref as ref
from _tiff import write_tiff_u16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OIP = os.path.join(ROOT, "opticalimageprocessor_amd", "lib", "oip")


# ---- the properties include/oip_c.h claims -------------------------------------------------------------------------------------
@pytest.mark.parametrize("gh,gw,density", [(40, 90, 0.5), (40, 90, 0.97), (7, 5, 0.9), (1, 70, 0.97), (30, 1, 0.97)])
def test_opening_and_buffer_properties(gh, gw, density):
    f = ref.flag_grid(gh, gw, density, gh + gw)
    X = f & ref.CANDIDATE != 0
    assert np.array_equal(ref.opening(X, 0), X)                                           # a = 0: identity
    previous = None
    for a in (1, 2, 7, 32):
        O = ref.opening(X, a)
        assert not (O & ~X).any()                                                         # O is a subset of X
        assert np.array_equal(ref.opening(O, a), O)                                       # idempotent
    for d in (0, 1, 5, 64):
        out, (n_cloud, n_buffer) = ref.morph(f, 1, d)
        D = out & (ref.CLOUD | ref.BUFFER) != 0
        assert previous is None or not (previous & ~D).any()                              # D grows with d
        previous = D
        assert np.array_equal(out & 19, f & 19)                                           # bits 1, 2, 16 are kept
        assert not ((out & ref.CLOUD != 0) & (out & ref.BUFFER != 0)).any()
        again, counts = ref.morph(out, 1, d)                                              # a second call changes nothing
        assert np.array_equal(again, out) and counts == (n_cloud, n_buffer)
        rc = ref.recount(out)
        assert (rc[5], rc[6]) == (n_cloud, n_buffer)
    assert ref.morph(f, 1, 0)[1][1] == 0 and (ref.morph(ref.flag_grid(gh, gw, 1.0, 1), 32, 64)[0] & ref.CLOUD != 0).all()


@pytest.mark.parametrize("spp,C", [(4, 4), (4, 8), (4, 16), (1, 4), (1, 8), (1, 16)])
def test_a_strip_cut_into_calls_and_the_counters(spp, C):
    rows, w = 5 * C + 3, 3 * C + 1
    img = ref.random_raster(rows, w * spp, 11 + C + spp)
    whole, counts = ref.cells(img, spp, C)
    assert whole.shape == (6, 4)
    parts, total = [], np.zeros(8, np.uint64)
    for a, b in ((0, C), (C, 4 * C), (4 * C, rows)):
        f, c = ref.cells(img[a:b], spp, C)
        parts.append(f)
        total += c
    assert np.array_equal(np.concatenate(parts), whole) and np.array_equal(total, counts)
    rc = ref.recount(whole)
    assert all(int(counts[k]) == v for k, v in rc.items() if k < 5)
    assert int(counts[7]) > 0 and (spp == 4) == bool(counts[3]) and (spp == 4 or counts[4] == 0)
    assert (whole & ref.NODATA).any() and (whole & ref.SATURATED).any()


def test_every_combination_of_disabled_tests():
    """on the crafted cells: a cell that fails test i alone (k = -1) is a candidate exactly when test i is disabled; with every
    test disabled CANDIDATE is `tested`; disabling a test never removes a candidate"""
    C = 8
    img, cases = ref.edge_raster(C)
    kw = dict(valid_min=1, sat_level=65535, full=ref.EDGE_FULL)
    base = None
    switches = ref.all_switches(ref.EDGE_Q8)
    assert len(set(switches)) == 16 and switches[0] == ref.EDGE_Q8
    for q8 in switches:
        f, counts = ref.cells(img, 4, C, q8=q8, **kw)
        cand = (f[0] & ref.CANDIDATE) != 0
        for i, (test, k, _) in enumerate(cases):
            assert cand[i] == (k >= 0 or q8[test] < 0), (q8, test, k)
        if base is None:
            base = cand
        assert not (base & ~cand).any()
        if q8 == (-1, -1, -1, -1):
            assert cand.all() and counts[4] == counts[3] == len(cases)


@pytest.mark.parametrize("C", [4, 8, 16])
def test_crafted_cells_sit_on_both_sides_of_equality(C):
    """margins(): at k = 0 the decided test is at equality, at -1 it fails, at +1 it passes, and the other three pass with room"""
    m = C * C
    for test, k, sums in ref.edge_cases(C):
        mg = ref.margins(sums, m, ref.EDGE_FULL, ref.EDGE_Q8)
        assert (mg[test] == 0) == (k == 0) and (mg[test] < 0) == (k < 0), (test, k, mg)
        assert all(v > 1000 for i, v in enumerate(mg) if i != test), (test, k, mg)
    img, cases = ref.edge_raster(C, band=(3, 0, 2, 1))
    f, _ = ref.cells(img, 4, C, 1, 65535, ref.EDGE_FULL, (3, 0, 2, 1), ref.EDGE_Q8)
    assert [bool(v & ref.CANDIDATE) for v in f[0]] == [k >= 0 for _, k, _ in cases]
    # the sums the cells were built from are the sums the restatement sees
    px = img.reshape(C, -1, 4).astype(np.int64)
    for i, (_, _, sums) in enumerate(cases):
        got = px[:, i * C:(i + 1) * C].sum(axis=(0, 1))
        assert tuple(int(got[c]) for c in (3, 0, 2, 1)) == tuple(sums)


def test_partial_cells_are_tested_against_their_own_size():
    """2 m >= n_cell with n_cell the pixels the cell holds: a 3 x 3 image is one cell of 9 pixels"""
    img = np.full((3, 12), 3000, np.uint16)
    f, counts = ref.cells(img, 4, 8)
    assert f.shape == (1, 1) and counts[3] == 1 and f[0, 0] == ref.CANDIDATE
    img[:2] = 0                                                                           # 6 of 9 without data: 2 * 3 < 9
    f, counts = ref.cells(img, 4, 8)
    assert counts[3] == 0 and f[0, 0] == ref.NODATA
    f, counts = ref.cells(img, 4, 8, valid_min=0)                                          # zeros are data: dark, no candidate
    assert counts[3] == 1 and f[0, 0] == 0


# ---- ground truth ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_scene_ground_truth(seed):
    """scene(512, 768, seed) at cell 8, 10 bits, open 1, buffer 2, default fractions"""
    dn, cloud, _ = ref.scene(512, 768, seed)
    kw = dict(valid_min=1, sat_level=ref.FULL10, full=ref.FULL10, band=ref.SCENE_BAND)
    f, counts = ref.mask(dn.reshape(512, -1), 4, 8, 1, 2, **kw)
    n_cloud_px = ref._cell_sums(cloud, 8)
    is_cloud, in_d = f & ref.CLOUD != 0, f & (ref.CLOUD | ref.BUFFER) != 0
    assert (n_cloud_px == 64).any() and is_cloud[n_cloud_px == 64].all()                  # every cell that is all cloud has CLOUD
    assert not is_cloud[n_cloud_px == 0].any()                                            # no cell without a cloud pixel has it
    assert in_d[n_cloud_px > 0].all()                                                     # every cell with a cloud pixel: CLOUD or BUFFER
    roofs = (f & ref.CANDIDATE != 0) & (n_cloud_px == 0)
    assert roofs.sum() >= 10                                                              # candidates without a cloud pixel: the roofs
    f0, _ = ref.mask(dn.reshape(512, -1), 4, 8, 0, 2, **kw)
    assert (f0 & ref.CLOUD != 0)[roofs].all()                                             # open 0 leaves them in
    assert counts[0] == 64 * 96 and counts[1] == 0 and counts[5] == is_cloud.sum()


# ---- host entry points ------------------------------------------------------------------------------------------------------------
def test_mask_grid_and_tile_flag_against_the_restatement():
    for w, h, C in ((202, 77, 8), (203, 77, 4), (3, 3, 16), (16, 16, 16), (0, 0, 8), (1024, 64, 8)):
        assert capi.mask_grid(w, h, C) == ref.grid(w, h, C)
    for bad in ((10, 10, 5), (-1, 10, 8), (10, -1, 8)):
        with pytest.raises(ValueError):
            capi.mask_grid(*bad)
    rng = np.random.default_rng(5)
    for C, (w, h) in ((4, (37, 22)), (8, (70, 41)), (16, (70, 41))):
        gw, gh = ref.grid(w, h, C)
        f = np.where(rng.random((gh, gw)) < 0.15, rng.choice([4, 8, 16, 1], (gh, gw)), 0).astype(np.uint8)
        rects = [(0, 0, w, h), (0, 0, 1, 1), (w - 1, h - 1, 1, 1), (w - 1, h - 1, 50, 50), (-5, -5, 5, 5), (-5, -5, 6, 6), (w, 0, 4, 4), (3, 3, 0, 4)]
        for _ in range(150):
            x, y = int(rng.integers(-C, w + C)), int(rng.integers(-C, h + C))
            rects.append((x, y, int(rng.integers(1, 3 * C)), int(rng.integers(1, 3 * C))))
        for j in range(min(gh, 3)):                                                       # rectangles on cell borders
            for i in range(min(gw, 4)):
                rects += [(i * C, j * C, C, C), (i * C - 1, j * C, 1, C), (i * C + C, j * C + C, 1, 1), (i * C, j * C - 1, C, 1)]
        hits = 0
        for x, y, tw, th in rects:
            for bits in (12, 4, 16):
                want = ref.tile_flag(f, C, x, y, tw, th, bits)
                assert capi.mask_tile_flag(f, C, x, y, tw, th, bits) == want, (C, x, y, tw, th, bits)
                hits += want
        assert 0 < hits < 3 * len(rects)
        wide = np.zeros((gh, gw + 3), np.uint8)                                           # a pitch wider than the grid: the bytes behind a line do not count
        wide[:, :gw], wide[:, gw:] = f, 255
        assert capi.mask_tile_flag(wide[:, :gw], C, 0, 0, w + 100, h + 100, 32) is False


def test_maskreport_program(tmp_path):
    """tests/cpp/maskreport_test.cpp: the q8 form, the report writer, read_tiff_u8 on write_tiff_u8's output (one strip, several)
    and its refusals (truncated, 16-bit, 3 samples, compressed), the two host entry points -- under ASan + UBSan, a program of
    its own"""
    src = [os.path.join(ROOT, "tests", "cpp", "maskreport_test.cpp"), os.path.join(ROOT, "opticalimageprocessor_amd", "csrc", "host.cpp")]
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "opticalimageprocessor_amd", "csrc")]
    exe = tmp_path / "maskreport_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + inc + src +
                   ["-o", str(exe)], check=True)
    r = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and " checks, 0 bad" in r.stdout and "FAILED" not in r.stdout, r.stdout + r.stderr
    assert int(r.stdout.split()[-4]) >= 40, r.stdout                   # every part ran


def test_the_new_symbols_are_bound():
    assert oip.capi.load_library() is not None
    for name in ("oip_mask_cells_u16", "oip_mask_morph_u8", "oip_mask_grid", "oip_mask_tile_flag"):
        assert name in capi.declared_symbols() and name in capi._SIGS
    assert hasattr(oip.Context, "mask_cells_u16") and hasattr(oip.Context, "mask_morph_u8")


# ---- the command line, before a device is touched ---------------------------------------------------------------------------------
def test_cli_refusals_need_no_device(tmp_path):
    """what run_mask / run_regcheck (option values: 104-109) and MaskCheck / RegcheckCheck (the file, the outputs: 2) refuse; after
    every row the directory holds what it held before"""
    d = str(tmp_path)
    rng = np.random.default_rng(3)
    rng.integers(1, 4096, (32, 64), dtype=np.uint16).tofile(os.path.join(d, "P.RAW"))
    write_tiff_u16(os.path.join(d, "P.TIFF"), rng.integers(1, 4096, (32, 64, 4), dtype=np.uint16))
    write_tiff_u16(os.path.join(d, "T3.TIFF"), rng.integers(1, 4096, (32, 64, 3), dtype=np.uint16))
    open(os.path.join(d, "P.BIN"), "wb").write(b"\0" * 128)
    open(os.path.join(d, "there.TIFF"), "wb").write(b"kept")
    open(os.path.join(d, "there.CSV"), "w").write("kept")
    env = dict(os.environ, LOGFILE=os.path.join(d, "oip.log"))
    files = lambda: {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d)) if n != "oip.log"}   # noqa: E731
    before = files()
    raw = ["P.RAW", "--width", "64"]
    exists = "exists: mask does not replace a file without --force"
    mask = (
        ([], 106, "IMAGE is required"), (["missing.RAW"], 105, "does not exist"),
        (raw + ["--cell", "5"], 105, "--cell: 4, 8 or 16 expected"), (raw + ["--cell", "32"], 105, "--cell"), (raw + ["--cell", "x"], 104, "Could not convert"),
        (raw + ["--bits", "7"], 105, "--bits: 8 <= N <= 16 expected"), (raw + ["--bits", "17"], 105, "--bits"),
        (raw + ["--bands", "1,1,2,3"], 105, "--bands: B,G,R,N, a permutation of the channels 1,2,3,4, expected"),
        (raw + ["--bands", "1,2,3"], 105, "--bands"), (raw + ["--bands", "1,2,3,5"], 105, "--bands"), (raw + ["--bands", "1,2,3,4,"], 105, "--bands"),
        (raw + ["--bright", "1.5"], 105, "--bright: a fraction 0 <= F <= 1 expected"), (raw + ["--white", "-0.1"], 105, "--white"),
        (raw + ["--hot", "nan"], 105, "--hot"), (raw + ["--ndvi", "2"], 105, "--ndvi"), (raw + ["--ndvi", "x"], 104, "Could not convert"),
        (raw + ["--open", "33"], 105, "--open: 0 <= A <= 32 expected"), (raw + ["--open", "-1"], 105, "--open"),
        (raw + ["--buffer", "65"], 105, "--buffer: 0 <= D <= 64 expected"), (raw + ["--buffer", "-1"], 105, "--buffer"),
        (raw + ["--saturation", "0"], 105, "--saturation: 1 <= DN <= 65535 expected"), (raw + ["--saturation", "65536"], 105, "--saturation"),
        (raw + ["--valid-min", "65536"], 105, "--valid-min: 0 <= N <= 65535 expected"),
        (["P.RAW", "--width", "0"], 105, "--width: a positive line width expected"), (raw + ["--bil"], 109, "was not expected"),
        (["P.BIN"], 2, "mask: only RAW and TIFF image supported"),
        (["P.RAW", "--width", "63"], 2, "image file size invalid: should be multiplies of 126"),
        (["T3.TIFF"], 2, "mask: a TIFF of 1 or 4 samples per pixel expected"),
        (raw + ["-o", "there.TIFF"], 2, "output file [there.TIFF] " + exists), (raw + ["--report", "there.CSV"], 2, "output file [there.CSV] " + exists),
        (raw + ["-o", "P.RAW", "--force"], 2, "output file [P.RAW] is the input image"),
        (["P.TIFF", "-o", "P.TIFF", "--force"], 2, "output file [P.TIFF] is the input image"),
        (["P.TIFF", "--report", "P.TIFF", "--force"], 2, "output file [P.TIFF] is the input image"),
        (raw + ["-o", "x.TIFF", "--report", "x.TIFF"], 2, "is named for the mask and for the report"),
    )
    reg = ["--image1", "P.RAW", "--width", "64", "--tile", "8", "--search", "1"]
    regcheck = (
        (reg + ["--mask", "there.TIFF"], 107, "--mask requires --mask-cell"),
        (reg + ["--mask-cell", "8"], 107, "--mask-cell / --mask-bits require --mask"), (reg + ["--mask-bits", "4"], 107, "require --mask"),
        (reg + ["--mask", "missing.TIFF", "--mask-cell", "8"], 105, "--mask: File does not exist"),
        (reg + ["--mask", "there.TIFF", "--mask-cell", "5"], 105, "--mask-cell: 4, 8 or 16 expected"),
        (reg + ["--mask", "there.TIFF", "--mask-cell", "8", "--mask-bits", "0"], 105, "--mask-bits: 1 <= B <= 255 expected"),
        (reg + ["--mask", "there.TIFF", "--mask-cell", "8", "--mask-bits", "256"], 105, "--mask-bits"),
        (reg + ["--mask", "there.TIFF", "--mask-cell", "8"], 2, "read 8-bit TIFF [there.TIFF]: truncated file"),
        (reg + ["--mask", "P.TIFF", "--mask-cell", "8"], 2, "read 8-bit TIFF [P.TIFF]: 16-bit samples are not supported"),
    )
    bad = []
    for tool, table in (("mask", mask), ("regcheck", regcheck)):
        for args, code, text in table:
            r = subprocess.run([OIP, tool] + args, cwd=d, env=env, capture_output=True, text=True)
            if r.returncode != code or text not in r.stdout + r.stderr:
                bad.append((tool, args, code, text, r.returncode, r.stdout + r.stderr))
            assert files() == before, args
    assert not bad, "\n".join(map(repr, bad))
    usage = subprocess.run([OIP, "--help"], cwd=d, env=env, capture_output=True, text=True).stdout
    assert "mask       IMAGE.TIFF|IMAGE.RAW" in usage and "--mask FILE --mask-cell C" in usage and "nothing was measured on real imagery" in usage
