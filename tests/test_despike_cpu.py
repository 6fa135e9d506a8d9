"""CPU suite: the host side of `oip despike` -- the restatement itself (_despike_ref.py) on cases worked by hand, the
column table, the list files and the dead-column listing (oip_despike_column_table, oip_load_column_list,
oip_write_column_list, oip_rrc_dead_columns) against their restatements, and the argument surface of the sub-command and of
`oip rrc-calib --bad-pan / --bad-mss`.  Nothing here touches a GPU."""
import os
import subprocess

import numpy as np
import pytest

import opticalimageprocessor_amd as oip
import _despike_ref as ref
from _colstats_ref import totals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OIP = os.path.join(ROOT, "opticalimageprocessor_amd", "lib", "oip")


def _run(args, cwd, tool="despike"):
    env = dict(os.environ, LOGFILE=os.path.join(cwd, "oip.log"))
    return subprocess.run([OIP, tool] + args, cwd=cwd, env=env, capture_output=True, text=True)


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def test_restatement_one_spike():
    """[[10 11 12] [13 500 14] [15 16 17]], threshold 100.  Centre: the nine sorted are 10 .. 17, 500, the 5th is 14 and
    |500 - 14| = 486 > 100: replaced by 14, counted in column 1.  Corner (0, 0) with the border replicated sees
    10 10 11 / 10 10 11 / 13 13 500: sorted 10 10 10 10 11 11 13 13 500, median 11, |10 - 11| <= 100: kept.  Every other
    sample has at most one outlier among its nine, so its median lies in 10 .. 17 and it is kept."""
    img = np.array([[10, 11, 12], [13, 500, 14], [15, 16, 17]], np.uint16)
    out, cnt = ref.despike(img, 100, 0, 1)
    want = img.copy()
    want[1, 1] = 14
    assert np.array_equal(out, want) and cnt.tolist() == [0, 1, 0]
    # threshold 0: the plain median; the corner worked above becomes 11
    out0, cnt0 = ref.despike(img, 0, 0, 1)
    assert out0[0, 0] == 11 and out0[1, 1] == 14 and cnt0.sum() == (out0 != img).sum()


def test_restatement_no_data():
    """A zero centre passes through and is not counted, whatever surrounds it.  A zero neighbour stands in as the centre:
    700 amid eight zeros sees nine times 700 at valid_min 1 and is kept even at threshold 0; at valid_min 0 the zeros are
    data, the median is 0 and 700 is replaced."""
    hole = np.array([[10, 11, 12], [13, 0, 14], [15, 16, 17]], np.uint16)
    out, cnt = ref.despike(hole, 0, 0, 1)
    assert out[1, 1] == 0 and cnt[1] == (out[:, 1] != hole[:, 1]).sum() and (out[hole > 0] >= 1).all()
    lone = np.zeros((3, 3), np.uint16)
    lone[1, 1] = 700
    out, cnt = ref.despike(lone, 0, 0, 1)
    assert np.array_equal(out, lone) and not cnt.any()
    out, cnt = ref.despike(lone, 0, 0, 0)
    assert not out.any() and cnt.tolist() == [0, 1, 0]


def test_restatement_threshold_boundary():
    """A flat 1000 with another centre: every median is 1000.  thr_abs 50, thr_rel_q8 64: T = 50 + (1000 * 64 >> 8) = 50 + 250
    = 300.  d == 300 keeps, d == 301 replaces, on either side of the median."""
    for d, replaced in [(300, False), (301, True), (-300, False), (-301, True)]:
        img = np.full((3, 3), 1000, np.uint16)
        img[1, 1] = 1000 + d
        out, cnt = ref.despike(img, 50, 64, 1)
        assert (out[1, 1] == 1000) == replaced and out[1, 1] == (1000 if replaced else 1000 + d) and cnt.sum() == int(replaced)
    img = np.full((3, 3), 1000, np.uint16)
    img[1, 1] = 1051
    assert ref.despike(img, 50, 0, 1)[0][1, 1] == 1000 and ref.despike(img, 51, 0, 1)[0][1, 1] == 1051     # without the relative part


def test_restatement_channels_and_bands_never_mix():
    rng = np.random.default_rng(3)
    px = rng.integers(0, 65536, (9, 11, 4), dtype=np.uint16)
    px[rng.random(px.shape) < 0.05] = 0
    out, cnt = ref.despike(px.reshape(9, 44), 9000, 32, 1, spp=4)
    assert cnt.sum() > 0
    for c in range(4):                                              # 4 samples per pixel: four 1-sample runs
        o, n = ref.despike(px[:, :, c], 9000, 32, 1)
        assert np.array_equal(out.reshape(9, 11, 4)[:, :, c], o) and np.array_equal(cnt.reshape(11, 4)[:, c], n)
    line = rng.integers(0, 65536, (9, 28), dtype=np.uint16)          # groups 4: four independent runs on the band segments
    tab, _ = ref.column_table([0, 6, 7, 13, 27], 28, 4)
    out, cnt = ref.despike(line, 9000, 32, 1, groups=4, coltab=tab)
    for b in range(4):
        sub = tab[7 * b:7 * b + 7] - 7 * b
        o, n = ref.despike(line[:, 7 * b:7 * b + 7], 9000, 32, 1, coltab=sub)
        assert np.array_equal(out[:, 7 * b:7 * b + 7], o) and np.array_equal(cnt[7 * b:7 * b + 7], n)
    assert not np.array_equal(out, ref.despike(line, 9000, 32, 1, groups=1, coltab=ref.column_table([0, 6, 7, 13, 27], 28, 1)[0])[0])


@pytest.mark.parametrize("shape,spp", [((7, 9), 1), ((1, 5), 1), ((6, 1), 1), ((5, 12), 4)])
def test_restatement_plain_median_and_identity(shape, spp):
    rng = np.random.default_rng(shape[0] * 31 + shape[1])
    img = rng.integers(0, 65536, shape, dtype=np.uint16)
    L = shape[0]
    px = img.reshape(L, -1, spp)
    pad = np.pad(px, ((1, 1), (1, 1), (0, 0)), mode="edge")
    want = np.zeros_like(px)
    for y in range(L):
        for x in range(px.shape[1]):
            for c in range(spp):
                want[y, x, c] = sorted(pad[y:y + 3, x:x + 3, c].ravel().tolist())[4]
    out, cnt = ref.despike(img, 0, 0, 0, spp)
    assert np.array_equal(out, want.reshape(shape)) and np.array_equal(cnt, (out != img).sum(0))
    for vmin in (0, 1, 500):                                        # thr_abs 65535: |ctr - med| <= 65535 <= T, nothing is replaced
        out, cnt = ref.despike(img, 65535, 0, vmin, spp)
        assert np.array_equal(out, img) and not cnt.any()


def test_restatement_column_repair_arithmetic():
    """One line, thr_abs 65535 (the output is the repaired input), valid_min 1.
    D = 2, a = 10, b = 13: (10 + 13 + 1) / 2 = 12 (11.5 rounds up).
    D = 3, a = 10, b = 20: x = 1: (20 + 20 + 1) / 3 = 13 (13.33); x = 2: (10 + 40 + 1) / 3 = 17 (16.67 rounds up).
    D = 4, a = 10, b = 13: x = 1: (30 + 13 + 2) / 4 = 11 (10.75); x = 2: (20 + 26 + 2) / 4 = 12 (11.5 rounds up);
                           x = 3: (10 + 39 + 2) / 4 = 12 (12.25).
    An endpoint below valid_min: the other one is copied; both: b (no data stays no data)."""
    def repaired(vals, bad, vmin=1):
        img = np.array([vals], np.uint16)
        return ref.despike(img, 65535, 0, vmin, coltab=ref.column_table(bad, len(vals))[0])[0][0].tolist()
    assert repaired([10, 999, 13], [1]) == [10, 12, 13]
    assert repaired([10, 999, 999, 20], [1, 2]) == [10, 13, 17, 20]
    assert repaired([10, 999, 999, 999, 13], [1, 2, 3]) == [10, 11, 12, 12, 13]
    assert repaired([0, 999, 13], [1]) == [0, 13, 13]
    assert repaired([10, 999, 0], [1]) == [10, 10, 0]
    assert repaired([0, 999, 0], [1]) == [0, 0, 0]
    assert repaired([0, 999, 13], [1], vmin=0) == [0, 7, 13]        # valid_min 0: the zero is data, (0 + 13 + 1) / 2 = 7
    assert repaired([999, 999, 5, 6, 999], [0, 1, 4]) == [5, 5, 5, 6, 6]        # runs reaching an edge: a copy
    assert repaired([65535, 0, 65535], [1]) == [65535, 65535, 65535]
    # 65535 * W above int32: W = 40000 columns, all but the outer two listed; the middle column is the mean
    W = 40001
    img = np.zeros((1, W), np.uint16)
    img[0, 0], img[0, -1] = 65535, 65533
    out = ref.despike(img, 65535, 0, 1, coltab=ref.column_table(range(1, W - 1), W)[0])[0][0]
    assert out[W // 2] == 65534 and out[1] == 65535 and out[-2] == 65533


# ---- the column table -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,groups,bad", [
    (16, 1, []), (16, 1, [0]), (16, 1, [15]), (16, 1, [0, 15]), (16, 1, [5, 6, 7]), (16, 1, [0, 1, 2]), (16, 1, [13, 14, 15]),
    (32, 4, [7, 8, 15, 16, 23, 24]), (32, 4, [7]), (32, 4, [8]), (32, 4, [6, 7, 8, 9]), (32, 4, [0, 31]), (32, 4, list(range(8, 15))),
    (32, 1, [7, 8, 15, 16, 23, 24]), (12, 4, [0, 1, 4, 5, 8, 9, 10]), (1, 1, []), (16, 1, [9, 3, 3, 9, 4]),
])
def test_column_table_equals_restatement(w, groups, bad):
    tab, run = oip.despike_column_table(bad, w, groups)
    want, want_run = ref.column_table(bad, w, groups)
    assert np.array_equal(tab, want) and run == want_run
    gw = w // groups
    for x in range(w):
        lx, rx = tab[x]
        assert lx // gw == rx // gw == x // gw and lx not in bad and rx not in bad          # good columns of the same group
        if x not in bad:
            assert lx == rx == x
        elif lx != rx:
            assert lx < x < rx


def test_column_table_values():
    tab, run = oip.despike_column_table([0, 5, 6, 7, 15], 16)
    assert tab[0].tolist() == [1, 1] and tab[15].tolist() == [14, 14] and run == 3          # an edge: a copy
    assert [tab[x].tolist() for x in (5, 6, 7)] == [[4, 8]] * 3
    tab, run = oip.despike_column_table([7, 8], 32, 4)              # either side of a band border: never across it
    assert tab[7].tolist() == [6, 6] and tab[8].tolist() == [9, 9] and run == 1
    tab, run = oip.despike_column_table([7, 8], 32, 1)              # one group: a run of 2 between 6 and 9
    assert tab[7].tolist() == [6, 9] and tab[8].tolist() == [6, 9] and run == 2


def test_column_table_refusals():
    with pytest.raises(ValueError, match="group 2"):
        oip.despike_column_table(list(range(16, 24)), 32, 4)        # a whole band
    with pytest.raises(ValueError):
        ref.column_table(list(range(16, 24)), 32, 4)
    with pytest.raises(ValueError, match="group 0"):
        oip.despike_column_table([0], 1, 1)
    for bad, w, groups in [([16], 16, 1), ([-1], 16, 1), ([], 0, 1), ([], 18, 4), ([], 16, 2), ([], 16, 3)]:
        with pytest.raises(ValueError):
            oip.despike_column_table(bad, w, groups)
        with pytest.raises(ValueError):
            ref.column_table(bad, w, groups)


# ---- list files -----------------------------------------------------------------------------------------------------------------
def test_column_list_files(tmp_path):
    p = str(tmp_path / "bad.txt")
    open(p, "w").write("# dead detectors of CCD 1\n12 7\t7\n\n  3 # flickers\n#9\n+5\r\n0\n11#x\n")
    assert oip.load_column_list(p, 13).tolist() == [0, 3, 5, 7, 11, 12] == ref.parse_column_list(p, 13)
    for text in ["", "# nothing\n", "\n\n"]:                       # an empty list is valid
        open(p, "w").write(text)
        assert oip.load_column_list(p, 8).tolist() == [] == ref.parse_column_list(p, 8)
    for text in ["1 x 2\n", "1 2.5\n", "0x10\n", "1e2\n", "7-\n", "-\n", "3,4\n", "99999999999999999999\n", "13\n", "-1\n", "5 \x00 6\n", "4 # c\n12 13\n"]:
        open(p, "wb").write(text.encode())
        with pytest.raises(ValueError):
            oip.load_column_list(p, 13)
        with pytest.raises(ValueError):
            ref.parse_column_list(p, 13)
    open(p, "w").write("1 2 3 3 2 1\n")
    assert oip.load_column_list(p, 13, cap=3).tolist() == [1, 2, 3]  # duplicates do not count
    with pytest.raises(ValueError, match="room for 2"):
        oip.load_column_list(p, 13, cap=2)
    with pytest.raises(OSError):
        oip.load_column_list(str(tmp_path / "missing.txt"), 13)
    with pytest.raises(OSError):
        oip.load_column_list(str(tmp_path), 13)                      # a directory
    with pytest.raises(OSError):
        ref.parse_column_list(str(tmp_path / "missing.txt"), 13)
    # write -> load
    cols = [0, 4, 5, 4095]
    oip.write_column_list(p, cols, "from a test\nsecond line")
    text = open(p).read()
    assert text == "# from a test second line\n0\n4\n5\n4095\n"
    assert oip.load_column_list(p, 4096).tolist() == cols == ref.parse_column_list(p, 4096)
    oip.write_column_list(p, [], "none")                            # replaces the longer file
    assert open(p).read() == "# none\n" and oip.load_column_list(p, 4096).size == 0
    with pytest.raises(OSError):
        oip.write_column_list(str(tmp_path / "no" / "dir.txt"), cols)


# ---- the dead columns of the RRC fit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["moments", "gain"])
@pytest.mark.parametrize("groups", [1, 4])
def test_dead_columns_are_the_ones_the_fit_refuses(mode, groups):
    w, rows = 64, 50
    rng = np.random.default_rng(11)
    img = rng.integers(300, 3800, (rows, w)).astype(np.uint16)
    img[:, 5] = 1234                                                # constant: dead in moments mode, usable in gain mode
    img[:, 33] = 0                                                  # zero sum: dead in both
    img[:, 63] = 0
    acc = totals(img)
    acc[:, 40] = totals(img[:9, 40:41])[:, 0]                       # n = 9 < min_count: dead in both
    dead = oip.rrc_dead_columns(acc, mode, 10)
    assert dead.tolist() == ([5, 33, 40, 63] if mode == "moments" else [33, 40, 63])
    kb, per_group, _ = oip.rrc_fit_columns(acc, groups, mode, 10)
    identity = (kb[:, 0] == 1.0) & (kb[:, 1] == 0.0)
    assert np.flatnonzero(identity).tolist() == dead.tolist()       # listed exactly when the fit gives (1, 0)
    gw = w // groups
    assert [int(((dead // gw) == g).sum()) for g in range(groups)] == per_group.tolist()
    assert oip.rrc_dead_columns(acc, mode, 0).tolist() == [c for c in dead.tolist() if c != 40]
    assert oip.rrc_dead_columns(totals(rng.integers(300, 3800, (rows, w)).astype(np.uint16)), mode, 0).size == 0
    with pytest.raises(ValueError):
        oip.rrc_dead_columns(acc, 2, 0)


# ---- the sub-commands -----------------------------------------------------------------------------------------------------------
def _no_device(r):
    """exit code 2 is also what a missing GPU gives: the refusal must have come first"""
    return r.returncode == 2 and "MI355X" not in r.stdout


def test_cli_refusals_before_the_device(tmp_path):
    d = str(tmp_path)
    for name in ("P.RAW", "P.IMG", "P.TIFF"):
        np.zeros((8, 64), np.uint16).tofile(os.path.join(d, name))
    open(os.path.join(d, "ok.txt"), "w").write("# two\n3 40\n")
    base = ["P.RAW", "--width", "64"]
    thr = ["--threshold", "100"]
    r = _run(base, d)                                               # neither --threshold nor --bad-columns: no default threshold
    assert r.returncode == 254 and "USAGE ERROR" in r.stdout and "--threshold" in r.stdout
    assert _run(base + ["--relative", "0.1"], d).returncode == 254
    assert _run(base + ["--bad-columns", "ok.txt", "--relative", "0.1"], d).returncode == 107       # --relative needs --threshold
    assert _run(thr, d).returncode == 106                           # IMAGE is required
    assert _run(["missing.RAW"] + thr, d).returncode == 105
    assert _run(base + thr + ["--frobnicate"], d).returncode == 109
    for bad in (["--threshold", "-1"], ["--threshold", "65536"], thr + ["--relative", "-0.1"], thr + ["--relative", "1.5"],
                thr + ["--valid-min", "-1"], thr + ["--valid-min", "65536"], ["--bad-columns", "missing.txt"]):
        assert _run(base + bad, d).returncode == 105, bad
    assert _run(base + ["--threshold", "1e2"], d).returncode == 104
    r = _run(["P.IMG", "--width", "64"] + thr, d)                    # neither .RAW nor .TIFF
    assert _no_device(r) and "RAW and TIFF" in r.stdout
    for extra in (["--bad-columns", "ok.txt"], ["--bil"]):          # a product's columns are no longer detector columns
        r = _run(["P.TIFF"] + thr + extra, d)
        assert _no_device(r) and "RAW strip" in r.stdout, extra
    r = _run(["P.RAW", "--width", "60"] + thr, d)                    # 1024 bytes are not lines of 120
    assert _no_device(r) and "size invalid" in r.stdout
    r = _run(["P.RAW", "--width", "2", "--bil"] + thr, d)            # BIL: a multiple of 4
    assert _no_device(r) and "--width" in r.stdout
    r = _run(base + thr + ["-o", "out.TIFF"], d)                    # the container of the input
    assert _no_device(r) and "container" in r.stdout
    r = _run(base + thr + ["-o", "P.RAW"], d)
    assert _no_device(r) and "is the input image" in r.stdout
    r = _run(base + thr + ["--report", "P.RAW"], d)
    assert _no_device(r) and "P.RAW" in r.stdout
    r = _run(base + thr + ["--report", "P.DSPK.RAW"], d)            # the report is the (default) output
    assert _no_device(r) and "P.DSPK.RAW" in r.stdout
    # list files: a bad token, a column beyond the line, a whole band
    open(os.path.join(d, "tok.txt"), "w").write("3 4x\n")
    r = _run(base + ["--bad-columns", "tok.txt"], d)
    assert _no_device(r) and "tok.txt" in r.stdout and "4x" in r.stdout
    open(os.path.join(d, "far.txt"), "w").write("3 64\n")
    r = _run(base + ["--bad-columns", "far.txt"], d)
    assert _no_device(r) and "far.txt" in r.stdout
    open(os.path.join(d, "band.txt"), "w").write(" ".join(str(c) for c in range(16, 32)))
    r = _run(base + ["--bil", "--bad-columns", "band.txt"], d)
    assert _no_device(r) and "group 1" in r.stdout
    assert sorted(os.listdir(d)) == ["P.IMG", "P.RAW", "P.TIFF", "band.txt", "far.txt", "oip.log", "ok.txt", "tok.txt"]


@pytest.mark.parametrize("which", ["default", "named", "report"])
def test_cli_existing_output_is_refused_without_force(tmp_path, which):
    d = str(tmp_path)
    np.zeros((8, 64), np.uint16).tofile(os.path.join(d, "P.RAW"))
    name = {"default": "P.DSPK.RAW", "named": "mine.RAW", "report": "hits.txt"}[which]
    out = os.path.join(d, name)
    with open(out, "wb") as f:
        f.write(b"not a repaired strip")
    extra = {"default": [], "named": ["-o", "mine.RAW"], "report": ["--report", "hits.txt"]}[which]
    r = _run(["P.RAW", "--width", "64", "--threshold", "100"] + extra, d)
    assert _no_device(r) and name in r.stdout and "--force" in r.stdout
    assert open(out, "rb").read() == b"not a repaired strip"


def test_rrc_calib_bad_list_arguments(tmp_path):
    d = str(tmp_path)
    np.zeros((8, 64), np.uint16).tofile(os.path.join(d, "P.RAW"))
    msb = []
    for b in range(4):
        msb += ["--rrc-msb%d" % (b + 1), "m%d.csv" % (b + 1)]
    pan = ["--width", "64", "--pan", "P.RAW", "--rrc-pan", "pan.csv"]
    assert _run(["--width", "64", "--bad-pan", "bad.txt"], d, "rrc-calib").returncode == 107        # a list comes with its image
    assert _run(pan + ["--bad-mss", "bad.txt"], d, "rrc-calib").returncode == 107
    assert _run(["--width", "64", "--mss", "P.RAW", "--bad-pan", "bad.txt"] + msb, d, "rrc-calib").returncode == 107
    r = _run(pan + ["--bad-pan", "pan.csv"], d, "rrc-calib")         # one file for two outputs
    assert _no_device(r) and "two outputs" in r.stdout
    r = _run(["--width", "64", "--pan", "P.RAW", "--rrc-pan", "pan.csv", "--mss", "P.RAW", "--bad-pan", "b.txt", "--bad-mss", "b.txt"] + msb, d, "rrc-calib")
    assert _no_device(r) and "two outputs" in r.stdout
    open(os.path.join(d, "bad.txt"), "w").write("kept")
    r = _run(pan + ["--bad-pan", "bad.txt"], d, "rrc-calib")         # under the same --force rule
    assert _no_device(r) and "bad.txt" in r.stdout and "--force" in r.stdout
    assert open(os.path.join(d, "bad.txt")).read() == "kept" and not os.path.exists(os.path.join(d, "pan.csv"))


def test_help_lists_the_sub_command(tmp_path):
    r = subprocess.run([OIP, "--help"], cwd=str(tmp_path), capture_output=True, text=True)
    assert r.returncode == 255 and "despike" in r.stdout and "--bad-columns" in r.stdout and "--threshold" in r.stdout
    assert "--bad-pan" in r.stdout and "--bad-mss" in r.stdout
