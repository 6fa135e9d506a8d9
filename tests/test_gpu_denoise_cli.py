"""GPU: `oip denoise` end to end -- the product is the restatement's (_denoise_ref.py) of the input file's samples, sample for
sample, in the container of the input, however the strip is cut into line blocks; the log's counters are the restatement's; a
report of another band count is refused before a pixel is filtered; and the loop noise -> denoise -> noise shows the measured
sigma falling by at least the bar of the CPU test."""
import os
import re
import subprocess

import numpy as np
import pytest

import _denoise_ref as ref
import _noise_ref
from _tiff import read_tags, read_tiff_u16, write_tiff_u16

pytestmark = pytest.mark.gpu
OIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "opticalimageprocessor_amd", "lib", "oip")


def _run(tool, args, cwd, **env):
    env = dict(os.environ, LOGFILE=os.path.join(cwd, "oip.log"), **env)
    return subprocess.run([OIP, tool] + args, cwd=cwd, env=env, capture_output=True, text=True)


def _band_line(k, a, b):
    return "# band %d: blocks 10 nodata 0 structured 2 levels 3 a %r b %r mu_ref 1896 sigma_ref 5.2 snr_ref 364.6\n" % (k, a, b)


def _counters(stdout):
    m = re.search(r"counters: valid (\d+) alone (\d+) members (\d+) changed (\d+)", stdout)
    assert m, stdout
    return [int(v) for v in m.groups()]


def _thresholds_logged(stdout):
    return [[int(v) for v in m.groups()] for m in re.finditer(r"band \d+ thresholds at levels 0, 64, 128, 255: (\d+) (\d+) (\d+) (\d+)", stdout)]


def test_raw_strip_in_several_line_blocks(tmp_path):
    """96 x 500 through --noise.  OIP_DENOISE_BLOCK_LINES forces line blocks of 64 lines (eight blocks: both device blocks of
    either kind are reused, the two halo lines above and below a block come from the file, the last block is short), of 7 lines
    and the tool's own single block: the same bytes.  The default name, -o, the refusal of an existing output, --force."""
    d = str(tmp_path)
    W, L = 96, 500
    img = ref.image(W, L, 1, 5)
    img.tofile(os.path.join(d, "P.RRC.RAW"))
    a, b = 400.0, 0.9
    open(os.path.join(d, "n.csv"), "w").write("# oip noise image=P.RRC.RAW\n1,0,15,100,2.5,3.2\n" + _band_line(1, a, b))
    thr = ref.thresholds(a, b, 2.0)[None, :]
    want = ref.sigma_filter_parts(img, thr, 2, None, 1)
    base = ["P.RRC.RAW", "--width", str(W), "--noise", "n.csv"]
    r = _run("denoise", base, d, OIP_DENOISE_BLOCK_LINES="64")
    assert r.returncode == 0, r.stdout + r.stderr
    out = os.path.join(d, "P.RRC.DNS.RAW")
    assert np.array_equal(np.fromfile(out, np.uint16).reshape(L, W), want["out"])
    assert not np.array_equal(want["out"], img) and (want["out"][img == 0] == 0).all()
    assert _counters(r.stdout) == want["stats"] and min(want["stats"]) > 0
    assert _thresholds_logged(r.stdout) == [[int(thr[0, l]) for l in (0, 64, 128, 255)]]
    # blocks of 7 lines and one block give the same bytes and counters
    for extra, env in ((["-o", "seven.RAW"], dict(OIP_DENOISE_BLOCK_LINES="7")), (["-o", "one.RAW"], {})):
        r = _run("denoise", base + extra, d, **env)
        assert r.returncode == 0, r.stdout + r.stderr
        assert open(os.path.join(d, extra[1]), "rb").read() == open(out, "rb").read() and _counters(r.stdout) == want["stats"]
    # an existing output: refused, then replaced with --force (another radius, K, min-members and valid-min: another result)
    other = ["--radius", "3", "--k-sigma", "1.5", "--min-members", "3", "--valid-min", "0"]
    r = _run("denoise", base + ["-o", "one.RAW"] + other, d)
    assert r.returncode == 2 and "--force" in r.stdout
    assert open(os.path.join(d, "one.RAW"), "rb").read() == want["out"].tobytes()
    with open(os.path.join(d, "one.RAW"), "ab") as f:
        f.write(b"longer than the product")
    r = _run("denoise", base + ["-o", "one.RAW", "--force"] + other, d, OIP_DENOISE_BLOCK_LINES="64")
    assert r.returncode == 0, r.stdout + r.stderr
    want3 = ref.sigma_filter_parts(img, ref.thresholds(a, b, 1.5)[None, :], 3, 3, 0)
    assert open(os.path.join(d, "one.RAW"), "rb").read() == want3["out"].tobytes() and not np.array_equal(want3["out"], want["out"])
    assert _counters(r.stdout) == want3["stats"]


@pytest.mark.parametrize("compress", ["none", "lzw"])
def test_four_sample_tiff_and_the_band_count(tmp_path, compress):
    d = str(tmp_path)
    w, rows = 131, 100
    img = ref.image(w, rows, 4, 9)
    write_tiff_u16(os.path.join(d, "A.TIFF"), img.reshape(rows, w, 4), lzw=compress == "lzw", predictor=2 if compress == "lzw" else 1,
                   rows_per_strip=16 if compress == "lzw" else None)
    models = [(400.0, 0.9), (100.0, 0.3), (0.0, 2.0), (2500.0, 0.0)]
    open(os.path.join(d, "four.csv"), "w").write("".join(_band_line(k + 1, a, b) for k, (a, b) in enumerate(models)))
    open(os.path.join(d, "one.csv"), "w").write(_band_line(1, 400.0, 0.9))
    thr = np.stack([ref.thresholds(a, b, 2.5) for a, b in models])
    r = _run("denoise", ["A.TIFF", "--noise", "four.csv", "--k-sigma", "2.5", "--radius", "3", "--tiff-compress", compress], d)
    assert r.returncode == 0, r.stdout + r.stderr
    out = os.path.join(d, "A.DNS.TIFF")
    got = read_tiff_u16(out)[0]
    want = ref.sigma_filter_parts(img, thr, 3, None, 1, 4)
    assert got.shape == (rows, w, 4) and np.array_equal(got.reshape(rows, -1), want["out"]) and _counters(r.stdout) == want["stats"]
    assert _thresholds_logged(r.stdout) == [[int(thr[c, l]) for l in (0, 64, 128, 255)] for c in range(4)]
    assert read_tags(out)[259][0] == (5 if compress == "lzw" else 1)   # Compression
    # a one-band report on the four-sample file: refused before a pixel is filtered, nothing written
    before = sorted(os.listdir(d))
    r = _run("denoise", ["A.TIFF", "--noise", "one.csv", "-o", "B.TIFF"], d)
    assert r.returncode == 2 and "holds 1 band, the image has 4 samples per pixel" in r.stdout, r.stdout + r.stderr
    assert "counters:" not in r.stdout and sorted(os.listdir(d)) == before
    assert np.array_equal(read_tiff_u16(os.path.join(d, "A.TIFF"))[0].reshape(rows, -1), img)


def test_one_sample_tiff_through_sigma(tmp_path):
    d = str(tmp_path)
    w, rows = 200, 77
    img = ref.image(w, rows, 1, 13)
    write_tiff_u16(os.path.join(d, "S.TIFF"), img)
    r = _run("denoise", ["S.TIFF", "--sigma", "37.3", "--radius", "1"], d)
    assert r.returncode == 0, r.stdout + r.stderr
    thr = np.full((1, 256), 75, np.uint16)                             # ceil(2 * 37.3)
    got = read_tiff_u16(os.path.join(d, "S.DNS.TIFF"))[0].reshape(rows, w)
    want = ref.sigma_filter_parts(img, thr, 1, None, 1)
    assert np.array_equal(got, want["out"]) and _counters(r.stdout) == want["stats"]
    assert _thresholds_logged(r.stdout) == [[75, 75, 75, 75]]
    # the same on the RAW strip, and a sigma beyond the range saturates the table: every sample with data is a member
    img.tofile(os.path.join(d, "S.RAW"))
    r = _run("denoise", ["S.RAW", "--width", str(w), "--sigma", "37.3", "--radius", "1"], d)
    assert r.returncode == 0 and open(os.path.join(d, "S.DNS.RAW"), "rb").read() == want["out"].tobytes(), r.stdout + r.stderr
    r = _run("denoise", ["S.RAW", "--width", str(w), "--sigma", "1e9", "-o", "all.RAW"], d)
    assert r.returncode == 0 and _thresholds_logged(r.stdout) == [[65535] * 4], r.stdout + r.stderr
    assert open(os.path.join(d, "all.RAW"), "rb").read() == ref.sigma_filter(img, np.full((1, 256), 65535, np.uint16), 2).tobytes()


def test_noise_denoise_noise(tmp_path):
    """the 1024 x 512 scene of the noise tool's recovery test (flat steps, a textured third; sigma^2 = 4 + 0.01 level):
    `oip noise`, `oip denoise --noise` with its report, `oip noise` again.  The second report's sigma_ref is below the first's
    by at least the r = 2 bar of the flat-field test; the product is the restatement's for the tables of the first report."""
    d = str(tmp_path)
    W, L = 1024, 512
    a0, b0 = _noise_ref.RECOVERY_MODELS[0]
    img = _noise_ref.scene(a0, b0, 100)
    img.tofile(os.path.join(d, "P.RAW"))
    r = _run("noise", ["P.RAW", "--width", str(W), "--min-blocks", "50"], d)
    assert r.returncode == 0, r.stdout + r.stderr
    first = _noise_ref.parse_report(os.path.join(d, "P.NOISE.CSV"))[1][1]
    r = _run("denoise", ["P.RAW", "--width", str(W), "--noise", "P.NOISE.CSV"], d, OIP_DENOISE_BLOCK_LINES="200")
    assert r.returncode == 0, r.stdout + r.stderr
    thr = ref.thresholds(first["a"], first["b"], 2.0)[None, :]
    want = ref.sigma_filter_parts(img, thr, 2, None, 1)
    assert open(os.path.join(d, "P.DNS.RAW"), "rb").read() == want["out"].tobytes() and _counters(r.stdout) == want["stats"]
    r = _run("noise", ["P.DNS.RAW", "--width", str(W), "--min-blocks", "50"], d)
    assert r.returncode == 0, r.stdout + r.stderr
    second = _noise_ref.parse_report(os.path.join(d, "P.DNS.NOISE.CSV"))[1][1]
    print("\nsigma_ref %.3f -> %.3f: ratio %.3f (bar %.3f)" % (first["sigma_ref"], second["sigma_ref"], second["sigma_ref"] / first["sigma_ref"], ref.FLAT_BARS[2]))
    assert second["sigma_ref"] <= ref.FLAT_BARS[2] * first["sigma_ref"]
