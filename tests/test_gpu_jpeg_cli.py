"""GPU: `oip quicklook --format jpeg` end to end -- the browse JPEG it writes is, byte for byte, the restatement's encoding
(tests/_jpeg_ref.py) of the restated browse image (tests/_quicklook_ref.py) of the file; Pillow opens it; without --format the tool
writes the TIFF it always wrote; and the refusals of the two new options."""
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

import _jpeg_ref as J
import _quicklook_ref as ref
from _tiff import write_tiff_u16

pytestmark = pytest.mark.gpu
OIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "opticalimageprocessor_amd", "lib", "oip")


def _run(args, cwd):
    env = dict(os.environ, LOGFILE=os.path.join(cwd, "oip.log"))
    return subprocess.run([OIP, "quicklook"] + args, cwd=cwd, env=env, capture_output=True, text=True)


def _assert_is(path, want, quality):
    with open(path, "rb") as f:
        data = f.read()
    assert data == J.encode(want, quality).file
    with Image.open(path) as im:
        im.load()
        assert im.mode == ("L" if want.ndim == 2 else "RGB") and im.size == (want.shape[1], want.shape[0])


@pytest.fixture(scope="module")
def pan():
    from opticalimageprocessor_amd import synth
    return synth.pan_strip(64, 3000, 1280, synth.lut(1280), device="cuda").cpu().numpy()


def test_pan_raw_as_jpeg(tmp_path, pan):
    d = str(tmp_path)
    pan.tofile(os.path.join(d, "P.RAW"))
    r = _run(["P.RAW", "--width", "1280", "--factor", "16", "--format", "jpeg"], d)
    assert r.returncode == 0, r.stdout + r.stderr
    want, _ = ref.quicklook([ref.decimate(pan, 16)])
    assert want.shape == (188, 80)
    _assert_is(os.path.join(d, "P.QL.JPG"), want, 90)
    assert "JPEG, quality 90" in r.stdout and not os.path.exists(os.path.join(d, "P.QL.TIFF"))
    # the same file again is refused, --force replaces it with the same bytes
    first = open(os.path.join(d, "P.QL.JPG"), "rb").read()
    assert _run(["P.RAW", "--width", "1280", "--format", "jpeg"], d).returncode == 2
    assert _run(["P.RAW", "--width", "1280", "--format", "jpeg", "--force"], d).returncode == 0
    assert open(os.path.join(d, "P.QL.JPG"), "rb").read() == first


def test_without_format_the_tiff_as_before(tmp_path, pan):
    d = str(tmp_path)
    pan.tofile(os.path.join(d, "P.RAW"))
    want, _ = ref.quicklook([ref.decimate(pan, 16)])
    for extra in ([], ["--format", "tiff", "--force"]):
        r = _run(["P.RAW", "--width", "1280", "--factor", "16"] + extra, d)
        assert r.returncode == 0 and "JPEG" not in r.stdout, r.stdout + r.stderr
        with Image.open(os.path.join(d, "P.QL.TIFF")) as im:
            assert im.format == "TIFF" and im.mode == "L" and np.array_equal(np.asarray(im), want)
        assert not os.path.exists(os.path.join(d, "P.QL.JPG"))


def test_bil_rgb_as_jpeg(tmp_path):
    W, Lm, F = 1000, 1501, 8
    bw = W // 4
    d = str(tmp_path)
    mss = np.concatenate([np.random.default_rng(50 + b).integers(100 * (b + 1), 900 * (b + 1), (Lm, bw), dtype=np.uint16) for b in range(4)], 1)
    mss.tofile(os.path.join(d, "M.RAW"))
    r = _run(["M.RAW", "--width", str(W), "--bil", "--bands", "3,2,1", "--factor", str(F), "--format", "jpeg"], d)
    assert r.returncode == 0, r.stdout + r.stderr
    want, _ = ref.quicklook([ref.decimate(mss[:, b * bw:(b + 1) * bw], F) for b in (2, 1, 0)])
    assert want.shape == (188, 32, 3)
    _assert_is(os.path.join(d, "M.QL.JPG"), want, 90)


def test_four_sample_tiff_quality_and_name(tmp_path):
    rows, w, F = 121, 83, 4
    d = str(tmp_path)
    img = np.random.default_rng(60).integers(0, 3000, (rows, w, 4), dtype=np.uint16)
    write_tiff_u16(os.path.join(d, "A.TIFF"), img, lzw=True, predictor=2, rows_per_strip=16)
    r = _run(["A.TIFF", "--factor", str(F), "--format", "jpeg", "--quality", "60", "-o", "browse.jpg"], d)
    assert r.returncode == 0 and "JPEG, quality 60" in r.stdout, r.stdout + r.stderr
    want, _ = ref.quicklook(list(ref.decimate(img, F)[:3]))
    _assert_is(os.path.join(d, "browse.jpg"), want, 60)


def test_refusals(tmp_path):
    d = str(tmp_path)
    np.zeros((64, 1280), np.uint16).tofile(os.path.join(d, "P.RAW"))
    base = ["P.RAW", "--width", "1280"]
    for args, code, text in ((["--format", "jpeg", "--quality", "0"], 105, "1 <= Q <= 100 expected"),
                             (["--format", "jpeg", "--quality", "101"], 105, "1 <= Q <= 100 expected"),
                             (["--format", "png"], 105, "tiff or jpeg expected"),
                             (["--quality", "80"], 107, "--quality requires --format jpeg")):
        r = _run(base + args, d)
        assert r.returncode == code and text in r.stdout + r.stderr, (args, r.returncode, r.stdout + r.stderr)
    assert not [f for f in os.listdir(d) if ".QL." in f]
    # a browse image higher than 65535: 131100 lines at --factor 2
    np.full((131100, 8), 700, np.uint16).tofile(os.path.join(d, "N.RAW"))
    r = _run(["N.RAW", "--width", "8", "--factor", "2", "--format", "jpeg"], d)
    assert r.returncode == 2 and "65535" in r.stdout + r.stderr and "--factor" in r.stdout + r.stderr, r.stdout + r.stderr
    assert not os.path.exists(os.path.join(d, "N.QL.JPG"))
