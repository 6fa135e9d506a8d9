"""GPU: `oip quicklook` end to end -- the browse image it writes is the numpy restatement (_quicklook_ref.py) of the file's
contents, pixel for pixel, and the limits it logs are the restatement's."""
import os
import re
import subprocess

import numpy as np
import pytest

import _quicklook_ref as ref
from _tiff import write_tiff_u16

pytestmark = pytest.mark.gpu
OIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "opticalimageprocessor_amd", "lib", "oip")


def _run(args, cwd):
    env = dict(os.environ, LOGFILE=os.path.join(cwd, "oip.log"))
    return subprocess.run([OIP, "quicklook"] + args, cwd=cwd, env=env, capture_output=True, text=True)


def _read(path):
    from PIL import Image
    with Image.open(path) as im:
        return im.mode, im.size, np.asarray(im).copy()


def _logged(stdout):
    """[(band, lines, N, lo, hi)] of the log's per-band lines, in order"""
    return [tuple(int(v) for v in m) for m in re.findall(r"band (\d+): (\d+) lines, (\d+) valid samples, stretch (\d+)\.\.(\d+)", stdout)]


def test_pan_raw_one_band(tmp_path):
    from opticalimageprocessor_amd import synth
    W, L = 1280, 3000
    d = str(tmp_path)
    pan = synth.pan_strip(64, L, W, synth.lut(W), device="cuda").cpu().numpy()
    pan.tofile(os.path.join(d, "P.RAW"))
    r = _run(["P.RAW", "--width", str(W), "--factor", "16"], d)
    assert r.returncode == 0, r.stdout + r.stderr
    mode, size, got = _read(os.path.join(d, "P.QL.TIFF"))
    assert mode == "L" and size == (80, 188)
    want, lim = ref.quicklook([ref.decimate(pan, 16)])
    assert np.array_equal(got, want)
    lo, hi, n = lim[0]
    assert _logged(r.stdout) == [(1, L, n, lo, hi)] and "MBps" in r.stdout
    assert 0 < lo < hi and got.min() == 0 and got.max() == 255     # precondition: there is a contrast to stretch
    # the same file again is refused, --force replaces it with the same bytes
    first = open(os.path.join(d, "P.QL.TIFF"), "rb").read()
    assert _run(["P.RAW", "--width", str(W)], d).returncode == 2
    assert _run(["P.RAW", "--width", str(W), "--force"], d).returncode == 0
    assert open(os.path.join(d, "P.QL.TIFF"), "rb").read() == first


@pytest.mark.parametrize("W", [1280, 1000])
def test_bil_bands_in_the_order_given(tmp_path, W):
    """MSS line layout, --bands 3,2,1: RGB, each band stretched with its own limits.  W = 1280: band windows start on 16-byte
    boundaries; W = 1000: bands 2 to 4 start at bytes 500, 1000 and 1500, the kernel for misaligned windows behind the CLI"""
    from opticalimageprocessor_amd import synth
    Lm, bw, F = 1501, W // 4, 8
    d = str(tmp_path)
    if W == 1280:
        kb4 = np.concatenate([synth.lut(bw, 10 + b) for b in range(4)], 0)
        mss = synth.mss_strip(16, Lm, W, kb4, device="cuda").cpu().numpy()
    else:
        mss = np.concatenate([np.random.default_rng(50 + b).integers(100 * (b + 1), 900 * (b + 1), (Lm, bw), dtype=np.uint16) for b in range(4)], 1)
    mss.tofile(os.path.join(d, "M.RAW"))
    r = _run(["M.RAW", "--width", str(W), "--bil", "--bands", "3,2,1", "--factor", str(F), "-o", "browse.TIFF"], d)
    assert r.returncode == 0, r.stdout + r.stderr
    mode, size, got = _read(os.path.join(d, "browse.TIFF"))
    assert mode == "RGB" and size == (-(-bw // F), -(-Lm // F))
    planes = [ref.decimate(mss[:, b * bw:(b + 1) * bw], F) for b in (2, 1, 0)]
    want, lim = ref.quicklook(planes)
    assert np.array_equal(got, want)
    assert _logged(r.stdout) == [(b, Lm, n, lo, hi) for b, (lo, hi, n) in zip((3, 2, 1), lim)]
    assert len({(lo, hi) for lo, hi, _ in lim}) == 3               # precondition: the bands' limits differ


def test_four_sample_lzw_tiff(tmp_path):
    """a 4-sample LZW product (predictor 2, several strips), default bands 1,2,3; options that are not the defaults"""
    rows, w, F = 121, 83, 4                                       # (the test's pure-Python LZW writer sets the size)
    d = str(tmp_path)
    img = np.random.default_rng(60).integers(0, 3000, (rows, w, 4), dtype=np.uint16)
    img[:, :, 1] += 500
    img[:18] = 0
    write_tiff_u16(os.path.join(d, "A.TIFF"), img, lzw=True, predictor=2, rows_per_strip=16)
    r = _run(["A.TIFF", "--factor", str(F), "--clip-low", "5", "--clip-high", "90", "--valid-min", "10", "--valid-max", "2900"], d)
    assert r.returncode == 0, r.stdout + r.stderr
    mode, size, got = _read(os.path.join(d, "A.QL.TIFF"))
    assert mode == "RGB" and size == (-(-w // F), -(-rows // F))
    want, lim = ref.quicklook(list(ref.decimate(img, F)[:3]), valid_min=10, valid_max=2900, p_lo=5.0, p_hi=90.0)
    assert np.array_equal(got, want)
    assert _logged(r.stdout) == [(b + 1, rows, n, lo, hi) for b, (lo, hi, n) in enumerate(lim)]


def test_one_sample_tiff_line_range(tmp_path):
    rows, w, F = 130, 77, 2
    d = str(tmp_path)
    img = np.random.default_rng(61).integers(0, 4096, (rows, w), dtype=np.uint16)
    write_tiff_u16(os.path.join(d, "S.tiff"), img)
    r = _run(["S.tiff", "--factor", str(F), "--line-offset", "10", "--lines", "101", "--bands", "1"], d)
    assert r.returncode == 0, r.stdout + r.stderr
    mode, size, got = _read(os.path.join(d, "S.QL.TIFF"))
    want, lim = ref.quicklook([ref.decimate(img[10:111], F)])
    assert mode == "L" and np.array_equal(got, want)
    assert _logged(r.stdout) == [(1, 101, lim[0][2], lim[0][0], lim[0][1])]
    assert _run(["S.tiff", "--bands", "1,2,3", "--force"], d).returncode == 254      # the image has one band


def test_strip_larger_than_the_device_blocks(tmp_path):
    """the strip is never resident: 13000 lines of 8192 px are four line blocks through the two alternating device buffers
    (the third and fourth refill a buffer a queued kernel has read); 13000 is no multiple of the factor"""
    import torch
    W, L, F = 8192, 13000, 16
    d = str(tmp_path)
    g = torch.Generator(device="cuda")
    g.manual_seed(78)
    img = torch.randint(64, 4096, (L, W), device="cuda", generator=g, dtype=torch.int32).to(torch.int16).view(torch.uint16).cpu().numpy()
    img[:, 4096:] //= 3                                            # something to stretch after 256 samples are averaged
    img.tofile(os.path.join(d, "P.RAW"))
    r = _run(["P.RAW", "--width", str(W)], d)
    assert r.returncode == 0, r.stdout + r.stderr
    mode, size, got = _read(os.path.join(d, "P.QL.TIFF"))
    want, lim = ref.quicklook([ref.decimate(img, F)])
    assert size == (W // F, -(-L // F)) and np.array_equal(got, want)
    assert _logged(r.stdout) == [(1, L, lim[0][2], lim[0][0], lim[0][1])]


def test_zero_border_stays_out_of_the_limits(tmp_path):
    """300 leading lines of zeros, as prestitch and the aligner leave them: with the default --valid-min 1 the limits are
    those of the image proper, and the border maps to 0"""
    from opticalimageprocessor_amd import synth
    W, L, F = 1280, 3000, 16
    d = str(tmp_path)
    pan = synth.pan_strip(64, L, W, synth.lut(W), device="cuda").cpu().numpy()
    pan[:300] = 0
    pan.tofile(os.path.join(d, "P.RAW"))
    r = _run(["P.RAW", "--width", str(W)], d)
    assert r.returncode == 0, r.stdout + r.stderr
    _, _, got = _read(os.path.join(d, "P.QL.TIFF"))
    dec = ref.decimate(pan, F)
    want, lim = ref.quicklook([dec])
    lo, hi, n = lim[0]
    assert np.array_equal(got, want) and _logged(r.stdout) == [(1, L, n, lo, hi)]
    assert n == np.count_nonzero(dec) and n < dec.size and lo > 0
    assert (lo, hi) == ref.stretch_limits(dec[dec > 0], 0, 65535)[:2]          # the limits of the non-zero samples alone
    assert not got[:300 // F].any()
