"""GPU: `oip rrc-calib` end to end -- the files it writes are the fit of numpy's totals bit for bit, and applied with the
existing RRC kernels they bring every column's mean to its group's reference."""
import os
import subprocess

import numpy as np
import pytest

from _colstats_ref import totals

pytestmark = pytest.mark.gpu
OIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "opticalimageprocessor_amd", "lib", "oip")
MSB = ["--rrc-msb%d" % (b + 1) for b in range(4)]


def _run(args, cwd):
    env = dict(os.environ, LOGFILE=os.path.join(cwd, "oip.log"))
    return subprocess.run([OIP, "rrc-calib"] + args, cwd=cwd, env=env, capture_output=True, text=True)


def _column_means(img):
    return img.astype(np.uint64).sum(0).astype(np.float64) / img.shape[0]


def _check_corrected(raw, corrected, kb, mu_ref):
    """InplaceRRC truncates a positive k*v + b toward zero, lowering each pixel by an amount in [0, 1); moment matching puts
    the untruncated column mean at mu_ref: the corrected mean lies in (mu_ref - 1, mu_ref] (1e-6 for the fp64 roundings of
    the mean itself).  Nothing clips or wraps: checked on each column's extreme samples."""
    k, b = kb[:, 0], kb[:, 1]
    lo, hi = k * raw.min(0).astype(np.float64) + b, k * raw.max(0).astype(np.float64) + b
    print("k*v + b over each column's extreme samples: min %.3f max %.3f" % (lo.min(), hi.max()))
    assert (lo > 0).all() and (hi < 65535).all()
    mean = _column_means(corrected)
    print("corrected column mean - mu_ref: min %.6f max %.6f" % ((mean - mu_ref).min(), (mean - mu_ref).max()))
    assert (mean > mu_ref - 1).all() and (mean <= mu_ref + 1e-6).all()


def test_calibrate_then_correct_closes_the_loop(ctx, tmp_path):
    """Strip length.  The synthetic counts are clamped to [64, 4095], so most PAN columns hold a sample of 64, and the
    no-wrap precondition needs k * 64 + b > 0, i.e. b > -58 for k >= 0.9.  b = mu_ref - k * mu_x moves by 1830 DN times the
    relative error of the column's sigma estimate, so that error has to stay under 3.2 %.  The texture (Gaussian blur,
    sigma 1.5 lines) decorrelates over ~5.3 lines: L lines are ~L / 5.3 independent samples and the estimate's relative
    standard deviation is sqrt(5.3 / (2 L)) -- 2 % at 6400 lines (columns fail), 0.64 % at 64000 (3.2 % is 5 sigma).
    Moment matching is a long-strip method; the test uses a long strip."""
    import torch
    import opticalimageprocessor_amd as oip
    from opticalimageprocessor_amd import synth
    W, Lp = 1280, 64000
    bw, Lm = W // 4, Lp // 4
    d = str(tmp_path)
    kb_true = synth.lut(W)
    kb4_true = np.concatenate([synth.lut(bw, 10 + b) for b in range(4)], 0)
    raw_pan = synth.pan_strip(64, Lp, W, kb_true, device="cuda")
    raw_mss = synth.mss_strip(16, Lm, W, kb4_true, device="cuda")
    pan, mss = raw_pan.cpu().numpy(), raw_mss.cpu().numpy()
    pan.tofile(os.path.join(d, "P.RAW")); mss.tofile(os.path.join(d, "M.RAW"))
    # precondition: there is something to calibrate
    for img in [pan] + [mss[:, b * bw:(b + 1) * bw] for b in range(4)]:
        m = _column_means(img)
        assert m.max() - m.min() > 1.0
    args = ["--width", str(W), "--pan", "P.RAW", "--rrc-pan", "pan.csv", "--mss", "M.RAW"]
    for b in range(4):
        args += [MSB[b], "msb%d.csv" % (b + 1)]
    r = _run(args, d)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PAN: %d lines, %d usable / 0 dead columns" % (Lp, W) in r.stdout
    assert "MSS band 4: %d lines, %d usable / 0 dead columns" % (Lm, bw) in r.stdout and "MBps" in r.stdout

    # the files are the fit of numpy's totals, bit for bit
    kb = oip.load_rrc_param_file(os.path.join(d, "pan.csv"), W)
    want, dead, ref = oip.rrc_fit_columns(totals(pan), 1, "moments", 0)
    assert np.array_equal(kb.view(np.uint64), want.view(np.uint64)) and dead[0] == 0
    kb4 = np.concatenate([oip.load_rrc_param_file(os.path.join(d, "msb%d.csv" % (b + 1)), bw) for b in range(4)], 0)
    want4, dead4, ref4 = oip.rrc_fit_columns(totals(mss), 4, "moments", 0)
    assert np.array_equal(kb4.view(np.uint64), want4.view(np.uint64)) and not dead4.any()

    # applied by the existing kernels
    out = torch.empty_like(raw_pan)
    ctx.rrc_u16(raw_pan, out, W, Lp, ctx.upload_kb(kb))
    planes = torch.zeros(4, Lm, bw, dtype=torch.uint16, device="cuda")
    ctx.mss_split_rrc_u16(raw_mss, planes, Lm * bw, W, Lm, ctx.upload_kb(kb4))
    ctx.sync()
    _check_corrected(pan, out.cpu().numpy(), kb, ref[0, 0])
    for b in range(4):
        _check_corrected(mss[:, b * bw:(b + 1) * bw], planes[b].cpu().numpy(), kb4[b * bw:(b + 1) * bw], ref4[b, 0])


def test_force_and_line_range(tmp_path):
    import opticalimageprocessor_amd as oip
    W, L = 1001, 5000                                             # not a multiple of 8: the column-per-lane kernel behind the CLI
    d = str(tmp_path)
    rng = np.random.default_rng(41)
    img = np.clip(np.rint(rng.integers(200, 3900, (L, W)) * rng.uniform(0.9, 1.1, W) + rng.uniform(-8, 8, W)), 0, 65535).astype(np.uint16)
    img.tofile(os.path.join(d, "P.RAW"))
    base = ["--width", str(W), "--pan", "P.RAW", "--rrc-pan", "pan.csv"]
    assert _run(base, d).returncode == 0
    first = open(os.path.join(d, "pan.csv"), "rb").read()
    r = _run(base + ["--mode", "gain"], d)                         # would write other numbers
    assert r.returncode == 2 and "pan.csv" in r.stdout
    assert open(os.path.join(d, "pan.csv"), "rb").read() == first
    assert _run(base + ["--force"], d).returncode == 0
    assert open(os.path.join(d, "pan.csv"), "rb").read() == first
    # a sub-range of the lines, a valid range and a minimum count, in gain mode
    img[1000:4000, 7] = 0                                         # a dead detector inside the range
    img.tofile(os.path.join(d, "P.RAW"))
    r = _run(["--width", str(W), "--pan", "P.RAW", "--rrc-pan", "sub.csv", "--line-offset", "1000", "--lines", "3000", "--mode", "gain",
              "--valid-min", "1", "--valid-max", "4095", "--min-count", "100"], d)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PAN: 3000 lines, %d usable / 1 dead columns" % (W - 1) in r.stdout
    want, dead, _ = oip.rrc_fit_columns(totals(img[1000:4000], 1, 4095), 1, "gain", 100)
    got = oip.load_rrc_param_file(os.path.join(d, "sub.csv"), W)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)) and dead[0] == 1 and tuple(got[7]) == (1.0, 0.0)


def test_strip_larger_than_the_device_blocks(tmp_path):
    """the strip is never resident: 13000 lines of 8192 px are four line blocks through the two alternating device
    buffers (the third and fourth refill a buffer a queued kernel has read)"""
    import torch
    import opticalimageprocessor_amd as oip
    W, L = 8192, 13000
    d = str(tmp_path)
    g = torch.Generator(device="cuda")
    g.manual_seed(77)
    img = torch.randint(64, 4096, (L, W), device="cuda", generator=g, dtype=torch.int32).to(torch.int16).view(torch.uint16).cpu().numpy()
    img.tofile(os.path.join(d, "P.RAW"))
    r = _run(["--width", str(W), "--pan", "P.RAW", "--rrc-pan", "pan.csv"], d)
    assert r.returncode == 0, r.stdout + r.stderr
    want, _, _ = oip.rrc_fit_columns(totals(img), 1, "moments", 0)
    got = oip.load_rrc_param_file(os.path.join(d, "pan.csv"), W)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
