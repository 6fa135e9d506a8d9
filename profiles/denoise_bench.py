"""Times oip_sigma_filter_u16 at radius 1, 2 and 3 against its yardstick, oip_convolve_u16 at 3 x 3, 5 x 5 and 7 x 7 with
valid_min 1, on the same HBM-resident raster in one process, and prints one JSON line (to be kept as
profiles/denoise_kernel.json and quoted in DESIGN.md 4.1h).

    python profiles/denoise_bench.py [--reps 10] [--lines 100000] [--small]

A PAN strip of 30000 x --lines x 1 (100000 lines: 6 GB in, 6 GB out).  Device events around each call on the one stream torch and
the library share; the calls alternate inside the timed loop, medians are reported with the extremes.  Every call reads the
raster once and writes it once (2 B in, 2 B out per sample); the window re-reads come from LDS.  Data: a 12-bit scene of flat
steps with Gaussian noise of sigma^2 = 4 + 0.01 level and no no-data, filtered with the tables oip_denoise_thresholds gives for
that model at K = 2, min_members 2 r + 1; the sigma filter is timed without counters, and at radius 2 once more with them.
--small: a tenth of the lines (a rehearsal, not a measurement)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import opticalimageprocessor_amd as oip  # noqa: E402

HBM_PEAK = 8.0e12
A, B = 4.0, 0.01


def raster(lines, w, seed):
    """flat steps 52 samples wide from 300 to 3800 DN plus the model's noise, made on the device in blocks of lines"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    x = torch.arange(w, device="cuda", dtype=torch.float32)
    s = 300.0 + 3500.0 * torch.floor(x / 52) * 52 / (w - 1)
    sd = torch.sqrt(A + B * s)
    out = torch.empty(lines, w, dtype=torch.uint16, device="cuda")
    for r in range(0, lines, 4096):
        m = min(4096, lines - r)
        v = s[None, :] + torch.randn(m, w, device="cuda", generator=g) * sd[None, :]
        out.view(torch.int16)[r:r + m] = v.round_().clamp_(1, 32767).to(torch.int16)
    return out


def taps(k):
    """a k x k sharpening kernel of DC gain 1: separable, negative lobes falling off from the centre (profiles/mtfc_bench.py's)"""
    r = k // 2
    f = np.array([-0.5 ** abs(i) for i in range(-r, r + 1)])
    f[r] = 0.0
    f *= 0.29 / -f.sum()
    f[r] = 1.29
    return oip.mtfc_quantise(np.outer(f, f))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def summary(v, nbytes):
    s = statistics.median(v)
    return {"seconds_median": s, "seconds_min": min(v), "seconds_max": max(v), "GBps": nbytes / s / 1e9, "fraction_of_8TBps_peak": nbytes / s / HBM_PEAK}


def measure(ctx, W, L, reps):
    src = raster(L, W, 1)
    out = torch.empty_like(src)
    thr = torch.from_numpy(oip.denoise_thresholds(A, B, 2.0)).cuda()
    stats = torch.zeros(4, dtype=torch.int64, device="cuda")
    runs = {}
    for r in (1, 2, 3):
        k = 2 * r + 1
        runs["convolve_%dx%d" % (k, k)] = lambda t=taps(k): ctx.convolve_u16(src, out, W, L, 1, t, 1)
        runs["sigma_r%d" % r] = lambda r=r: ctx.sigma_filter_u16(src, out, W, L, 1, r, thr, None, 1, None)
    runs["sigma_r2_counters"] = lambda: ctx.sigma_filter_u16(src, out, W, L, 1, 2, thr, None, 1, stats)
    t = {k: [] for k in runs}
    for _ in range(2):
        for fn in runs.values():
            fn()
    ctx.sync()
    stats.zero_()
    for _ in range(reps):
        for k, fn in runs.items():
            t[k].append(timed(fn))
    nbytes = 2 * src.numel() * 2
    res = {"W": W, "lines": L, "spp": 1, "reps": reps, "noise_model": {"a": A, "b": B, "k_sigma": 2.0}}
    for k in runs:
        res[k] = summary(t[k], nbytes)
    for r in (1, 2, 3):
        k = 2 * r + 1
        res["sigma_r%d_over_convolve_%dx%d_time" % (r, k, k)] = res["sigma_r%d" % r]["seconds_median"] / res["convolve_%dx%d" % (k, k)]["seconds_median"]
    res["sigma_r2_counters_over_sigma_r2_time"] = res["sigma_r2_counters"]["seconds_median"] / res["sigma_r2"]["seconds_median"]
    # what the filter did, from the counters of the timed radius-2 runs (reps calls over the same raster)
    s = [int(v) // reps for v in stats.cpu().tolist()]
    res["sigma_r2_per_call"] = {"valid": s[0], "left_alone": s[1], "mean_members": s[2] / max(1, s[0] - s[1]), "changed": s[3]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--lines", type=int, default=100000)
    ap.add_argument("--small", action="store_true")
    a = ap.parse_args()
    ctx = oip.Context(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream)
    lines = a.lines // (10 if a.small else 1)
    res = {"tool": "denoise_bench", "arch": torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]}
    res["pan_30000x%dx1" % lines] = measure(ctx, 30000, lines, a.reps)
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
