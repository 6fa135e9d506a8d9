"""Times oip_convolve_u16 at 3 x 3, 5 x 5 and 9 x 9 against its yardstick, oip_rrc_u16 out of place on the same bytes, on
HBM-resident rasters in one process, and prints one JSON line (to be kept as profiles/mtfc_kernel.json and quoted in
DESIGN.md 4.1c).

    python profiles/mtfc_bench.py [--reps 20] [--small]

Two geometries: a PAN strip of 30000 x 100000 x 1 and an aligned-MSS product of 7500 x 25000 x 4 (1.5 GB: inside the
Infinity Cache's reach only in small part).  Device events around each call on the one stream torch and the library share;
the calls alternate inside the timed loop, medians are reported with the extremes.  Every call reads the raster once and
writes it once (2 B in, 2 B out per sample); the filter re-reads halo lines and columns from the caches.  Data: 12-bit
sensor values without no-data, plus one 3 x 3 run on a copy with 3 % zeros (every tile then takes the no-data form of the
loop).  --small: a tenth of the lines (a rehearsal, not a measurement)."""
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


def raster(lines, ws, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    out = torch.empty(lines, ws, dtype=torch.uint16, device="cuda")
    for r in range(0, lines, 8192):
        m = min(8192, lines - r)
        v = torch.randint(64, 4096, (m, ws), device="cuda", generator=g, dtype=torch.int32)
        out.view(torch.int16)[r:r + m] = v.to(torch.int16)
    return out


def taps(k):
    """a k x k sharpening kernel of DC gain 1 and sum |t| near 2.5 * 4096: separable, negative lobes falling off from the centre"""
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


def measure(ctx, W, L, spp, reps):
    ws = W * spp
    src = raster(L, ws, 1)
    holes = src.clone()
    for r in range(0, L, 8192):
        m = min(8192, L - r)
        holes.view(torch.int16)[r:r + m].masked_fill_(torch.rand(m, ws, device="cuda") < 0.03, 0)
    out = torch.empty_like(src)
    kb = ctx.upload_kb(np.tile([1.01, 3.0], ws))
    sets = {k: taps(k) for k in (3, 5, 9)}
    runs = {"rrc_u16": lambda: ctx.rrc_u16(src, out, ws, L, kb)}
    for k, t in sets.items():
        runs["convolve_%dx%d" % (k, k)] = lambda t=t: ctx.convolve_u16(src, out, W, L, spp, t, 1)
    runs["convolve_3x3_nodata"] = lambda: ctx.convolve_u16(holes, out, W, L, spp, sets[3], 1)
    t = {k: [] for k in runs}
    for _ in range(3):
        for fn in runs.values():
            fn()
    ctx.sync()
    for _ in range(reps):
        for k, fn in runs.items():
            t[k].append(timed(fn))
    nbytes = 2 * src.numel() * 2
    res = {"W": W, "lines": L, "spp": spp, "reps": reps, "sum_abs_taps": {str(k): int(np.abs(v).sum()) for k, v in sets.items()}}
    for k in runs:
        res[k] = summary(t[k], nbytes)
    base = res["rrc_u16"]["seconds_median"]
    for k in runs:
        if k != "rrc_u16":
            res[k + "_over_rrc_time"] = res[k]["seconds_median"] / base
    # run-to-run spread of the yardstick itself: what a ratio near 1 has to be read against
    res["rrc_u16_spread"] = (res["rrc_u16"]["seconds_max"] - res["rrc_u16"]["seconds_min"]) / base
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--small", action="store_true")
    a = ap.parse_args()
    ctx = oip.Context(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream)
    div = 10 if a.small else 1
    res = {"tool": "mtfc_bench", "arch": torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]}
    res["pan_30000x100000x1"] = measure(ctx, 30000, 100000 // div, 1, a.reps)
    torch.cuda.empty_cache()
    res["mss_7500x25000x4"] = measure(ctx, 7500, 25000 // div, 4, a.reps)
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
