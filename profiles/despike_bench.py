"""Times oip_despike_u16 against its yardstick, oip_convolve_u16 with 3 x 3 taps (the same bytes through the same tile
shape), on HBM-resident rasters in one process, and prints one JSON line (to be kept as profiles/despike_kernel.json and
quoted in DESIGN.md 4.1d).

    python profiles/despike_bench.py [--reps 20] [--small]

Two geometries: a PAN strip of 30000 x 100000 x 1 and a product of 7500 x 25000 x 4.  Device events around each call on the
one stream torch and the library share; the calls alternate inside the timed loop, medians are reported with the extremes.
Every call reads the raster once and writes it once (2 B in, 2 B out per sample).  Data: 12-bit sensor values without
no-data, uniform in [64, 4096).  The runs:
    convolve_3x3      the yardstick
    despike_quiet     threshold 4096: nothing is replaced (a clean strip), counts requested
    despike_busy      threshold 1000: a large share of the samples is replaced (reported) -- every column of every tile issues its atomic
    despike_nocount   threshold 1000 without counts
    despike_table20   despike_quiet with a table of 20 bad columns (1 sample per pixel only)
    despike_nodata    despike_quiet on a copy with 3 % zeros (every tile takes the no-data form)
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


def raster(lines, ws, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    out = torch.empty(lines, ws, dtype=torch.uint16, device="cuda")
    for r in range(0, lines, 8192):
        m = min(8192, lines - r)
        v = torch.randint(64, 4096, (m, ws), device="cuda", generator=g, dtype=torch.int32)
        out.view(torch.int16)[r:r + m] = v.to(torch.int16)
    return out


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
    cnt = torch.zeros(ws, dtype=torch.int64, device="cuda")
    taps = oip.mtfc_quantise(oip.mtfc_design3(0.5, 0.5, 2.0))
    runs = {
        "convolve_3x3": lambda: ctx.convolve_u16(src, out, W, L, spp, taps, 1),
        "despike_quiet": lambda: ctx.despike_u16(src, out, W, L, spp, 4096, 0, 1, 1, None, cnt),
        "despike_busy": lambda: ctx.despike_u16(src, out, W, L, spp, 1000, 0, 1, 1, None, cnt),
        "despike_nocount": lambda: ctx.despike_u16(src, out, W, L, spp, 1000, 0, 1, 1, None, None),
        "despike_nodata": lambda: ctx.despike_u16(holes, out, W, L, spp, 4096, 0, 1, 1, None, cnt),
    }
    if spp == 1:
        bad = sorted(set(int(c) for c in np.random.default_rng(20).choice(W, 20, replace=False)))
        tab = torch.from_numpy(oip.despike_column_table(bad, W, 1)[0]).cuda()
        runs["despike_table20"] = lambda: ctx.despike_u16(src, out, W, L, spp, 4096, 0, 1, 1, tab, cnt)
    t = {k: [] for k in runs}
    for _ in range(3):
        for fn in runs.values():
            fn()
    ctx.sync()
    cnt.zero_()
    runs["despike_busy"]()
    ctx.sync()
    replaced = int(cnt.sum().item())
    for _ in range(reps):
        for k, fn in runs.items():
            t[k].append(timed(fn))
    nbytes = 2 * src.numel() * 2
    res = {"W": W, "lines": L, "spp": spp, "reps": reps, "despike_busy_replaced_share": replaced / src.numel()}
    for k in runs:
        res[k] = summary(t[k], nbytes)
    base = res["convolve_3x3"]["seconds_median"]
    for k in runs:
        if k != "convolve_3x3":
            res[k + "_over_convolve_3x3_time"] = res[k]["seconds_median"] / base
    # run-to-run spread of the yardstick itself: what a ratio near 1 has to be read against
    res["convolve_3x3_spread"] = (res["convolve_3x3"]["seconds_max"] - res["convolve_3x3"]["seconds_min"]) / base
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
    res = {"tool": "despike_bench", "arch": torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]}
    res["pan_30000x100000x1"] = measure(ctx, 30000, 100000 // div, 1, a.reps)
    torch.cuda.empty_cache()
    res["mss_7500x25000x4"] = measure(ctx, 7500, 25000 // div, 4, a.reps)
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
