"""Times oip_halve_u16 against its yardstick, oip_decimate_box_u16 at factor 2 and 1 sample per pixel (an existing kernel
with the same bytes in and out), on HBM-resident rasters in one process, and prints one JSON line (to be kept as
profiles/overviews_kernel.json and quoted in DESIGN.md 4.1f).

    python profiles/overviews_bench.py [--reps 20] [--small]

Two geometries: a PAN strip of 12288 x 60000 x 1 and an image of 6144 x 60000 x 4.  Device events around each call on the one
stream torch and the library share; the calls alternate inside the timed loop, medians are reported with the extremes.  Every
call reads the raster once and writes a quarter of it (2 B in, 0.5 B out: 2.5 B per source sample).  Data: 12-bit sensor
values without no-data, uniform in [64, 4096).  The runs:
    decimate_f2       the yardstick (1 sample per pixel only: at 4 it de-interleaves into planes)
    halve_vm1         valid_min 1: every block takes the form that counts its valid samples
    halve_vm0         valid_min 0: full blocks divide by a shift
    halve_vm1_nodata  halve_vm1 on a copy with 3 % zeros
--small: a tenth of the lines (a rehearsal, not a measurement)."""
import argparse
import json
import os
import statistics
import sys

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
    ow, oh = (W + 1) // 2, (L + 1) // 2
    out = torch.empty(oh, ow * spp, dtype=torch.uint16, device="cuda")
    runs = {}
    if spp == 1:
        runs["decimate_f2"] = lambda: ctx.decimate_box_u16(src, ws, W, L, 1, 2, out, ow)
    runs["halve_vm1"] = lambda: ctx.halve_u16(src, ws, W, L, spp, 1, out, ow * spp)
    runs["halve_vm0"] = lambda: ctx.halve_u16(src, ws, W, L, spp, 0, out, ow * spp)
    runs["halve_vm1_nodata"] = lambda: ctx.halve_u16(holes, ws, W, L, spp, 1, out, ow * spp)
    t = {k: [] for k in runs}
    for _ in range(3):
        for fn in runs.values():
            fn()
    ctx.sync()
    for _ in range(reps):
        for k, fn in runs.items():
            t[k].append(timed(fn))
    nbytes = src.numel() * 2.5
    res = {"W": W, "lines": L, "spp": spp, "reps": reps, "bytes_per_source_sample": 2.5}
    for k in runs:
        res[k] = summary(t[k], nbytes)
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
    res = {"tool": "overviews_bench", "arch": torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]}
    pan = res["pan_12288x60000x1"] = measure(ctx, 12288, 60000 // div, 1, a.reps)
    torch.cuda.empty_cache()
    res["img_6144x60000x4"] = measure(ctx, 6144, 60000 // div, 4, a.reps)
    # the yardstick is the spp = 1 strip's, in the same run; its own run-to-run spread is what a ratio near 1 is read against
    base = pan["decimate_f2"]["seconds_median"]
    res["decimate_f2_spread"] = (pan["decimate_f2"]["seconds_max"] - pan["decimate_f2"]["seconds_min"]) / base
    for k in ("halve_vm1", "halve_vm0", "halve_vm1_nodata"):
        res["pan_" + k + "_over_decimate_f2_time"] = pan[k]["seconds_median"] / base
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
