"""Times oip_warp_grid_bicubic_u16, the kernel of `oip regfix`, beside its yardstick remap_shift8_kernel (the constant-shift
bicubic of prestitch: the same 16-tap sum with the weights shared by the 8 pixels of a lane) on the same HBM-resident raster in
one process, and prints one JSON line (kept as profiles/regfix_kernel.json and quoted in DESIGN.md 4.2a).

    python profiles/regfix_bench.py [--reps 10] [--small] [--only pan|mss] [--out FILE]

Two geometries: a PAN strip of 30000 x 100000 x 1 and a product of 7500 x 25000 x 4 (the yardstick, which knows one sample per
pixel, takes the product's bytes as 30000 x 25000 x 1).  The field: nodes every 64 pixels, dx = 1.2 sin(2 pi y / 20000) + 0.3,
dy = 0.6 cos(2 pi x / 7000) - 0.5 px -- smooth, as a report of regcheck is.  Per call: device events around it on the one stream
torch and the library share (for the warp that includes the copy of the node lines to the device), and the library's own events
around the kernel alone (oip_profile_*).  The calls alternate inside the timed loop; medians are reported with the extremes.
Every call reads the raster once and writes it once: 2 B in, 2 B out per sample is what the rates count.
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
STEP = 64


def raster(lines, ws, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    out = torch.empty(lines, ws, dtype=torch.uint16, device="cuda")
    for r in range(0, lines, 8192):
        m = min(8192, lines - r)
        v = torch.randint(64, 4096, (m, ws), device="cuda", generator=g, dtype=torch.int32)
        out.view(torch.int16)[r:r + m] = v.to(torch.int16)
    return out


def field(W, L):
    nx, ny = (W - 1) // STEP + 2, (L - 1) // STEP + 2
    y, x = np.arange(ny)[:, None] * STEP, np.arange(nx)[None, :] * STEP
    NX = np.rint((1.2 * np.sin(2 * np.pi * y / 20000.0) + 0.3 + 0 * x) * 1024).astype(np.int32)
    NY = np.rint((0.6 * np.cos(2 * np.pi * x / 7000.0) - 0.5 + 0 * y) * 1024).astype(np.int32)
    return NX, NY


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
    src = raster(L, W * spp, 1)
    out = torch.empty_like(src)
    NX, NY = field(W, L)
    sec, guard = (30000, 32767) if L > 32767 else (max(300, L // 3),) * 2      # the reference's constants where the strip allows them
    runs = {
        "remap_shift8": lambda: ctx.remap_shift_bicubic_u16(src, out, W * spp, L, 1.53, -0.77, sec, guard),
        "warp_grid": lambda: ctx.warp_grid_bicubic_u16(src, out, W, L, spp, NX, NY, 0, 0, STEP, STEP),
    }
    if spp == 4:
        runs["warp_grid_band3"] = lambda: ctx.warp_grid_bicubic_u16(src, out, W, L, spp, NX, NY, 0, 0, STEP, STEP, 4)
    kernels = {"remap_shift8": "remap_shift8_kernel", "warp_grid": "warp_grid_kernel", "warp_grid_band3": "warp_grid_kernel"}
    for _ in range(2):
        for fn in runs.values():
            fn()
    ctx.sync()
    t = {k: [] for k in runs}
    tk = {k: [] for k in runs}
    ctx.profile_enable(True)
    for _ in range(reps):
        for k, fn in runs.items():
            ctx.profile_reset()
            t[k].append(timed(fn))
            ctx.sync()
            tk[k].append(ctx.profile()[kernels[k]][0] * 1e-3)
    ctx.profile_enable(False)
    nbytes = 2 * src.numel() * 2
    res = {"W": W, "lines": L, "spp": spp, "reps": reps, "step": STEP, "nodes": [int(NX.shape[1]), int(NX.shape[0])], "bytes_counted": nbytes}
    for k in runs:
        res[k] = {"call": summary(t[k], nbytes), "kernel": summary(tk[k], nbytes), "kernel_name": kernels[k]}
        res[k]["kernel"]["ns_per_pixel"] = res[k]["kernel"]["seconds_median"] * 1e9 / (W * L)
    base = res["remap_shift8"]["kernel"]["seconds_median"]
    for k in runs:
        if k != "remap_shift8":
            res[k + "_over_remap_shift8_kernel_time"] = res[k]["kernel"]["seconds_median"] / base
    res["remap_shift8_spread"] = (res["remap_shift8"]["kernel"]["seconds_max"] - res["remap_shift8"]["kernel"]["seconds_min"]) / base
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--only", choices=["pan", "mss"])
    ap.add_argument("--out")
    a = ap.parse_args()
    ctx = oip.Context(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream)
    div = 10 if a.small else 1
    res = {"tool": "regfix_bench", "arch": torch.cuda.get_device_properties(0).gcnArchName.split(":")[0], "small": a.small}
    if a.only != "mss":
        res["pan_30000x100000x1"] = measure(ctx, 30000, 100000 // div, 1, a.reps)
        torch.cuda.empty_cache()
    if a.only != "pan":
        res["mss_7500x25000x4"] = measure(ctx, 7500, 25000 // div, 4, a.reps)
    ctx.close()
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
