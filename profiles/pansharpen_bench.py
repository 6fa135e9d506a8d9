"""Times oip_pansharpen_sfim_u16, the kernel of `oip pansharpen`, on HBM-resident rasters and prints one JSON line (kept as
profiles/pansharpen_kernel.json and quoted in DESIGN.md 4.2b).

    python profiles/pansharpen_bench.py [--reps 10] [--small] [--only scene|wide] [--out FILE]

Two geometries: the scene the tool's products have, PAN 24376 x 100000 with MSS 6094 x 25000, and a wide one, PAN 30000 x 100000
with MSS 7500 x 25000.  The rasters are 12-bit noise, PAN a smoothed version of it so that the gains stay near 1.  Per call:
device events around it on the one stream torch and the library share, and the library's own events around the kernel alone
(oip_profile_*).  Beside it, in the same loop, a device-to-device copy of half the product onto the other half (the product's
bytes moved once: the copy ceiling of this process).  Medians are reported with the extremes.
Bytes counted per PAN pixel: 2 B of PAN in, 8 B of product out, and per MSS pixel 8 B of MSS and 2 B of low-resolution PAN in
(0.625 B per PAN pixel; the neighbours' re-reads are served by the caches and not counted): 10.625 B.
--small: a tenth of the lines (a rehearsal, not a measurement).  Counters are collected in a run of their own (rocprofv3 --pmc
... -- python profiles/pansharpen_bench.py --reps 1 --only scene)."""
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
COPY_CEILING = 6.29e12          # the plain aligned 16-byte copy


def raster(lines, ws, seed, lo=64, hi=4096):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    out = torch.empty(lines, ws, dtype=torch.uint16, device="cuda")
    for r in range(0, lines, 8192):
        m = min(8192, lines - r)
        v = torch.randint(lo, hi, (m, ws), device="cuda", generator=g, dtype=torch.int32)
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
    return {"seconds_median": s, "seconds_min": min(v), "seconds_max": max(v), "GBps": nbytes / s / 1e9, "fraction_of_8TBps_peak": nbytes / s / HBM_PEAK,
            "fraction_of_copy_ceiling": nbytes / s / COPY_CEILING}


def measure(ctx, w, h, reps):
    pan = raster(4 * h, 4 * w, 1, 1500, 2600)                     # a narrow range: PAN / up(low(PAN)) stays within 0.6 .. 1.7
    mss = raster(h, 4 * w, 2)
    low = torch.empty(h, w, dtype=torch.uint16, device="cuda")
    out = torch.empty(4 * h, 16 * w, dtype=torch.uint16, device="cuda")
    st = torch.zeros(2, dtype=torch.int64, device="cuda")
    half = out.view(torch.int16)[:2 * h], out.view(torch.int16)[2 * h:]
    runs = {
        "decimate_box4": lambda: ctx.decimate_box_u16(pan, 4 * w, 4 * w, 4 * h, 1, 4, low, w),
        "pansharpen": lambda: ctx.pansharpen_sfim_u16(pan, mss, low, w, h, out, 4, st),
        "copy_of_product_bytes": lambda: half[1].copy_(half[0]),
    }
    kernels = {"pansharpen": "pansharpen_sfim_kernel"}
    px = 16 * w * h
    nbytes = {"decimate_box4": px * 2 + w * h * 2, "pansharpen": px * 10 + w * h * 10, "copy_of_product_bytes": px * 8}
    for _ in range(2):
        for fn in runs.values():
            fn()
    ctx.sync()
    t = {k: [] for k in runs}
    tk = {k: [] for k in kernels}
    ctx.profile_enable(True)
    for _ in range(reps):
        for k, fn in runs.items():
            ctx.profile_reset()
            t[k].append(timed(fn))
            ctx.sync()
            if k in kernels:
                tk[k].append(ctx.profile()[kernels[k]][0] * 1e-3)
    ctx.profile_enable(False)
    counts = [int(v) for v in st.cpu().numpy()]
    res = {"pan": [4 * w, 4 * h], "mss": [w, h], "reps": reps, "ul_zero_share": counts[0] / (px * (reps + 2.0)), "gain_cut_share": counts[1] / (px * (reps + 2.0))}
    for k in runs:
        res[k] = {"bytes_counted": nbytes[k], "call": summary(t[k], nbytes[k])}
        if k in kernels:
            res[k]["kernel"] = summary(tk[k], nbytes[k])
            res[k]["kernel_name"] = kernels[k]
            res[k]["kernel"]["ns_per_pan_pixel"] = res[k]["kernel"]["seconds_median"] * 1e9 / px
    res["pansharpen_rate_over_copy_rate"] = res["pansharpen"]["kernel"]["GBps"] / res["copy_of_product_bytes"]["call"]["GBps"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--only", choices=["scene", "wide"])
    ap.add_argument("--out")
    a = ap.parse_args()
    ctx = oip.Context(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream)
    div = 10 if a.small else 1
    res = {"tool": "pansharpen_bench", "arch": torch.cuda.get_device_properties(0).gcnArchName.split(":")[0], "small": a.small}
    if a.only != "wide":
        res["scene_24376x100000"] = measure(ctx, 6094, 25000 // div, a.reps)
        torch.cuda.empty_cache()
    if a.only != "scene":
        res["wide_30000x100000"] = measure(ctx, 7500, 25000 // div, a.reps)
    ctx.close()
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
