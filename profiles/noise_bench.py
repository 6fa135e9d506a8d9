"""Times oip_noise_blocks_u16 against its yardstick, oip_colstats_u16 (a read-only pass with the same traffic), on the same
HBM-resident raster in one process, and prints one JSON line (committed as profiles/noise_kernel.json, quoted in DESIGN.md 4.2c).

    python profiles/noise_bench.py [--lines 100000] [--reps 20]

Device events around each call on the one stream torch and the library share; the kernels alternate inside the timed loop,
medians are reported.  Bytes are what the algorithm needs: 2 B per sample read (the keys are 1/64 of that at B 8 and less at
B 16, and are left out).  The raster is 30000 x LINES samples, seen as spp 1 at B 8 and B 16 and as 7500 pixels of 4 samples at
B 8; colstats reads the same bytes as 30000 columns."""
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
W = 30000


def raster(lines, w, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    out = torch.empty(lines, w, dtype=torch.uint16, device="cuda")
    for r in range(0, lines, 8192):
        m = min(8192, lines - r)
        out[r:r + m] = torch.randint(64, 4096, (m, w), device="cuda", generator=g, dtype=torch.int32).to(torch.int16).view(torch.uint16)
    return out


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    ctx = oip.Context(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream)
    img = raster(a.lines, W, 1)
    acc = torch.zeros(3, W, dtype=torch.int64, device="cuda")
    keys = torch.zeros(4 * (W // 8) * (a.lines // 8), dtype=torch.int16, device="cuda")
    runs = {"colstats": lambda: ctx.colstats_u16(img, W, W, a.lines, acc)}
    for name, spp, B in (("noise_spp1_b8", 1, 8), ("noise_spp1_b16", 1, 16), ("noise_spp4_b8", 4, 8)):
        px = W // spp
        nbx, nby = px // B, a.lines // B
        runs[name] = lambda px=px, spp=spp, B=B, nbx=nbx, nby=nby: ctx.noise_blocks_u16(img, W, px, a.lines, spp, B, 4, keys, nbx, nbx * nby)
    t = {k: [] for k in runs}
    for _ in range(3):
        for fn in runs.values():
            fn()
    ctx.sync()
    for _ in range(a.reps):
        for k, fn in runs.items():
            t[k].append(timed(fn))
    nbytes = 2 * W * a.lines
    res = {"tool": "noise_bench", "arch": torch.cuda.get_device_properties(0).gcnArchName.split(":")[0], "w": W, "lines": a.lines, "reps": a.reps,
           "bytes_read": nbytes}
    for k, v in t.items():
        s = statistics.median(v)
        res[k] = {"seconds_median": s, "seconds_min": min(v), "seconds_max": max(v), "GBps": nbytes / s / 1e9, "fraction_of_8TBps_peak": nbytes / s / HBM_PEAK}
    for k in t:
        if k != "colstats":
            res[k]["time_over_colstats"] = res[k]["seconds_median"] / res["colstats"]["seconds_median"]
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
