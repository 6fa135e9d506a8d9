"""Times oip_rescale_u16 against code that exists, on one HBM-resident raster in one process, and prints one JSON line (quoted in
profiles/rescale_speed.md and DESIGN.md):

  same_cubic   `cubic` at equal sizes (4 x 4 taps)  against  oip_warp_grid_bicubic_u16 with a zero field: the same 16-sample
                                                             footprint, taken separably here (8 multiply-adds a sample against 16)
  up4          x 4 on both axes (lanczos, 6 x 6)     against  a device-to-device copy of the bytes read plus the bytes written
  quarter      1/4 on both axes (lanczos, 24 x 24)   against  a device-to-device copy of the bytes read plus the bytes written

    python profiles/rescale_bench.py [--width 6144] [--lines 60000] [--reps 10] [--spp 1,4]

Device events on the stream the context shares with torch give the times; the runs alternate inside the timed loop, medians
are reported with the minimum and maximum.  Bytes are what the algorithm needs: 2 B per source sample read and 2 B per output
sample written (the tables are noise).  A copy of n bytes reads n and writes n, so the yardstick copies (read + written) / 2."""
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
from opticalimageprocessor_amd import capi  # noqa: E402

HBM_PEAK = 8.0e12


def raster(lines, ws, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    out = torch.empty(lines, ws, dtype=torch.uint16, device="cuda")
    for r in range(0, lines, 4096):
        m = min(4096, lines - r)
        out[r:r + m] = torch.randint(64, 4096, (m, ws), device="cuda", generator=g, dtype=torch.int32).to(torch.int16).view(torch.uint16)
    return out


def tables(kind, W, Wo, L, Lo):
    fx, tx = capi.rescale_taps(kind, W, Wo)
    fy, ty = capi.rescale_taps(kind, L, Lo)
    return [torch.from_numpy(a).cuda() for a in (fx, tx, fy, ty)] + [tx.shape[1], ty.shape[1]]


def timed(fn, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=6144)
    ap.add_argument("--lines", type=int, default=60000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--spp", default="1,4")
    a = ap.parse_args()
    ctx = oip.Context(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream)
    res = {"tool": "rescale_bench", "arch": torch.cuda.get_device_properties(0).gcnArchName.split(":")[0], "width": a.width, "lines": a.lines, "reps": a.reps}
    for spp in [int(s) for s in a.spp.split(",")]:
        W, L = a.width, a.lines
        img = raster(L, W * spp, spp)
        zero = np.zeros((2, 2), np.int32)
        for name, kind, Wo, Lo in (("same_cubic", "cubic", W, L), ("up4", "lanczos", 4 * W, 4 * L), ("quarter", "lanczos", W // 4, L // 4)):
            fx, tx, fy, ty, Kx, Ky = tables(kind, W, Wo, L, Lo)
            moved = 2 * spp * (W * L + Wo * Lo)
            free = torch.cuda.mem_get_info()[0]
            if 2 * spp * Wo * Lo + moved > 0.9 * free:                  # the output and the two buffers of the copy
                res["spp%d_%s" % (spp, name)] = {"skipped": "needs %d bytes of device memory, %d free" % (2 * spp * Wo * Lo + moved, free)}
                continue
            out = torch.empty(Lo, Wo * spp, dtype=torch.uint16, device="cuda")
            runs = {"rescale": lambda: ctx.rescale_u16(img, 0, L, W, L, spp, out, 0, Lo, Wo, Lo, fx, tx, Kx, fy, ty, Ky, 0)}
            if name == "same_cubic":
                runs["rescale_valid_min_1"] = lambda: ctx.rescale_u16(img, 0, L, W, L, spp, out, 0, Lo, Wo, Lo, fx, tx, Kx, fy, ty, Ky, 1)
                runs["warp_zero_field"] = lambda: ctx.warp_grid_bicubic_u16(img, out, W, L, spp, zero, zero, 0, 0, W, L)
            ca = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
            cb = torch.empty_like(ca)
            runs["copy"] = lambda: cb.copy_(ca)
            t = {k: [] for k in runs}
            for _ in range(2):
                for fn in runs.values():
                    fn()
            ctx.sync()
            torch.cuda.synchronize()
            for _ in range(a.reps):
                for k, fn in runs.items():
                    t[k].append(timed(fn, stream))
            entry = {"out": [Wo, Lo], "taps": [Kx, Ky], "bytes": moved}
            for k, v in t.items():
                s = statistics.median(v)
                entry[k] = {"seconds_median": s, "seconds_min": min(v), "seconds_max": max(v), "GBps": moved / s / 1e9,
                            "fraction_of_8TBps_peak": moved / s / HBM_PEAK}
            yard = "warp_zero_field" if name == "same_cubic" else "copy"
            entry["time_over_" + yard] = entry["rescale"]["seconds_median"] / entry[yard]["seconds_median"]
            entry["time_over_copy"] = entry["rescale"]["seconds_median"] / entry["copy"]["seconds_median"]
            res["spp%d_%s" % (spp, name)] = entry
            del out, ca, cb, fx, tx, fy, ty
            torch.cuda.empty_cache()
        del img
        torch.cuda.empty_cache()
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
