"""Times oip_stitch_balanced_u16 and oip_seam_moments_u16 against their yardstick, oip_stitch_rows_u16, on the same
HBM-resident image pairs in one process, and prints one JSON line (to be kept as profiles/seam_kernel.json and quoted in
DESIGN.md 4.1b).

    python profiles/seam_bench.py [--reps 20] [--small]

Two geometries: a PAN pair of 30000 x 100000 with --fold-cols 200 (fold 100, spp 1) and an aligned-MSS pair of
7500 x 25000 x 4 with --fold-cols 50 (fold 25, spp 4).  Device events around each call on the one stream torch and the
library share; the four calls alternate inside the timed loop, medians are reported with the extremes.  The plain stitch and
the balanced one move the same bytes (2 B in, 2 B out per output sample) plus, with h = fold, the second image's samples
of the blend zone; the moments pass reads 2 * 2 fold * spp samples per line.  --small: a tenth of the lines (a rehearsal,
not a measurement)."""
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


def raster(lines, ws, seed, scale=1.0):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    out = torch.empty(lines, ws, dtype=torch.uint16, device="cuda")
    for r in range(0, lines, 8192):
        m = min(8192, lines - r)
        v = torch.randint(64, 4096, (m, ws), device="cuda", generator=g, dtype=torch.int32)
        out[r:r + m] = (v * scale).to(torch.int32).to(torch.int16).view(torch.uint16)
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


def measure(ctx, W, L, fold, spp, reps):
    ws, fs = W * spp, fold * spp
    left, right = raster(L, ws, 1), raster(L, ws, 2, 0.9)
    out = torch.empty(L, 2 * (ws - fs), dtype=torch.uint16, device="cuda")
    acc = torch.zeros(6, spp, dtype=torch.int64, device="cuda")
    ctx.seam_moments_u16(left, right, ws, L, fs, spp, acc, 1, 65535)
    ctx.sync()
    G, O, ident, report = oip.seam_fit(acc.cpu().numpy().view(np.uint64), "gain", 0)
    ident_g = torch.full((spp,), 65536, dtype=torch.int32, device="cuda")
    zero_o = torch.zeros(spp, dtype=torch.int32, device="cuda")
    fit_g, fit_o = torch.from_numpy(G).cuda(), torch.from_numpy(O).cuda()
    runs = {"stitch_rows": lambda: ctx.stitch_rows_u16(left, right, out, ws, L, fs),
            "balanced_identity_h0": lambda: ctx.stitch_balanced_u16(left, right, out, ws, L, fs, spp, ident_g, zero_o, 0, 1),
            "balanced_fitted_hfold": lambda: ctx.stitch_balanced_u16(left, right, out, ws, L, fs, spp, fit_g, fit_o, fold, 1),
            "seam_moments": lambda: ctx.seam_moments_u16(left, right, ws, L, fs, spp, acc, 1, 65535)}
    t = {k: [] for k in runs}
    for _ in range(3):
        for fn in runs.values():
            fn()
    ctx.sync()
    for _ in range(reps):
        for k, fn in runs.items():
            t[k].append(timed(fn))
    stitch_bytes = 2 * out.numel() * 2
    res = {"W": W, "lines": L, "fold": fold, "spp": spp, "reps": reps, "gain_q16": G.tolist(), "offset_q16": O.tolist()}
    res["stitch_rows"] = summary(t["stitch_rows"], stitch_bytes)
    res["balanced_identity_h0"] = summary(t["balanced_identity_h0"], stitch_bytes)
    res["balanced_fitted_hfold"] = summary(t["balanced_fitted_hfold"], stitch_bytes + 2 * fs * L * 2)
    res["seam_moments"] = summary(t["seam_moments"], 2 * 2 * fs * L * 2)
    base = res["stitch_rows"]["seconds_median"]
    for k in ("balanced_identity_h0", "balanced_fitted_hfold", "seam_moments"):
        res[k + "_over_stitch_rows_time"] = res[k]["seconds_median"] / base
    # run-to-run spread of the yardstick itself: what a ratio near 1 has to be read against
    res["stitch_rows_spread"] = (res["stitch_rows"]["seconds_max"] - res["stitch_rows"]["seconds_min"]) / base
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
    res = {"tool": "seam_bench", "arch": torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]}
    res["pan_30000x100000_fold100"] = measure(ctx, 30000, 100000 // div, 100, 1, a.reps)
    torch.cuda.empty_cache()
    res["mss_7500x25000x4_fold25"] = measure(ctx, 7500, 25000 // div, 25, 4, a.reps)
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
