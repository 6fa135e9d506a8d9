"""Times oip_stitch_balanced_lines_u16 and oip_seam_moments_blocks_u16 against their yardsticks, oip_stitch_balanced_u16 and
oip_seam_moments_u16, on the same HBM-resident image pairs in one process, and prints one JSON line (to be kept as
profiles/seam_lines_kernel.json and quoted in DESIGN.md 4.1b).

    python profiles/seam_lines_bench.py [--reps 20] [--small]

Two geometries, as profiles/seam_bench.py: a PAN pair of 30000 x 100000 with fold 100 (spp 1) and an aligned-MSS pair of
7500 x 25000 x 4 with fold 25 (spp 4).  Device events around each call on the one stream torch and the library share; the
six calls alternate inside the timed loop, medians are reported with the extremes.  The per-line stitch moves the bytes of
the balanced one plus 8 * spp bytes of table per line; it runs once on the fitted pair repeated on every line and once on
tables that drift along the strip (gain 0.90 -> 1.10, offset 40 -> -25 DN).  The block moments run at B = 1024.
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
BLOCK_LINES = 1024


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
    nb = max(1, L // BLOCK_LINES)
    acc = torch.zeros(6, spp, dtype=torch.int64, device="cuda")
    acc_blocks = torch.zeros(nb, 6, spp, dtype=torch.int64, device="cuda")
    ctx.seam_moments_u16(left, right, ws, L, fs, spp, acc, 1, 65535)
    ctx.sync()
    G, O, ident, report = oip.seam_fit(acc.cpu().numpy().view(np.uint64), "gain", 0)
    fit_g, fit_o = torch.from_numpy(G).cuda(), torch.from_numpy(O).cuda()
    const_g, const_o = (torch.from_numpy(np.ascontiguousarray(np.tile(v, (L, 1)))).cuda() for v in (G, O))
    t = np.linspace(0.0, 1.0, L)[:, None] * np.ones((1, spp))
    drift_g = torch.from_numpy(np.rint((0.90 + 0.20 * t) * 65536).astype(np.int32)).cuda()
    drift_o = torch.from_numpy(np.rint((40.0 - 65.0 * t) * 65536).astype(np.int32)).cuda()
    runs = {"stitch_rows": lambda: ctx.stitch_rows_u16(left, right, out, ws, L, fs),
            "balanced_fitted_hfold": lambda: ctx.stitch_balanced_u16(left, right, out, ws, L, fs, spp, fit_g, fit_o, fold, 1),
            "lines_constant_hfold": lambda: ctx.stitch_balanced_lines_u16(left, right, out, ws, L, fs, spp, const_g, const_o, fold, 1),
            "lines_drifting_hfold": lambda: ctx.stitch_balanced_lines_u16(left, right, out, ws, L, fs, spp, drift_g, drift_o, fold, 1),
            "seam_moments": lambda: ctx.seam_moments_u16(left, right, ws, L, fs, spp, acc, 1, 65535),
            "seam_moments_blocks": lambda: ctx.seam_moments_blocks_u16(left, right, ws, L, fs, spp, BLOCK_LINES, acc_blocks, 1, 65535)}
    times = {k: [] for k in runs}
    for _ in range(3):
        for fn in runs.values():
            fn()
    ctx.sync()
    for _ in range(reps):
        for k, fn in runs.items():
            times[k].append(timed(fn))
    stitch_bytes = 2 * out.numel() * 2
    blend_bytes = 2 * fs * L * 2
    res = {"W": W, "lines": L, "fold": fold, "spp": spp, "reps": reps, "block_lines": BLOCK_LINES, "blocks": nb, "gain_q16": G.tolist(),
           "offset_q16": O.tolist()}
    res["stitch_rows"] = summary(times["stitch_rows"], stitch_bytes)
    res["balanced_fitted_hfold"] = summary(times["balanced_fitted_hfold"], stitch_bytes + blend_bytes)
    for k in ("lines_constant_hfold", "lines_drifting_hfold"):
        res[k] = summary(times[k], stitch_bytes + blend_bytes + 8 * spp * L)
    for k in ("seam_moments", "seam_moments_blocks"):
        res[k] = summary(times[k], 2 * 2 * fs * L * 2)
    # the yardsticks in this run, and their own min-to-max spread: what a ratio near 1 has to be read against
    for k, base in (("lines_constant_hfold", "balanced_fitted_hfold"), ("lines_drifting_hfold", "balanced_fitted_hfold"),
                    ("balanced_fitted_hfold", "stitch_rows"), ("seam_moments_blocks", "seam_moments")):
        res[k + "_over_" + base + "_time"] = res[k]["seconds_median"] / res[base]["seconds_median"]
    for base in ("balanced_fitted_hfold", "seam_moments"):
        res[base + "_spread"] = (res[base]["seconds_max"] - res[base]["seconds_min"]) / res[base]["seconds_median"]
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
    res = {"tool": "seam_lines_bench", "arch": torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]}
    res["pan_30000x100000_fold100"] = measure(ctx, 30000, 100000 // div, 100, 1, a.reps)
    torch.cuda.empty_cache()
    res["mss_7500x25000x4_fold25"] = measure(ctx, 7500, 25000 // div, 25, 4, a.reps)
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
