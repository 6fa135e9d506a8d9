"""Times oip_interband_correlate_units where the peak search of the spectral route cannot prune: ten 16000 x 3000 units
whose PAN and band windows are independent 12-bit noise, so that every column bound exceeds every surface value and all
lane tiles are searched.  Prints one JSON line (kept as profiles/peak_prune.json).

    python profiles/peak_prune_bench.py [--reps 10] [--units 10] [--kernels]

Run it on two builds of the library on the same box, interleaved, to compare them (OIP_LIBRARY names another build; a
build without oip_peak_prune_stats reports no tile counts).  Host wall time around the call, which ends with the
download of the results; medians with the extremes."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import opticalimageprocessor_amd as oip  # noqa: E402

ROWS, COLS = 16000, 3000


def noise(rows, cols, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    v = torch.randint(0, 4096, (rows, cols), device="cuda", generator=g, dtype=torch.int32)
    return v.to(torch.int16).view(torch.uint16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--units", type=int, default=10)
    ap.add_argument("--kernels", action="store_true", help="add the library profiler's per-kernel times of one more call")
    a = ap.parse_args()
    ctx = oip.Context(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream)
    pans = [noise(ROWS, COLS, 100 + u) for u in range(a.units)]
    bands = [[noise(ROWS // 4, COLS // 4, 1000 + 4 * u + b) for b in range(4)] for u in range(a.units)]
    run = lambda: ctx.interband_correlate_units(pans, [COLS] * a.units, bands, [COLS // 4] * a.units, ROWS, COLS)
    stats = getattr(ctx, "peak_prune_stats", None)
    for _ in range(2):
        res = run()
    if stats:
        stats()
    t = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = run()
        t.append(time.perf_counter() - t0)
    out = {"tool": "peak_prune_bench", "arch": torch.cuda.get_device_properties(0).gcnArchName.split(":")[0],
           "library": os.environ.get("OIP_LIBRARY", "in-tree"), "units": a.units, "rows": ROWS, "cols": COLS, "reps": a.reps,
           "ms_median": 1e3 * statistics.median(t), "ms_min": 1e3 * min(t), "ms_max": 1e3 * max(t),
           "largest_response": float(res[..., 2].max())}
    if stats:
        searched, total = stats()
        out["tiles_searched"], out["tiles_total"] = searched, total
    if a.kernels:
        ctx.profile_enable(True)
        ctx.profile_reset()
        run()
        ctx.sync()
        out["kernels_ms_total_and_launches"] = {k: [round(ms, 4), n] for k, (ms, n) in ctx.profile().items()}
        ctx.profile_enable(False)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
