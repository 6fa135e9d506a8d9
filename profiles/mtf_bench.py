"""Times the two passes of `oip mtf` (oip_mtf_tiles_u16 on either axis, oip_mtf_esf_u16 on the status-0 tiles of axis x) against
their yardstick, oip_noise_blocks_u16 (a read-once pass over the same bytes), on the same HBM-resident raster in one process,
and prints one JSON line (committed as profiles/mtf_kernel.json, quoted in DESIGN.md).

    python profiles/mtf_bench.py [--lines 100000] [--reps 10]

Device events around each call on the one stream torch and the library share; the kernels alternate inside the timed loop,
medians are reported.  Bytes are what the algorithm needs: pass 1 reads 2 B per sample once (the records are 16 B per 1024
samples and axis, and are left out); pass 2 reads 2 KB and writes 512 B per listed tile.  The raster is synth.edge_field:
30000 x LINES samples, a quarter of the cells an x edge, a quarter a y edge, a quarter flat, a quarter texture."""
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
from opticalimageprocessor_amd import synth  # noqa: E402

HBM_PEAK = 8.0e12
W = 30000


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
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    L = a.lines
    ctx = oip.Context(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream)
    img = synth.edge_field(L, W, 1)
    keys = torch.zeros((W // 8) * (L // 8), dtype=torch.int16, device="cuda")
    geo = {"x": (L // 32, (W - 32) // 16 + 1), "y": ((L - 32) // 16 + 1, W // 32)}
    rec = {k: torch.zeros(nty, ntx, 4, dtype=torch.int32, device="cuda") for k, (nty, ntx) in geo.items()}
    runs = {"noise_spp1_b8": lambda: ctx.noise_blocks_u16(img, W, W, L, 1, 8, 4, keys, W // 8, 0)}
    for k in ("x", "y"):
        runs["mtf_tiles_" + k] = lambda k=k: ctx.mtf_tiles_u16(img, W, W, L, 1, k, rec[k], geo[k][1], 0)
    for fn in runs.values():
        fn()
    ctx.sync()
    status = {k: np.bincount(rec[k][..., 0].cpu().numpy().ravel(), minlength=8).tolist() for k in rec}
    ok = torch.nonzero(rec["x"][..., 0] == 0).to(torch.int32)
    n = ok.shape[0]
    entries = torch.cat([torch.zeros(n, 1, dtype=torch.int32, device="cuda"), ok], dim=1).contiguous()
    esf = torch.zeros(max(n, 1), 128, dtype=torch.int32, device="cuda")
    runs["mtf_esf_x"] = lambda: ctx.mtf_esf_u16(img, W, W, L, 1, "x", entries, n, esf)
    t = {k: [] for k in runs}
    for _ in range(2):
        for fn in runs.values():
            fn()
    ctx.sync()
    for _ in range(a.reps):
        for k, fn in runs.items():
            t[k].append(timed(fn))
    nbytes = 2 * W * L
    res = {"tool": "mtf_bench", "arch": torch.cuda.get_device_properties(0).gcnArchName.split(":")[0], "w": W, "lines": L, "reps": a.reps,
           "bytes_read": nbytes, "tiles": {k: geo[k][0] * geo[k][1] for k in geo}, "status_counts": status, "esf_tiles": n}
    for k, v in t.items():
        s = statistics.median(v)
        b = n * (2048 + 512) if k == "mtf_esf_x" else nbytes
        res[k] = {"seconds_median": s, "seconds_min": min(v), "seconds_max": max(v), "bytes": b, "GBps": b / s / 1e9, "fraction_of_8TBps_peak": b / s / HBM_PEAK}
    for k in ("mtf_tiles_x", "mtf_tiles_y"):
        res[k]["time_over_noise"] = res[k]["seconds_median"] / res["noise_spp1_b8"]["seconds_median"]
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
