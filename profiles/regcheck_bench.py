"""Times oip_match_tiles_u16, the kernel of `oip regcheck`, on HBM-resident rasters in one process and prints one JSON line
(to be kept as profiles/regcheck_kernel.json and quoted in DESIGN.md 4.1g).

    python profiles/regcheck_bench.py [--reps 7] [--small]

Two cases, both T = 64, S = 4, step 64 (the command's defaults):
    pan_dense    two PAN strips of 30000 x 100000 (6 GB each, stride 1): 467 x 1561 = 7.3e5 tiles, 2.4e11 sample-offsets
    mss_default  band 2 against band 1 of one aligned product of 7500 x 25000 x 4 (1.5 GB, stride 4): 117 x 390 tiles
Device events around each call on the one stream torch and the library share; medians with the extremes.  The yardstick is what
the command cannot avoid, reading and uploading its images: 0.219 s per 6 GB (the project's figure, rrc-calib); the kernel time
is given as a fraction of that.  Data: uniform 12-bit values -- the kernel's time does not depend on the values.
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

READ_UPLOAD_SECONDS_PER_BYTE = 0.219 / 6.0e9
T, S, STEP = 64, 4, 64


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


def measure(ctx, a, b, w, rows, stride, file_bytes, reps):
    """a, b: device addresses of the planes, both of `stride` and of pitch w * stride"""
    x0, y0, nx, ny = oip.match_grid(w, rows, T, S, STEP)
    rec = torch.empty(nx * ny * oip.capi.MATCH_RECORD_WORDS, dtype=torch.int64, device="cuda")
    fn = lambda: ctx.match_tiles_u16(a, w * stride, stride, b, w * stride, stride, w, rows, T, S, x0, y0, STEP, STEP, nx, ny, 1, 65535, rec)  # noqa: E731
    for _ in range(2):
        fn()
    ctx.sync()
    t = [timed(fn) for _ in range(reps)]
    s = statistics.median(t)
    macs = nx * ny * (2 * S + 1) ** 2 * T * T
    io = file_bytes * READ_UPLOAD_SECONDS_PER_BYTE
    return {"w": w, "rows": rows, "stride": stride, "tiles": nx * ny, "sample_offsets": macs, "reps": reps, "seconds_median": s, "seconds_min": min(t),
            "seconds_max": max(t), "sample_offsets_per_second": macs / s, "tiles_per_second": nx * ny / s, "file_bytes": file_bytes,
            "read_upload_seconds": io, "kernel_over_read_upload": s / io}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--small", action="store_true")
    a = ap.parse_args()
    ctx = oip.Context(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream)
    div = 10 if a.small else 1
    res = {"tool": "regcheck_bench", "arch": torch.cuda.get_device_properties(0).gcnArchName.split(":")[0], "T": T, "S": S, "step": STEP}
    W, L = 30000, 100000 // div
    pa, pb = raster(L, W, 1), raster(L, W, 2)
    res["pan_dense"] = measure(ctx, pa.data_ptr(), pb.data_ptr(), W, L, 1, 2 * W * L * 2, a.reps)
    del pa, pb
    torch.cuda.empty_cache()
    W, L = 7500, 25000 // div
    m = raster(L, W * 4, 3)
    res["mss_default"] = measure(ctx, m.data_ptr(), m.data_ptr() + 2, W, L, 4, W * L * 4 * 2, a.reps)
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
