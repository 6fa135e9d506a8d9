"""Times oip_colstats_u16 against its yardstick, oip_rrc_u16, on the same HBM-resident raster in one process, and prints one
JSON line (committed as profiles/colstats_kernel.json, quoted in DESIGN.md 4.1).

    python profiles/colstats_bench.py [--lines 100000] [--reps 20] [--cli DIR]

Device events around each call on the one stream torch and the library share; the two kernels alternate inside the timed
loop, medians are reported.  Bytes are what the algorithm needs: 2 B/px for the statistics, 4 B/px for RRC.  --cli DIR
(a directory on a RAM-backed file system) adds the wall time of `oip rrc-calib` on a 30000 x LINES PAN file next to the
time the staging layer needs merely to read that file into HBM."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import opticalimageprocessor_amd as oip  # noqa: E402
from opticalimageprocessor_amd import synth  # noqa: E402

HBM_PEAK = 8.0e12


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


def measure(ctx, img, pitch, w, lines, reps, with_rrc, ptr_offset=0):
    acc = torch.zeros(3, w, dtype=torch.int64, device="cuda")
    src = img.data_ptr() + 2 * ptr_offset
    stats = lambda: ctx.colstats_u16(src, pitch, w, lines, acc)  # noqa: E731
    runs = {"colstats": stats}
    if with_rrc:
        dst = torch.empty_like(img)
        kb = ctx.upload_kb(synth.lut(w))
        runs["rrc"] = lambda: ctx.rrc_u16(img, dst, w, lines, kb)
    t = {k: [] for k in runs}
    for _ in range(3):
        for fn in runs.values():
            fn()
    ctx.sync()
    for _ in range(reps):
        for k, fn in runs.items():
            t[k].append(timed(fn))
    px = w * lines
    out = {"w": w, "lines": lines, "pitch": pitch, "reps": reps}
    for k, v in t.items():
        s = statistics.median(v)
        bpp = 2 if k == "colstats" else 4
        out[k] = {"seconds_median": s, "seconds_min": min(v), "seconds_max": max(v), "bytes_per_px": bpp, "GBps": px * bpp / s / 1e9,
                  "fraction_of_8TBps_peak": px * bpp / s / HBM_PEAK}
    if with_rrc:
        out["colstats_over_rrc_time"] = out["colstats"]["seconds_median"] / out["rrc"]["seconds_median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cli", default="")
    a = ap.parse_args()
    ctx = oip.Context(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream)
    res = {"tool": "colstats_bench", "arch": torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]}
    img = raster(a.lines, 30000, 1)
    res["w30000"] = measure(ctx, img, 30000, 30000, a.lines, a.reps, True)
    # the same raster seen as a window that starts one pixel in: no 16-byte alignment, the column-per-lane kernel
    res["w29992_misaligned"] = measure(ctx, img, 30000, 29992, a.lines, a.reps, False, ptr_offset=1)
    if a.cli:
        path = os.path.join(a.cli, "colstats_bench_PAN.RAW")
        out = os.path.join(a.cli, "colstats_bench_pan.csv")
        nbytes = a.lines * 30000 * 2
        try:
            img.cpu().numpy().tofile(path)
            dst = torch.empty_like(img)
            ctx.read_file_to_device(path, dst)                                   # page cache and pinned ring warm
            ctx.sync()
            t0 = time.perf_counter()
            ctx.read_file_to_device(path, dst)
            ctx.sync()
            read_s = time.perf_counter() - t0
            del dst
            exe = os.path.join(ROOT, "opticalimageprocessor_amd", "lib", "oip")
            env = dict(os.environ, LOGFILE=os.path.join(a.cli, "colstats_bench_oip.log"))
            walls = []
            for _ in range(2):
                t0 = time.perf_counter()
                r = subprocess.run([exe, "rrc-calib", "--width", "30000", "--pan", path, "--rrc-pan", out, "--force"], env=env,
                                   capture_output=True, text=True)
                walls.append(time.perf_counter() - t0)
                if r.returncode != 0:
                    raise RuntimeError(r.stdout + r.stderr)
            m = re.search(r"bytes in ([0-9.]+) seconds \(([0-9.]+) MBps\)", r.stdout)        # the command's own read + statistics line
            res["cli_w30000"] = {"file_bytes": nbytes, "rrc_calib_wall_seconds": walls, "read_only_seconds_in_process": read_s,
                                 "read_only_GBps": nbytes / read_s / 1e9, "read_and_stats_seconds": float(m.group(1)) if m else None,
                                 "read_and_stats_MBps": float(m.group(2)) if m else None}
        except (OSError, RuntimeError) as e:                                     # e.g. DIR too small: the kernel figures stand
            res["cli_w30000"] = {"error": repr(e)[:300]}
        finally:
            for f in (path, out, os.path.join(a.cli, "colstats_bench_oip.log")):
                if os.path.exists(f):
                    os.remove(f)
    del img
    torch.cuda.empty_cache()
    img = raster(a.lines, 12288, 2)
    res["w12288"] = measure(ctx, img, 12288, 12288, a.lines, a.reps, True)
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
