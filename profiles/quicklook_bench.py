"""Times oip_decimate_box_u16 (F = 16, spp = 1) against its yardstick, oip_colstats_u16 without a mask, on the same
HBM-resident rasters in one process, and prints one JSON line (to be kept as profiles/quicklook_kernel.json and quoted in
DESIGN.md 4.1a).

    python profiles/quicklook_bench.py [--lines 100000] [--reps 20] [--cli DIR]

Device events around each call on the one stream torch and the library share; the two kernels alternate inside the timed
loop, medians are reported.  Both read 2 B/px; the decimator writes 2 / 256 B/px on top.  The other factors, the kernel for
misaligned windows and the histogram of the decimated plane are timed once each for the record.  --cli DIR (a directory on a
RAM-backed file system) adds the MBps lines of `oip quicklook` and `oip rrc-calib` on one 30000 x LINES PAN file: both
stream the file once."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import opticalimageprocessor_amd as oip  # noqa: E402

HBM_PEAK = 8.0e12
MBPS = re.compile(r"bytes in ([0-9.]+) seconds \(([0-9.]+) MBps\)")


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


def summary(v, nbytes):
    s = statistics.median(v)
    return {"seconds_median": s, "seconds_min": min(v), "seconds_max": max(v), "GBps": nbytes / s / 1e9, "fraction_of_8TBps_peak": nbytes / s / HBM_PEAK}


def measure(ctx, img, w, lines, reps):
    F = 16
    ow, oh = -(-w // F), -(-lines // F)
    dst = torch.empty(oh, ow, dtype=torch.uint16, device="cuda")
    acc = torch.zeros(3, w, dtype=torch.int64, device="cuda")
    runs = {"decimate_f16": lambda: ctx.decimate_box_u16(img, w, w, lines, 1, F, dst, ow),
            "colstats": lambda: ctx.colstats_u16(img, w, w, lines, acc)}
    t = {k: [] for k in runs}
    for _ in range(3):
        for fn in runs.values():
            fn()
    ctx.sync()
    for _ in range(reps):
        for k, fn in runs.items():
            t[k].append(timed(fn))
    px = w * lines
    out = {"w": w, "lines": lines, "reps": reps}
    out["decimate_f16"] = summary(t["decimate_f16"], px * 2 + ow * oh * 2)
    out["colstats"] = summary(t["colstats"], px * 2)
    out["decimate_over_colstats_time"] = out["decimate_f16"]["seconds_median"] / out["colstats"]["seconds_median"]
    # for the record: the other factors, the kernel for misaligned windows (one pixel in), the histogram of the decimated plane
    other = {}
    for f in (2, 4, 8, 32, 64):
        d2 = torch.empty(-(-lines // f), -(-w // f), dtype=torch.uint16, device="cuda")
        fn = lambda: ctx.decimate_box_u16(img, w, w, lines, 1, f, d2, d2.shape[1])  # noqa: E731
        fn()
        other["decimate_f%d_seconds" % f] = statistics.median([timed(fn) for _ in range(5)])
        del d2
    fn = lambda: ctx.decimate_box_u16(img.data_ptr() + 2, w, w - 8, lines, 1, F, dst, ow)  # noqa: E731
    fn()
    other["decimate_f16_misaligned_seconds"] = statistics.median([timed(fn) for _ in range(3)])
    hist = torch.zeros(65536, dtype=torch.int64, device="cuda")
    fn = lambda: ctx.histogram_u16(dst, ow, ow, oh, hist)  # noqa: E731
    fn()
    other["histogram_of_decimated_plane_seconds"] = statistics.median([timed(fn) for _ in range(5)])
    out["other"] = other
    return out


def cli(a, img, res):
    path = os.path.join(a.cli, "quicklook_bench_PAN.RAW")
    outs = [os.path.join(a.cli, "quicklook_bench_PAN.QL.TIFF"), os.path.join(a.cli, "quicklook_bench_pan.csv"), os.path.join(a.cli, "quicklook_bench_oip.log")]
    exe = os.path.join(ROOT, "opticalimageprocessor_amd", "lib", "oip")
    env = dict(os.environ, LOGFILE=outs[2])
    try:
        img.cpu().numpy().tofile(path)
        rec = {"file_bytes": os.path.getsize(path)}
        cmds = {"quicklook": [exe, "quicklook", path, "--width", "30000", "-o", outs[0], "--force"],
                "rrc_calib": [exe, "rrc-calib", "--width", "30000", "--pan", path, "--rrc-pan", outs[1], "--force"]}
        for _ in range(2):                                                       # the second round is the one recorded
            for k, cmd in cmds.items():
                r = subprocess.run(cmd, env=env, capture_output=True, text=True)
                if r.returncode != 0:
                    raise RuntimeError(r.stdout + r.stderr)
                m = MBPS.findall(r.stdout)[-1]
                rec[k] = {"seconds": float(m[0]), "MBps": float(m[1])}
        res["cli_w30000"] = rec
    except (OSError, RuntimeError) as e:                                         # e.g. DIR too small: the kernel figures stand
        res["cli_w30000"] = {"error": repr(e)[:300]}
    finally:
        for f in [path] + outs:
            if os.path.exists(f):
                os.remove(f)


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
    res = {"tool": "quicklook_bench", "arch": torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]}
    img = raster(a.lines, 30000, 1)
    res["w30000"] = measure(ctx, img, 30000, a.lines, a.reps)
    if a.cli:
        cli(a, img, res)
    del img
    torch.cuda.empty_cache()
    img = raster(a.lines, 12288, 2)
    res["w12288"] = measure(ctx, img, 12288, a.lines, a.reps)
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
