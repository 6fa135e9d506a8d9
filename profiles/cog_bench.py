"""Times oip_retile_u16 and oip_untile_u16 against their yardstick, a device-to-device copy of the same bytes (torch's copy_ of
the raster: hipMemcpyAsync on the stream), on HBM-resident rasters in one process, and prints one JSON line (to be kept as
profiles/cog_kernel.json and quoted in profiles/cog_speed.md and DESIGN.md 4.1g).

    python profiles/cog_bench.py [--reps 20] [--small] [--cli DIR]

Two geometries: a PAN strip of 12288 x 60000 x 1 and an image of 6144 x 60000 x 4, tiles of 256 and 128.  Device events around
each call on the one stream torch and the library share; the calls alternate inside the timed loop, medians are reported with
the extremes.  Every call reads the raster once and writes it once (2 B in, 2 B out per sample; the tile-major form of these
sizes has at most 0.5 % of padding, counted as written).  Data: 12-bit sensor values, uniform in [64, 4096).
--small: a tenth of the lines (a rehearsal, not a measurement).
--cli DIR: also the command line in DIR (a scratch directory): the image of 4 samples as a strip TIFF, then `oip cog --tile 256`,
`oip cog --tile 128` and `oip overviews` on it, wall time and the `TIMING tiff_lzw` lines of each (the device encoder's own
split: tiles of 512 KiB and 128 KiB a lane against strips of 64 KiB)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import opticalimageprocessor_amd as oip  # noqa: E402

HBM_PEAK = 8.0e12


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


def summary(v, nbytes):
    s = statistics.median(v)
    return {"seconds_median": s, "seconds_min": min(v), "seconds_max": max(v), "GBps": nbytes / s / 1e9, "fraction_of_8TBps_peak": nbytes / s / HBM_PEAK}


def measure(ctx, W, L, spp, reps):
    ws = W * spp
    src = raster(L, ws, 1)
    back = torch.empty_like(src)
    runs = {"copy_d2d": lambda: back.view(torch.int16).copy_(src.view(torch.int16))}
    bufs = {}
    for T in (256, 128):
        tx, ty = -(-W // T), -(-L // T)
        tiles = bufs[T] = torch.empty(tx * ty * T * T * spp, dtype=torch.uint16, device="cuda")
        runs["retile_T%d" % T] = lambda T=T, ty=ty, tiles=tiles: ctx.retile_u16(src, ws, W, L, spp, T, 0, ty, tiles)
        runs["untile_T%d" % T] = lambda T=T, ty=ty, tiles=tiles: ctx.untile_u16(tiles, W, L, spp, T, 0, ty, back, ws)
    t = {k: [] for k in runs}
    for _ in range(3):
        for fn in runs.values():
            fn()
    ctx.sync()
    assert torch.equal(back.view(torch.int16), src.view(torch.int16))       # (the last run was untile_T128 of retile_T128)
    for _ in range(reps):
        for k, fn in runs.items():
            t[k].append(timed(fn))
    nbytes = src.numel() * 4
    res = {"W": W, "lines": L, "spp": spp, "reps": reps, "bytes_per_sample": 4}
    for k in runs:
        res[k] = summary(t[k], nbytes)
    base = res["copy_d2d"]
    res["copy_d2d_spread"] = (base["seconds_max"] - base["seconds_min"]) / base["seconds_median"]
    for k in runs:
        if k != "copy_d2d":
            res[k + "_over_copy_time"] = res[k]["seconds_median"] / base["seconds_median"]
    return res


def cli(d, lines):
    """wall times and encoder splits of the command line on a 6144 x `lines` x 4 strip TIFF"""
    exe = os.path.join(ROOT, "opticalimageprocessor_amd", "lib", "oip")
    img = raster(lines, 6144 * 4, 2).cpu().numpy()
    env = dict(os.environ, LOGFILE=os.path.join(d, "oip.log"))
    out = {}

    def run(name, args):
        t0 = time.time()
        r = subprocess.run([exe] + args, cwd=d, env=env, capture_output=True, text=True)
        out[name] = {"wall_seconds": time.time() - t0, "returncode": r.returncode,
                     "timing": [ln for ln in r.stdout.splitlines() if ln.startswith("TIMING tiff_lzw")]}
    # the strip TIFF of 4 samples, by the test suite's writer, uncompressed
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _tiff import write_tiff_u16
    write_tiff_u16(os.path.join(d, "M.TIFF"), img.reshape(lines, 6144, 4))
    for rep in range(2):
        run("cog_T256_%d" % rep, ["cog", "M.TIFF", "--tile", "256", "--force"])
        run("cog_T128_%d" % rep, ["cog", "M.TIFF", "--tile", "128", "--force"])
        run("overviews_%d" % rep, ["overviews", "M.TIFF", "--force"])
        run("strip_product_%d" % rep, ["mtfc", "M.TIFF", "--mtf-x", "1", "--mtf-y", "1", "--force"])      # (a 4-sample LZW strip product of the same image)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--cli", default="")
    a = ap.parse_args()
    ctx = oip.Context(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream)
    div = 10 if a.small else 1
    res = {"tool": "cog_bench", "arch": torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]}
    res["pan_12288x60000x1"] = measure(ctx, 12288, 60000 // div, 1, a.reps)
    torch.cuda.empty_cache()
    res["img_6144x60000x4"] = measure(ctx, 6144, 60000 // div, 4, a.reps)
    torch.cuda.empty_cache()
    if a.cli:
        res["cli_6144x%dx4" % (20000 // div)] = cli(a.cli, 20000 // div)
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
