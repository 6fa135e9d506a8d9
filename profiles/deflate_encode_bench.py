"""Times the device Deflate encoder (oip_tiff_deflate_strips_u16) against two yardsticks and prints one JSON line (kept as
profiles/deflate_encode.json and quoted in profiles/deflate_encode.md and DESIGN.md 4.7b).  The sibling of profiles/deflate_bench.py.

    python profiles/deflate_encode_bench.py [--reps 20] [--small] [--cli DIR]

The image is the one of profiles/deflate_bench.py: 6144 x 20000 pixels of 4 samples, 983 MB of noise in [64, 4096), in the same
three layouts: strips of one row, tiles of 128 and tiles of 512 (a tile is passed as a strip of a T-wide image, as the writers do).
  * (a) the host route: the same coder (oip_deflate_stream_host, the host instantiation) on 16 threads over the predictor-2 bytes
    of every stream, wall seconds (the download of the image, which the host route also pays, is not in it);
  * (b) the sibling: oip_tiff_lzw_strips_u16 on the same image and layout, in the same process;
  device events around each device call on the one stream torch and the library share, the two device calls alternating inside
  the timed loop with the host run, medians with the extremes.  Sizes: the encoder's streams beside zlib level 1 and level 6 on the
  same bytes (every stream of the one-row layout is checked to inflate to its bytes).
  * --cli DIR: `oip cog --tiff-compress deflate` (tiles of 128 and of 512) on the image as an uncompressed TIFF in DIR (a scratch
    directory), wall seconds, twice each, with the device route (OIP_TIFF_GPU_DEFLATE=2 so that the route is the device's whatever
    the default is) and with OIP_TIFF_GPU_DEFLATE=0; and `oip overviews --tiff-compress deflate` for the strip layout.
--small: a tenth of the lines (a rehearsal, not a measurement)."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import opticalimageprocessor_amd as oip  # noqa: E402
from deflate_bench import W, SPP, raster, timed  # noqa: E402

THREADS = 16


def summary(v, nbytes):
    s = statistics.median(v)
    return {"seconds_median": s, "seconds_min": min(v), "seconds_max": max(v), "input_GBps": nbytes / s / 1e9}


def host_encode(lib, diff, n, rps, bound):
    """every stream of diff (rows x samples, predictor-2 differences) through the host instantiation on THREADS threads -> (seconds, sizes)"""
    rowbytes = diff.shape[1] * 2
    base = diff.ctypes.data
    outs = [np.empty(bound, np.uint8) for _ in range(THREADS)]
    sizes = np.zeros(n, np.int64)

    def work(t):
        dst = outs[t].ctypes.data
        for k in range(t, n, THREADS):
            sizes[k] = lib.oip_deflate_stream_host(C.c_void_p(base + k * rps * rowbytes), rps * rowbytes, C.c_void_p(dst), bound)
    t0 = time.time()
    with ThreadPoolExecutor(THREADS) as pool:
        list(pool.map(work, range(THREADS)))
    return time.time() - t0, sizes


def layout(ctx, lib, img, L, tile, reps):
    if tile:
        tx, ty = -(-W // tile), -(-L // tile)
        form = torch.empty(tx * ty * tile, tile * SPP, dtype=torch.uint16, device="cuda")
        ctx.retile_u16(img, W * SPP, W, L, SPP, tile, 0, ty, form)
        ctx.sync()
        rows, width, rps = tx * ty * tile, tile, tile
    else:
        form, rows, width, rps = img, L, W, 1
    host = form.view(torch.int16).cpu().numpy().view(np.uint16)
    diff = host.copy()
    diff[:, SPP:] -= host[:, :-SPP]                                     # predictor 2, modulo 2^16
    n = rows // rps
    stream_bytes = rps * width * SPP * 2
    d_img = form.view(torch.int16)
    d_def = torch.empty(ctx.tiff_deflate_worst_bytes(rows, width, SPP, rps), dtype=torch.uint8, device="cuda")
    d_dsc = torch.empty(ctx.tiff_deflate_scratch_bytes(rows, width, SPP, rps), dtype=torch.uint8, device="cuda")
    d_lzw = torch.empty(ctx.tiff_lzw_worst_bytes(rows, width, SPP, rps), dtype=torch.uint8, device="cuda")
    d_lsc = torch.empty(ctx.tiff_lzw_scratch_bytes(rows, width, SPP, rps), dtype=torch.uint8, device="cuda")
    out = {}
    runs = {"deflate_device": lambda: out.__setitem__("d", ctx.tiff_deflate_strips(d_img, rows, width, SPP, rps, d_def, scratch=d_dsc)),
            "lzw_device": lambda: out.__setitem__("l", ctx.tiff_lzw_strips(d_img, rows, width, SPP, rps, d_lzw, scratch=d_lsc))}
    for fn in runs.values():
        fn()                                                            # warm-up: first touch of the scratch
    off, ln, total = out["d"]
    bound = oip.deflate_stored_bound(stream_bytes)
    t = {k: [] for k in list(runs) + ["deflate_host_16_threads"]}
    sizes = None
    for _ in range(reps):
        for k, fn in runs.items():
            t[k].append(timed(fn))
        s, sizes = host_encode(lib, diff, n, rps, bound)
        t["deflate_host_16_threads"].append(s)
    assert np.array_equal(sizes, np.asarray(out["d"][1], np.int64)), "host and device stream sizes differ"
    pay = d_def.cpu().numpy()
    for k in range(0, n, max(1, n // 64)):                               # a sample of the streams inflates to its bytes
        assert zlib.decompress(pay[int(off[k]):int(off[k] + ln[k])].tobytes()) == diff[k * rps:(k + 1) * rps].tobytes(), k
    with ThreadPoolExecutor(THREADS) as pool:
        z1 = sum(pool.map(lambda k: len(zlib.compress(diff[k * rps:(k + 1) * rps].tobytes(), 1)), range(n)))
        z6 = sum(pool.map(lambda k: len(zlib.compress(diff[k * rps:(k + 1) * rps].tobytes(), 6)), range(n)))
    res = {"streams": n, "stream_bytes": stream_bytes, "input_bytes": host.nbytes, "deflate_bytes": int(sum(ln)), "lzw_bytes": int(out["l"][2]),
           "zlib_level1_bytes": z1, "zlib_level6_bytes": z6, "reps": reps}
    for k in t:
        res[k] = summary(t[k], host.nbytes)
    res["device_over_host_time"] = res["deflate_device"]["seconds_median"] / res["deflate_host_16_threads"]["seconds_median"]
    res["deflate_over_lzw_time"] = res["deflate_device"]["seconds_median"] / res["lzw_device"]["seconds_median"]
    return res


def cli(img, cli_dir):
    from _tiff import write_tiff_u16
    exe = os.path.join(ROOT, "opticalimageprocessor_amd", "lib", "oip")
    env = dict(os.environ, LOGFILE=os.path.join(cli_dir, "oip.log"))
    host = img.view(torch.int16).cpu().numpy().view(np.uint16)
    write_tiff_u16(os.path.join(cli_dir, "U.TIFF"), host.reshape(host.shape[0], W, SPP))
    res = {}
    for name, args in (("cog_tiles_128", ["cog", "U.TIFF", "-o", "C.TIFF", "--force", "--tile", "128", "--tiff-compress", "deflate"]),
                       ("cog_tiles_512", ["cog", "U.TIFF", "-o", "C.TIFF", "--force", "--tile", "512", "--tiff-compress", "deflate"]),
                       ("overviews_strips", ["overviews", "U.TIFF", "-o", "C.TIFF", "--force", "--tiff-compress", "deflate"])):
        res[name] = {}
        for route, knob in (("device", "2"), ("host_16_threads", "0")):
            res[name][route] = []
            for _ in range(2):
                t0 = time.time()
                r = subprocess.run([exe] + args, cwd=cli_dir, env=dict(env, OIP_TIFF_GPU_DEFLATE=knob), capture_output=True, text=True, timeout=900)
                res[name][route].append(time.time() - t0 if r.returncode == 0 else "failed: " + (r.stdout + r.stderr)[-300:])
    for f in ("U.TIFF", "C.TIFF"):
        if os.path.exists(os.path.join(cli_dir, f)):
            os.remove(os.path.join(cli_dir, f))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--cli", default="")
    a = ap.parse_args()
    ctx = oip.Context(0)
    lib = oip.load_library()
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream)
    L = 20000 // (10 if a.small else 1)
    img = raster(L, W * SPP, 2)
    res = {"tool": "deflate_encode_bench", "arch": torch.cuda.get_device_properties(0).gcnArchName.split(":")[0], "W": W, "lines": L, "spp": SPP,
           "host_threads": THREADS}
    for name, tile in (("strips_of_one_row", 0), ("tiles_128", 128), ("tiles_512", 512)):
        res[name] = layout(ctx, lib, img, L, tile, a.reps)
        torch.cuda.empty_cache()
        print(json.dumps({name: res[name]}), file=sys.stderr, flush=True)
    if a.cli:
        res["cli_wall_seconds"] = cli(img, a.cli)
        print(json.dumps({"cli_wall_seconds": res["cli_wall_seconds"]}), file=sys.stderr, flush=True)
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
