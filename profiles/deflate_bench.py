"""Times the device Deflate decoder (oip_tiff_deflate_decode_u16) against two yardsticks and prints one JSON line (to be kept as
profiles/deflate_kernel.json and quoted in profiles/deflate_speed.md and DESIGN.md 4.7a).

    python profiles/deflate_bench.py [--reps 20] [--small] [--cli DIR]

The image is the one of profiles/cog_speed.md: 6144 x 20000 pixels of 4 samples, 983 MB of noise in [64, 4096).  It is compressed
on the spot with zlib level 6 and predictor 2 (16 threads) in three layouts: strips of one row, tiles of 128 and tiles of 512 (a
tile is passed as a strip of a T-wide image, as the reader passes it).
  * the sibling: oip_tiff_lzw_decode_u16 on the LZW encoding (the device encoder's) of the same image and layout, in the same
    process: device events around each call on the one stream torch and the library share, the two calls alternating inside the
    timed loop, medians with the extremes;
  * --cli DIR: the host route.  The Deflate and the LZW file of every layout are written into DIR (a scratch directory) and
    `oip quicklook` runs on them: the Deflate file with the device decoder, the same file with OIP_TIFF_GPU_DEFLATE=0 (the 16
    worker threads of the host reader, then the upload), and the LZW file; wall seconds of each, twice.  read_tiff_to_device
    is the tools' own loader and has no binding, so this yardstick is process wall time of two runs, not device events.
--small: a tenth of the lines (a rehearsal, not a measurement)."""
import argparse
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
import _deflate_tiff as T  # noqa: E402

W, SPP = 6144, 4


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
    return {"seconds_median": s, "seconds_min": min(v), "seconds_max": max(v), "decoded_GBps": nbytes / s / 1e9}


def pack(streams):
    off, pos = [], 0
    for s in streams:
        pos += pos & 1
        off.append(pos)
        pos += len(s)
    blob = np.zeros(pos + 16, np.uint8)
    for o, s in zip(off, streams):
        blob[o:o + len(s)] = np.frombuffer(s, np.uint8)
    return blob, off, [len(s) for s in streams]


def layout(ctx, img, L, tile, reps, cli_dir):
    """img: the L x (W * SPP) raster on the device.  tile 0: strips of one row."""
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
    t0 = time.time()
    with ThreadPoolExecutor(16) as pool:
        streams = list(pool.map(lambda k: zlib.compress(diff[k * rps:(k + 1) * rps].tobytes(), 6), range(n)))
    t_compress = time.time() - t0
    blob, off, ln = pack(streams)
    d_file = torch.from_numpy(blob).cuda()
    d_pay = torch.empty(ctx.tiff_lzw_worst_bytes(rows, width, SPP, rps), dtype=torch.uint8, device="cuda")
    loff, lln, ltotal = ctx.tiff_lzw_strips(form.view(torch.int16), rows, width, SPP, rps, d_pay)
    back = torch.zeros(rows, width * SPP, dtype=torch.int16, device="cuda")
    runs = {"deflate_decode": lambda: ctx.tiff_deflate_decode(d_file, off, ln, rows, width, SPP, rps, 2, back),
            "lzw_decode": lambda: ctx.tiff_lzw_decode(d_pay, loff, lln, rows, width, SPP, rps, 2, back)}
    for k, fn in runs.items():
        back.zero_()
        fn()
        assert torch.equal(back, form.view(torch.int16)), k
    t = {k: [] for k in runs}
    for _ in range(reps):
        for k, fn in runs.items():
            t[k].append(timed(fn))
    res = {"streams": n, "stream_bytes": rps * width * SPP * 2, "decoded_bytes": host.nbytes, "deflate_bytes": int(sum(ln)), "lzw_bytes": int(ltotal),
           "zlib_level6_seconds_16_threads": t_compress, "reps": reps}
    for k in runs:
        res[k] = summary(t[k], host.nbytes)
    res["deflate_over_lzw_time"] = res["deflate_decode"]["seconds_median"] / res["lzw_decode"]["seconds_median"]
    if cli_dir:
        exe = os.path.join(ROOT, "opticalimageprocessor_amd", "lib", "oip")
        env = dict(os.environ, LOGFILE=os.path.join(cli_dir, "oip.log"))
        img_host = img.view(torch.int16).cpu().numpy().view(np.uint16)
        kw = {"tile": (tile, tile)} if tile else {"rps": 1}
        pay = d_pay.cpu().numpy()
        T.write(os.path.join(cli_dir, "D.TIFF"), img_host, SPP, 2, streams=streams, **kw)
        T.write(os.path.join(cli_dir, "Z.TIFF"), img_host, SPP, 2, compression=5, streams=[pay[int(o):int(o + m)].tobytes() for o, m in zip(loff, lln)], **kw)
        cli = res["quicklook_wall_seconds"] = {}
        for name, src, extra in (("deflate_device", "D.TIFF", {}), ("deflate_host_16_threads", "D.TIFF", {"OIP_TIFF_GPU_DEFLATE": "0"}), ("lzw_device", "Z.TIFF", {})):
            cli[name] = []
            for _ in range(2):
                t0 = time.time()
                r = subprocess.run([exe, "quicklook", src, "-o", "ql.TIFF", "--force"], cwd=cli_dir, env=dict(env, **extra), capture_output=True, text=True, timeout=600)
                cli[name].append(time.time() - t0 if r.returncode == 0 else "failed: " + (r.stdout + r.stderr)[-300:])
        for f in ("D.TIFF", "Z.TIFF", "ql.TIFF"):
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
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream)
    L = 20000 // (10 if a.small else 1)
    img = raster(L, W * SPP, 2)
    res = {"tool": "deflate_bench", "arch": torch.cuda.get_device_properties(0).gcnArchName.split(":")[0], "W": W, "lines": L, "spp": SPP}
    for name, tile in (("strips_of_one_row", 0), ("tiles_128", 128), ("tiles_512", 512)):
        res[name] = layout(ctx, img, L, tile, a.reps, a.cli)
        torch.cuda.empty_cache()
        print(json.dumps({name: res[name]}), file=sys.stderr, flush=True)
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
