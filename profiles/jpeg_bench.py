"""Times the device JPEG coder (oip_jpeg_scan_u8) and prints one JSON line (kept as profiles/jpeg_speed.json and quoted in
profiles/jpeg_speed.md, DESIGN.md and the README).  The sibling of profiles/deflate_encode_bench.py.

    python profiles/jpeg_bench.py [--reps 10] [--small] [--cli DIR]

Two browse images at quality 90, a smooth scene with noise of sigma 4 made on the device: 15000 x 50000 RGB (what --factor 2 makes
of a 30000 x 100000 strip, 2.25 GB) and 1875 x 6250 grey (--factor 16, 11.7 MB).
  * the scan: device events around the call on the one stream torch and the library share, medians with the extremes; GB/s of
    input; the share of the HBM peak taken over the bytes the call must move (the image read twice, once per pass, and the payload
    written once); the library's own profile of the two passes; and the cycles the storing pass's waves spent in the coder's five
    phases (the counters in the last 40 bytes of the scratch, include/oip_c.h), which says whether the prefix sum over the bit
    counts (counting and placing) or the one over the 0xFF flags (stuffing) dominates;
  * the yardstick: Pillow's libjpeg on the same arrays on the host, save(quality=90, subsampling=0, restart_marker_rows=1) of
    strips of lines on 16 threads (libjpeg has no threads of its own), wall seconds, and one thread on the grey image;
  * --cli DIR: `oip quicklook --factor 2` of a 6144 x 40000 RAW strip written to DIR (a scratch directory) with --format jpeg
    against --format tiff, wall seconds, twice each.
--small: a tenth of the lines of the large image (a rehearsal, not a measurement)."""
import argparse
import io
import json
import os
import statistics
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import opticalimageprocessor_amd as oip  # noqa: E402

THREADS = 16
HBM_PEAK = 8.0e12
Q = 90
PHASES = ("stage", "transform", "count_bits_and_prefix_sum", "place_codes", "stuff_and_store")


def scene(h, w, nch, seed):
    """(h, w * nch) uint8 on the device, made in blocks of lines"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    out = torch.empty(h, w * nch, dtype=torch.uint8, device="cuda")
    x = torch.arange(w, device="cuda", dtype=torch.float32)
    for r in range(0, h, 2048):
        m = min(2048, h - r)
        y = torch.arange(r, r + m, device="cuda", dtype=torch.float32)[:, None]
        base = 128 + 70 * torch.sin(x / 23.0)[None, :] * torch.cos(y / 31.0) + 30 * torch.sin((x[None, :] + y) / 7.0)
        if nch == 3:
            base = torch.stack([base, torch.roll(base, 11, 1), 255 - base], -1).reshape(m, w * 3)
        out[r:r + m] = (base + 4 * torch.randn(m, w * nch, device="cuda", generator=g)).round_().clamp_(0, 255).to(torch.uint8)
    return out


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def pillow(host, nch, threads):
    """the image in `threads` strips of whole 8-line rows through libjpeg -> (seconds, bytes)"""
    from PIL import Image
    h = host.shape[0]
    step = -(-h // threads + 7) // 8 * 8 if threads > 1 else h
    parts = [host[r:r + step] for r in range(0, h, step)]

    def work(a):
        b = io.BytesIO()
        Image.fromarray(a if nch == 1 else a.reshape(a.shape[0], -1, 3)).save(b, "JPEG", quality=Q, subsampling=0, restart_marker_rows=1)
        return b.tell()
    t0 = time.time()
    with ThreadPoolExecutor(threads) as pool:
        sizes = list(pool.map(work, parts))
    return time.time() - t0, sum(sizes)


def image(ctx, name, w, h, nch, reps, host_threads):
    img = scene(h, w, nch, 7)
    payload = torch.empty(ctx.jpeg_worst_bytes(w, h, nch), dtype=torch.uint8, device="cuda")
    scratch = torch.zeros(ctx.jpeg_scratch_bytes(w, h, nch), dtype=torch.uint8, device="cuda")
    out = {}
    run = lambda: out.__setitem__("r", ctx.jpeg_scan(img, w * nch, w, h, nch, Q, payload, scratch=scratch))  # noqa: E731
    run()                                                                   # warm-up: code object, first touch of the payload
    run()
    t = [timed(run) for _ in range(reps)]
    total = out["r"][2]
    cycles = scratch[-40:].cpu().numpy().view(np.uint64).astype(np.float64)
    ctx.profile_reset()
    ctx.profile_enable(True)
    for _ in range(3):
        run()
    prof = {k: v[0] / v[1] * 1e-3 for k, v in ctx.profile().items() if k.startswith("jpeg_")}
    ctx.profile_enable(False)
    s = statistics.median(t)
    nbytes = img.numel()
    res = {"w": w, "h": h, "nch": nch, "quality": Q, "input_bytes": nbytes, "payload_bytes": total, "payload_capacity_bytes": payload.numel(),
           "seconds_median": s, "seconds_min": min(t), "seconds_max": max(t), "reps": reps, "input_GBps": nbytes / s / 1e9,
           "bytes_moved": 2 * nbytes + total, "fraction_of_8TBps_peak": (2 * nbytes + total) / s / HBM_PEAK,
           "kernel_seconds": prof, "phase_share_of_storing_pass": dict(zip(PHASES, (cycles / cycles.sum()).round(4).tolist()))}
    host = img.cpu().numpy()
    del img, payload
    torch.cuda.empty_cache()
    res["pillow"] = {}
    for n in host_threads:
        sec, size = pillow(host, nch, n)
        res["pillow"]["%d_threads" % n] = {"seconds": sec, "bytes": size, "input_GBps": nbytes / sec / 1e9, "device_speedup": sec / s}
    print(json.dumps({name: res}), file=sys.stderr, flush=True)
    return res


def cli(cli_dir, small):
    """`oip quicklook --factor 2` of a 6144 x 40000 RAW strip (492 MB; browse image 3072 x 20000 grey), jpeg against tiff"""
    exe = os.path.join(ROOT, "opticalimageprocessor_amd", "lib", "oip")
    env = dict(os.environ, LOGFILE=os.path.join(cli_dir, "oip.log"))
    W, L = 6144, 40000 // (10 if small else 1)
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    strip = (scene(L, W, 1, 9).to(torch.int32) * 12 + torch.randint(64, 96, (L, W), device="cuda", generator=g, dtype=torch.int32)).to(torch.int16)
    strip.cpu().numpy().view(np.uint16).tofile(os.path.join(cli_dir, "S.RAW"))
    res = {"strip": [W, L]}
    for fmt in ("tiff", "jpeg"):
        res[fmt] = []
        for _ in range(2):
            t0 = time.time()
            r = subprocess.run([exe, "quicklook", "S.RAW", "--width", str(W), "--factor", "2", "--format", fmt, "-o", "B." + fmt, "--force"],
                               cwd=cli_dir, env=env, capture_output=True, text=True, timeout=600)
            res[fmt].append(time.time() - t0 if r.returncode == 0 else "failed: " + (r.stdout + r.stderr)[-300:])
        res[fmt + "_bytes"] = os.path.getsize(os.path.join(cli_dir, "B." + fmt)) if os.path.exists(os.path.join(cli_dir, "B." + fmt)) else 0
    for f in ("S.RAW", "B.tiff", "B.jpeg"):
        if os.path.exists(os.path.join(cli_dir, f)):
            os.remove(os.path.join(cli_dir, f))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--cli", default="")
    a = ap.parse_args()
    ctx = oip.Context(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream)
    res = {"tool": "jpeg_bench", "arch": torch.cuda.get_device_properties(0).gcnArchName.split(":")[0], "host_threads": THREADS}
    res["grey_1875x6250"] = image(ctx, "grey_1875x6250", 1875, 6250, 1, a.reps, (1, THREADS))
    res["rgb_15000x50000"] = image(ctx, "rgb_15000x50000", 15000, 50000 // (10 if a.small else 1), 3, a.reps, (THREADS,))
    if a.cli:
        res["cli_wall_seconds"] = cli(a.cli, a.small)
        print(json.dumps({"cli_wall_seconds": res["cli_wall_seconds"]}), file=sys.stderr, flush=True)
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
