"""Times the two kernels of `oip wallis` against their yardsticks on the same HBM-resident raster in one process, and prints one
JSON line (quoted in profiles/wallis_speed.md and DESIGN.md 4.2f):

  oip_block_moments_u16 (B 128)   against  oip_noise_blocks_u16 (spp 4, block 8): a read-only pass over the same bytes that also
                                            forms a sum and a 64-bit sum of squares per sample
  oip_wallis_apply_u16 (B 128)    against  oip_rrc_u16 on the same raster: the same 2 B in and 2 B out per sample, with fp64
                                            arithmetic where the Wallis transform has integers

    python profiles/wallis_bench.py [--width 6144] [--lines 60000] [--reps 20]

The context's own profiler (oip_profile_*: device events around each launch) gives the times; the kernels alternate inside the
timed loop, one profiler reading per repetition, medians are reported.  Bytes are what the algorithm needs: 2 B per sample read
for the moments (the planes are 1/10000 of that at B 128), 2 B read and 2 B written for the transform.  The raster is WIDTH
pixels of 4 samples by LINES lines; the spp 1 view of the same bytes, block 32 and, for the moments, block 256 (two waves per
block) ride along."""
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


def raster(lines, ws, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    out = torch.empty(lines, ws, dtype=torch.uint16, device="cuda")
    for r in range(0, lines, 4096):
        m = min(4096, lines - r)
        out[r:r + m] = torch.randint(64, 4096, (m, ws), device="cuda", generator=g, dtype=torch.int32).to(torch.int16).view(torch.uint16)
    return out


def nodes(gh, gw, spp, seed):
    rng = np.random.default_rng(seed)
    G = rng.integers(49152, 98304, (gh, gw, spp)).astype(np.int32)     # gains 0.75 .. 1.5
    O = rng.integers(-200 * 256, 200 * 256, (gh, gw, spp)).astype(np.int32)
    return torch.from_numpy(G).cuda(), torch.from_numpy(O).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=6144)
    ap.add_argument("--lines", type=int, default=60000)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    ctx = oip.Context(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream)
    w, L, ws = a.width, a.lines, 4 * a.width
    img = raster(L, ws, 1)
    out = torch.empty_like(img)
    keys = torch.zeros(4 * (w // 8) * (L // 8), dtype=torch.int16, device="cuda")
    acc = torch.zeros(12 * -(-ws // 32) * -(-L // 32), dtype=torch.int64, device="cuda")
    st = torch.zeros(3, dtype=torch.int64, device="cuda")
    kb = torch.from_numpy(np.stack([np.full(ws, 1.01), np.full(ws, 3.0)], axis=1).copy()).cuda()      # (k, b) per column, fp64
    runs = {"noise_spp4_b8": lambda: ctx.noise_blocks_u16(img, ws, w, L, 4, 8, 4, keys, w // 8, (w // 8) * (L // 8)),
            "rrc": lambda: ctx.rrc_u16(img, out, ws, L, kb)}
    # (spp 4, B 256 is the instantiation whose blocks are two waves that meet in LDS; at B 128 a block is one whole wave)
    for name, spp, B in (("moments_spp4_b128", 4, 128), ("moments_spp4_b32", 4, 32), ("moments_spp4_b256", 4, 256), ("moments_spp1_b128", 1, 128)):
        px = ws // spp
        gw, gh = -(-px // B), -(-L // B)
        runs[name] = lambda px=px, spp=spp, B=B, gw=gw, gh=gh: ctx.block_moments_u16(img, ws, px, L, spp, B, acc, gw, gw * gh)
    for name, spp, B in (("apply_spp4_b128", 4, 128), ("apply_spp4_b32", 4, 32), ("apply_spp1_b128", 1, 128)):
        px = ws // spp
        gw, gh = -(-px // B), -(-L // B)
        G, O = nodes(gh, gw, spp, B + spp)
        runs[name] = lambda px=px, spp=spp, B=B, gw=gw, gh=gh, G=G, O=O: ctx.wallis_apply_u16(img, out, 0, L, px, L, spp, B, G, O, gw, gh, 1, 65535, 4095, st)
    for _ in range(3):
        for fn in runs.values():
            fn()
    ctx.sync()
    ctx.profile_enable(True)
    t = {}
    for _ in range(a.reps):
        for k, fn in runs.items():
            ctx.profile_reset()
            fn()
            ctx.sync()
            for kernel, (ms, launches) in ctx.profile().items():
                t.setdefault(k + ":" + kernel, []).append(ms * 1e-3)
    ctx.profile_enable(False)
    nbytes = 2 * ws * L
    res = {"tool": "wallis_bench", "arch": torch.cuda.get_device_properties(0).gcnArchName.split(":")[0], "width": w, "lines": L, "spp": 4, "reps": a.reps,
           "bytes_read": nbytes}
    for k, v in t.items():
        s = statistics.median(v)
        moved = nbytes * (2 if k.startswith(("apply", "rrc")) else 1)
        res[k] = {"seconds_median": s, "seconds_min": min(v), "seconds_max": max(v), "bytes": moved, "GBps": moved / s / 1e9,
                  "fraction_of_8TBps_peak": moved / s / HBM_PEAK}
    yard_m = [v for k, v in res.items() if k.startswith("noise_spp4_b8:")][0]["seconds_median"]
    yard_a = [v for k, v in res.items() if k.startswith("rrc:")][0]["seconds_median"]
    for k in t:
        if k.startswith("moments_"):
            res[k]["time_over_noise"] = res[k]["seconds_median"] / yard_m
        if k.startswith("apply_"):
            res[k]["time_over_rrc"] = res[k]["seconds_median"] / yard_a
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
