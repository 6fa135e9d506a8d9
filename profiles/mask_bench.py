"""Times oip_mask_cells_u16 against its yardstick, oip_noise_blocks_u16 (spp 4, block 8: a read-only pass over the same bytes with
more arithmetic per sample), and the kernels of oip_mask_morph_u8 at open 1, buffer 2, on the same HBM-resident raster in one
process, and prints one JSON line (quoted in profiles/mask_speed.md and DESIGN.md 4.2e).

    python profiles/mask_bench.py [--width 6144] [--lines 60000] [--reps 20]

The context's own profiler (oip_profile_*: device events around each launch) gives the times; the kernels alternate inside the
timed loop, one profiler reading per repetition, medians are reported.  Bytes are what the algorithm needs: 2 B per sample read
(the flag bytes are 1/512 of that at cell 8 and are left out).  The raster is WIDTH pixels of 4 samples by LINES lines; the other
cell sizes and the spp 1 view of the same bytes ride along."""
import argparse
import json
import os
import statistics
import sys

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
    keys = torch.zeros(4 * (w // 8) * (L // 8), dtype=torch.int16, device="cuda")
    flags = torch.zeros(-(-ws // 4) * -(-L // 4), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
    gw8, gh8 = -(-w // 8), -(-L // 8)
    runs = {"noise_spp4_b8": lambda: ctx.noise_blocks_u16(img, ws, w, L, 4, 8, 4, keys, w // 8, (w // 8) * (L // 8))}
    for name, spp, C in (("mask_spp4_c8", 4, 8), ("mask_spp4_c4", 4, 4), ("mask_spp4_c16", 4, 16), ("mask_spp1_c8", 1, 8)):
        px = ws // spp
        runs[name] = lambda px=px, spp=spp, C=C: ctx.mask_cells_u16(img, ws, px, L, spp, C, flags, -(-px // C), cnt)

    def morph():                                                       # the flags of the cell 8 pass, opened and buffered
        ctx.mask_cells_u16(img, ws, w, L, 4, 8, flags, gw8, cnt)
        ctx.mask_morph_u8(flags, gw8, gw8, gh8, 1, 2, cnt)
    runs["morph_c8_open1_buffer2"] = morph
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
                if k.startswith("morph") and kernel.startswith("mask_cells"):
                    continue
                t.setdefault(k + ":" + kernel, []).append(ms * 1e-3)
    ctx.profile_enable(False)
    nbytes = 2 * ws * L
    res = {"tool": "mask_bench", "arch": torch.cuda.get_device_properties(0).gcnArchName.split(":")[0], "width": w, "lines": L, "spp": 4, "reps": a.reps,
           "bytes_read": nbytes, "cells_c8": gw8 * gh8}
    for k, v in t.items():
        s = statistics.median(v)
        res[k] = {"seconds_median": s, "seconds_min": min(v), "seconds_max": max(v)}
        if not k.startswith("morph"):
            res[k].update({"GBps": nbytes / s / 1e9, "fraction_of_8TBps_peak": nbytes / s / HBM_PEAK})
    yard = res["noise_spp4_b8:noise_blocks_u16_kernel"]["seconds_median"]
    for k in t:
        if k.startswith("mask_"):
            res[k]["time_over_noise"] = res[k]["seconds_median"] / yard
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
