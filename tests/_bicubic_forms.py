"""Inputs, cases and runs shared by tests/golden/make_bicubic_forms.py (records the hashes) and
tests/test_gpu_bicubic_golden.py (checks them): every form of the 8-pixels-per-lane bicubic kernels -- the plain call, the
window call with aligned and with scalar stores, RRC on load, each in f32 and in fp16 accumulate -- and one inter-band
align on the fast path.  Only SHA-256 digests are kept; nothing here needs the oracle."""
import functools
import hashlib

import numpy as np

# three LDS blocks of 254 x 8 columns across the line, section seams every 300 lines with both cuts (dy of either sign), and
# at 32 lines per block a last block of 11 lines that ends in lines outside a quad
W, L, SECTION_ROWS, ROW_GUARD = 4096, 1003, 300, 400
SEED = 20250
SHIFTS = [(1.51563, -1.62), (2.37, 1.4), (-2.25, 4.5)]
FOLDS = [100, 37]           # 16-byte stores aligned / pitch 2 (W - 37) not a multiple of 8: the scalar store tail


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def shift_groups(dx):
    """remap.hip's shift_group_regular for every 8-column group: first tap column, x phase, regular flag"""
    x = np.arange(W, dtype=np.float64)
    mapx = (x + dx).astype(np.float32)
    sx = np.rint(mapx * np.float32(32.0)).astype(np.int64)
    ix = (np.clip(sx >> 5, -32768, 32767) - 1).reshape(-1, 8)
    fx = (sx & 31).reshape(-1, 8)
    ix0, fx0 = ix[:, 0], fx[:, 0]
    regular = (ix == ix0[:, None] + np.arange(8)).all(1) & (fx == fx0[:, None]).all(1) & (ix0 >= 0) & (ix0 + 11 < W)
    return ix0, fx0, regular


def check_shift_properties():
    """what the three shifts were chosen for; asserted where the fixture is recorded"""
    n = W // 8
    ix0, _, reg = shift_groups(SHIFTS[0][0])
    bad = set(np.flatnonzero(~reg).tolist())
    assert (ix0[reg] % 2 == 0).all(), "shift 0: even first tap column"
    assert n - 1 in bad and any(0 < g < n - 1 for g in bad), ("shift 0: right border group and an interior group irregular", bad)
    ix0, _, reg = shift_groups(SHIFTS[1][0])
    assert (ix0[reg] % 2 == 1).all(), "shift 1: odd first tap column"
    _, _, reg = shift_groups(SHIFTS[2][0])
    assert not reg[0], "shift 2: left border group irregular"
    for dx, _ in SHIFTS:
        assert shift_groups(dx)[2].sum() > n - 8, "nearly every group takes the fast kernel"


def align_case():
    """the smallest shape of test_gpu_resample.ALIGN_CASES (by pixels) that takes align_mss8_kernel: even width >= 16"""
    from test_gpu_resample import ALIGN_CASES
    return min((c for c in ALIGN_CASES if c[0] % 2 == 0 and c[0] >= 16), key=lambda c: c[0] * c[1])


@functools.lru_cache(maxsize=None)
def inputs():
    """name -> array, generated once per process"""
    from test_gpu_resample import _coef, _rng, _scene
    rng = np.random.default_rng(SEED)
    src = rng.integers(0, 4096, (L, W), dtype=np.uint16)
    # the (k, b) recipe of test_remap_window_equals_remap_then_stitch: 12-bit data onto other 12-bit data
    kb = np.stack([np.full(W, 1.0), np.zeros(W)], 1)
    kb[:, 0] += rng.integers(-3, 4, W) / 64.0
    kb[:, 1] = rng.integers(-8, 9, W) / 4.0
    raw = rng.integers(16, 3900, (L, W), dtype=np.uint16)
    Wb, Lm, _, _, _, keep, _ = align_case()
    arng = _rng(Wb + Lm + int(keep))
    bands = np.stack([_scene(arng, Lm, Wb) for _ in range(4)], 0)
    cx, cy = _coef(arng, Wb)
    return {"src": src, "kb": kb, "raw": raw, "align_bands": bands, "align_cx": cx, "align_cy": cy}


def input_hashes():
    return {k: sha(v) for k, v in inputs().items()}


def remap_key(shift, f16):
    return "remap dx=%r dy=%r %s" % (shift[0], shift[1], "f16acc" if f16 else "f32")


def run_remap_forms(ctx, shift, f16):
    """form name -> output raster of one (shift, accumulate mode)"""
    import torch
    dx, dy = shift
    inp = inputs()
    src, raw = torch.from_numpy(inp["src"]).cuda(), torch.from_numpy(inp["raw"]).cuda()
    d_kb = ctx.upload_kb(inp["kb"])
    out = {}
    plain = torch.zeros(L, W, dtype=torch.uint16, device="cuda")
    ctx.remap_shift_bicubic_u16(src, plain, W, L, dx, dy, SECTION_ROWS, ROW_GUARD, f16acc=f16)
    out["plain"] = plain
    for fold in FOLDS:
        P = 2 * (W - fold)
        win = torch.zeros(L, P, dtype=torch.uint16, device="cuda")
        ctx.remap_shift_bicubic_u16_window(src, win, P, fold, W - fold, W, L, dx, dy, SECTION_ROWS, ROW_GUARD, f16acc=f16)
        out["window fold=%d" % fold] = win
        rrc = torch.zeros(L, P, dtype=torch.uint16, device="cuda")
        ctx.remap_shift_rrc_bicubic_u16_window(raw, d_kb, rrc, P, fold, W - fold, W, L, dx, dy, SECTION_ROWS, ROW_GUARD, f16acc=f16)
        out["rrc window fold=%d" % fold] = rrc
    ctx.sync()
    return {k: v.cpu().numpy() for k, v in out.items()}


def run_align(ctx):
    import torch
    Wb, Lm, lps, off, ovl, keep, minl = align_case()
    inp = inputs()
    planes = torch.from_numpy(inp["align_bands"]).cuda()
    rows = Lm - off - (0 if keep else ovl)
    dst = torch.full((rows, Wb, 4), 7, dtype=torch.uint16, device="cuda")
    ctx.align_mss_bicubic_u16x4(planes, Wb * Lm, dst, Wb, Lm, inp["align_cx"], inp["align_cy"], lps, off, ovl, keep, minl)
    ctx.sync()
    return dst.cpu().numpy()
