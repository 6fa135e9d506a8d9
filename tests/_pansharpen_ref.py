"""numpy restatement of `oip pansharpen` (include/oip_c.h: oip_pansharpen_sfim_u16, oip_pansharpen_geometry): smoothing-filter
intensity modulation, fused_b = up(MSS_b) * PAN / up(low(PAN)).  The up-sampling by 4 is integer arithmetic, the modulation three
IEEE single-precision operations each rounded on its own, so the device is compared with this by equality.

  P   PAN, (Hp, W) u16;  M  MSS product, (h, w, 4) u16;  W = 4 w;  off >= 0 the first PAN line used
  hh = min(h, (Hp - off) // 4) MSS lines are used; the product is (4 hh, 4 w, 4) u16
  Lm  = (sum of the 4 x 4 PAN block + 8) >> 4                                                      (hh, w)
  up  : cell i = x >> 2, phase r = x & 3, first tap c0 = i - 2 (r < 2) or i - 1, taps clamp(c0 + k, 0, n - 1), weights WEIGHTS[r]
        Hq = (sum wx s + 128) >> 8 along the lines, then U = clamp((sum wy Hq + 1024) >> 11, 0, 8 * 65535) across them
  g   = 0.125 where U(Lm) == 0, else min(f32(P) / f32(U(Lm)), G * 0.125)
  out = saturate_u16(rint(f32(U(M_b)) * g))
  counters: pixels with U(Lm) == 0, pixels whose quotient was above G * 0.125"""
from fractions import Fraction

import numpy as np

WEIGHTS = np.array([[-135, 873, 1535, -225], [-21, 235, 1981, -147], [-147, 1981, 235, -21], [-225, 1535, 873, -135]], dtype=np.int64)
PHASES = (Fraction(5, 8), Fraction(7, 8), Fraction(1, 8), Fraction(3, 8))       # the cubic's t of phase r; its first tap is floor - 1
U_MAX = 8 * 65535


def cubic_weights(t, a=Fraction(-3, 4)):
    """OpenCV's interpolateCubic at t, exact"""
    t = Fraction(t)
    c0 = ((a * (t + 1) - 5 * a) * (t + 1) + 8 * a) * (t + 1) - 4 * a
    c1 = ((a + 2) * t - (a + 3)) * t * t + 1
    c2 = ((a + 2) * (1 - t) - (a + 3)) * (1 - t) * (1 - t) + 1
    return [c0, c1, c2, 1 - c0 - c1 - c2]


def axis(n, x0, count):
    """tap indices (count, 4) into an axis of n cells and weights (count, 4) of output coordinates x0 .. x0 + count - 1"""
    x = np.arange(x0, x0 + count, dtype=np.int64)
    i, r = x >> 2, x & 3
    c0 = np.where(r < 2, i - 2, i - 1)
    return np.clip(c0[:, None] + np.arange(4), 0, n - 1), WEIGHTS[r]


def upsample(src, y0=0, rows=None, h=None, src_row0=0, extremes=False):
    """U (rows, 4 w) int64 of output lines [y0, y0 + rows) of the (h, w) raster whose lines src_row0 .. are `src`; extremes: also
    max |Hq| and the largest |sum| + 1024 of the pass across the lines"""
    src = np.asarray(src).astype(np.int64)
    h = src.shape[0] + src_row0 if h is None else h
    rows = 4 * h - y0 if rows is None else rows
    w = src.shape[1]
    ix, wx = axis(w, 0, 4 * w)
    iy, wy = axis(h, y0, rows)
    lo, hi = int(iy.min()), int(iy.max())
    s = src[lo - src_row0:hi + 1 - src_row0]
    assert s.shape[0] == hi + 1 - lo, "upsample: source lines %d .. %d needed" % (lo, hi)
    hq = ((s[:, ix] * wx[None]).sum(axis=2) + 128) >> 8                      # (lines, 4 w)
    acc = np.zeros((rows, 4 * w), np.int64)
    for k in range(4):
        acc += wy[:, k, None] * hq[iy[:, k] - lo]
    assert np.abs(acc).max(initial=0) + 1024 < 2 ** 31 and np.abs(hq).max(initial=0) < 2 ** 23
    u = np.clip((acc + 1024) >> 11, 0, U_MAX)
    return (u, int(np.abs(hq).max()), int(np.abs(acc).max()) + 1024) if extremes else u


def box4(P):
    """(S + 8) >> 4 of the 4 x 4 blocks of P (lines and columns multiples of 4)"""
    H, W = P.shape
    return (P.astype(np.int64).reshape(H // 4, 4, W // 4, 4).sum(axis=(1, 3)) + 8) >> 4


def geometry(W, Hp, w, h, off=0):
    """(out_w, out_h, mss_lines), or None where oip_pansharpen_geometry refuses"""
    if w < 1 or h < 1 or W != 4 * w or off < 0 or Hp - off < 4:
        return None
    hh = min(h, (Hp - off) // 4)
    return 4 * w, 4 * hh, hh


def modulate(pan, UL, UM, G=4):
    """pan, UL (n, 4 w); UM (n, 4 w, 4): the product's lines (n, 4 w, 4) u16 and the two counters"""
    p, ul = pan.astype(np.float32), UL.astype(np.float32)
    zero = UL == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        q = p / ul                                                            # one IEEE division
    gmax = np.float32(G) * np.float32(0.125)
    cut = ~zero & (q > gmax)
    g = np.where(zero, np.float32(0.125), np.minimum(q, gmax)).astype(np.float32)
    v = np.rint(UM.astype(np.float32) * g[:, :, None])                        # one IEEE product, ties to even
    return np.clip(v, 0, 65535).astype(np.uint16), (int(zero.sum()), int(cut.sum()))


def fuse_window(pan_lines, M, Lm, y0, h, m_row0=0, G=4):
    """output lines [y0, y0 + n) of the kernel: pan_lines (n, 4 w) the PAN lines under them; M (lines, w, 4) and Lm (lines, w) the
    low-resolution rasters from line m_row0 on, of h lines in all"""
    n = pan_lines.shape[0]
    UL = upsample(Lm, y0, n, h, m_row0)
    UM = np.stack([upsample(M[:, :, b], y0, n, h, m_row0) for b in range(4)], axis=2)
    return modulate(pan_lines, UL, UM, G)


def fuse(P, M, off=0, G=4, out_row0=0, out_rows=None):
    """the product of `oip pansharpen` (4 hh, 4 w, 4), or its lines [out_row0, out_row0 + out_rows), and (zero, cut)"""
    h, w, _ = M.shape
    _, oh, hh = geometry(P.shape[1], P.shape[0], w, h, off)
    Pu = P[off:off + oh]
    out_rows = oh - out_row0 if out_rows is None else out_rows
    return fuse_window(Pu[out_row0:out_row0 + out_rows], M[:hh], box4(Pu), out_row0, hh, 0, G)


def plain(M):
    """rint(U_b / 8): the up-sampling alone (what a zero low-resolution PAN gives)"""
    UM = np.stack([upsample(M[:, :, b]) for b in range(4)], axis=2)
    return np.clip(np.rint(UM.astype(np.float32) * np.float32(0.125)), 0, 65535).astype(np.uint16)


def scene(h, w, seed):
    """(T (4h, 4w, 4) float, PAN (4h, 4w) u16, MSS (h, w, 4) u16) of the quality condition"""
    rng = np.random.default_rng(seed)
    S = rng.standard_normal((4 * h + 24, 4 * w + 24))
    for ax in (0, 1):
        for _ in range(2):
            S = np.apply_along_axis(lambda v: np.convolve(v, np.ones(3) / 3, mode="same"), ax, S)
    S = S[12:-12, 12:-12]
    S = (S - S.mean()) / S.std()
    T = np.stack([np.clip(1800 + 300 * b + (500 + 60 * b) * S, 0, 4095) for b in range(4)], axis=2)
    P = np.rint(T.mean(axis=2)).astype(np.uint16)
    M = np.rint(T.reshape(h, 4, w, 4, 4).mean(axis=(1, 3))).astype(np.uint16)
    return T, P, M
