"""Restatement of `oip mtfc` in numpy / plain Python: the fixed-point convolution of include/oip_c.h (oip_convolve_u16) in
int64 with a per-tap loop and padding by index clamping, and the three host functions that make the taps (oip_mtfc_design3,
oip_mtfc_quantise, oip_mtfc_load_kernel) in Python floats, one rounded operation per step in the order the header states."""
import numpy as np


def convolve(img, taps, valid_min=1, spp=1):
    """img: (L, W * spp) uint16, pixel-interleaved; taps: (ky, kx) integers (Q12).  Returns (L, W * spp) uint16."""
    img = np.asarray(img)
    taps = np.asarray(taps, dtype=np.int64)
    L = img.shape[0]
    src = img.reshape(L, -1, spp).astype(np.int64)
    W = src.shape[1]
    ky, kx = taps.shape
    ry, rx = ky // 2, kx // 2
    ys, xs = np.arange(L), np.arange(W)
    acc = np.zeros_like(src)
    for j in range(ky):
        rows = np.clip(ys + j - ry, 0, L - 1)
        for i in range(kx):
            cols = np.clip(xs + i - rx, 0, W - 1)
            n = src[rows][:, cols]                         # tap (j, i) multiplies the sample at offset (j - ry, i - rx)
            n = np.where(n < valid_min, src, n)
            acc += taps[j, i] * n
    out = np.clip((acc + 2048) >> 12, valid_min, 65535)    # >> on int64 is arithmetic: the floor
    out = np.where(src < valid_min, src, out)
    return out.astype(np.uint16).reshape(img.shape)


def design3(mtf_x, mtf_y, max_gain=2.0):
    """(3, 3) float64 coefficients"""
    if not (0.0 < mtf_x <= 1.0 and 0.0 < mtf_y <= 1.0 and max_gain >= 1.0):
        raise ValueError("design3: 0 < mtf <= 1 and max_gain >= 1 expected")
    f = []
    for m in (float(mtf_x), float(mtf_y)):
        g = min(1.0 / m, float(max_gain))
        a = (g - 1.0) / 4.0
        f.append([-a, 1.0 + 2.0 * a, -a])
    fx, fy = f
    return np.array([[fy[j] * fx[i] for i in range(3)] for j in range(3)], dtype=np.float64)


def quantise(c):
    """(ky, kx) coefficients -> (ky, kx) int32 Q12 taps; ValueError as the library refuses"""
    c = np.asarray(c, dtype=np.float64)
    ky, kx = c.shape
    if not (ky % 2 == 1 and kx % 2 == 1 and ky <= 9 and kx <= 9):
        raise ValueError("quantise: odd sizes 1..9 expected")
    t = [int(np.rint(float(v) * 4096.0)) for v in c.ravel()]        # np.rint: ties to even
    s = 0.0
    for v in c.ravel():
        s += float(v)
    if not abs(s - 1.0) <= 1e-6:
        raise ValueError("quantise: the coefficients sum to %r" % s)
    t[(ky // 2) * kx + kx // 2] += 4096 - sum(t)
    if sum(abs(v) for v in t) > 32767:
        raise ValueError("quantise: sum |taps| = %d" % sum(abs(v) for v in t))
    return np.array(t, dtype=np.int32).reshape(ky, kx)


def load_kernel(path):
    tok = open(path).read().split()
    ky, kx = int(tok[0]), int(tok[1])
    if not (ky % 2 == 1 and kx % 2 == 1 and 1 <= ky <= 9 and 1 <= kx <= 9) or len(tok) != 2 + ky * kx:
        raise ValueError("load_kernel: malformed file")
    return np.array([float(v) for v in tok[2:]], dtype=np.float64).reshape(ky, kx)


def write_kernel(path, c):
    c = np.asarray(c, dtype=np.float64)
    with open(path, "w") as f:
        f.write("%d %d\n" % c.shape)
        for row in c:
            f.write(" ".join(repr(float(v)) for v in row) + "\n")


def random_taps(ky, kx, seed, total=32767):
    """signed, asymmetric integer taps with sum |t| == total exactly"""
    rng = np.random.default_rng(seed)
    t = rng.integers(-400, 401, (ky, kx)).astype(np.int64)
    t[t == 0] = 7
    rest = total - int(np.abs(t).sum())
    assert rest > 0
    c = (ky // 2, kx // 2)
    t[c] += rest if t[c] > 0 else -rest
    assert int(np.abs(t).sum()) == total and not np.array_equal(t, t[::-1]) and not np.array_equal(t, t[:, ::-1])
    return t.astype(np.int32)
