"""The definition of `oip regcheck` (include/oip_c.h: oip_match_tiles_u16, oip_match_grid, oip_match_peak, oip_match_summary)
restated in numpy with int64 sums, and the seeded textures its tests share.  No GPU library is imported.

Plane A is the reference image, plane B the sensed one, both uint16 and of the same w x rows.  A tile has its T x T template
at (ty, tx) in A; for every offset (dy, dx) in [-S, S]^2 it is compared with B's window at (ty + dy, tx + dx):

    sa, saa            sum of a and a^2 over the template            (once per tile)
    sb, sbb, sab       sum of b, b^2 and a b over the window         (per offset)
    bad_a, bad_b       samples outside [valid_min, valid_max] in the template / in B's whole (T + 2S)^2 search window
    n = T^2;  num = n sab - sa sb;  va = n saa - sa^2;  vb = n sbb - sb^2        (all exact in int64)
    score = num / sqrt(float(va) * float(vb)),  no score (-2) where va <= 0 or vb <= 0

The peak is the largest score, the first in row-major order (dy, then dx) among equal ones; where no offset has a score it is
the offset (0, 0).  A record is 20 uint64: sa, saa, bad_a, bad_b, the peak index (dy + S) (2S + 1) + (dx + S), then
(sb, sbb, sab) at the peak and at its left (dx - 1), right (dx + 1), upper (dy - 1) and lower (dy + 1) neighbour, three zeros
for a neighbour outside the range.  (dx, dy) is where A's template is found in B, relative to its own position."""
import numpy as np

NODATA, FLAT, EDGE, WEAK = 1, 2, 4, 8
RECORD_WORDS = 20
NO_SCORE = -2.0


def grid(w, rows, T, S, step):
    """(x0, y0, nx, ny): the tiles at x0 + i step, y0 + j step whose search windows lie inside w x rows; nx = ny = 0 if none"""
    nx = (w - 2 * S - T) // step + 1 if w >= T + 2 * S else 0
    ny = (rows - 2 * S - T) // step + 1 if rows >= T + 2 * S else 0
    if nx <= 0 or ny <= 0:
        return S, S, 0, 0
    return S, S, nx, ny


def tile_sums(A, B, ty, tx, T, S, valid_min=1, valid_max=65535):
    """-> (sa, saa, bad_a, bad_b, sums (2S + 1, 2S + 1, 3) int64)"""
    assert ty - S >= 0 and tx - S >= 0 and ty + T + S <= A.shape[0] and tx + T + S <= A.shape[1] and A.shape == B.shape
    a = A[ty:ty + T, tx:tx + T].astype(np.int64)
    win = B[ty - S:ty + T + S, tx - S:tx + T + S].astype(np.int64)
    bad_a = int(((a < valid_min) | (a > valid_max)).sum())
    bad_b = int(((win < valid_min) | (win > valid_max)).sum())
    K = 2 * S + 1
    sums = np.zeros((K, K, 3), np.int64)
    for j in range(K):
        for i in range(K):
            b = win[j:j + T, i:i + T]
            sums[j, i] = (b.sum(), (b * b).sum(), (a * b).sum())
    return int(a.sum()), int((a * a).sum()), bad_a, bad_b, sums


def scores(sa, saa, sums, T):
    """fp64 score per offset from the integer sums; NO_SCORE where a variance is not positive"""
    n = T * T
    s = sums.astype(np.int64)
    num = n * s[..., 2] - sa * s[..., 0]
    va = n * saa - sa * sa
    vb = n * s[..., 1] - s[..., 0] * s[..., 0]
    ok = (vb > 0) & (va > 0)
    den = np.sqrt(np.float64(va) * vb.astype(np.float64))
    out = np.full(s.shape[:-1], NO_SCORE)
    out[ok] = num[ok].astype(np.float64) / den[ok]
    return out


def peak_index(sc):
    """row-major index of the peak of a (K, K) score table; the centre where nothing has a score"""
    K = sc.shape[0]
    if not (sc > NO_SCORE).any():
        return (K // 2) * K + K // 2
    return int(np.argmax(sc.reshape(-1)))


def record(sa, saa, bad_a, bad_b, sums, T):
    K = sums.shape[0]
    pk = peak_index(scores(sa, saa, sums, T))
    j, i = divmod(pk, K)
    rec = np.zeros(RECORD_WORDS, np.uint64)
    rec[:5] = (sa, saa, bad_a, bad_b, pk)
    for k, (jj, ii) in enumerate(((j, i), (j, i - 1), (j, i + 1), (j - 1, i), (j + 1, i))):
        if 0 <= jj < K and 0 <= ii < K:
            rec[5 + 3 * k:8 + 3 * k] = sums[jj, ii].astype(np.uint64)
    return rec


def match_tiles(A, B, T, S, x0, y0, step_x, step_y, nx, ny, valid_min=1, valid_max=65535):
    """-> (records (ny nx, 20) uint64, sums (ny nx, (2S + 1)^2, 3) uint64, gap (ny nx,): best minus second-best score)"""
    K = 2 * S + 1
    recs = np.zeros((ny * nx, RECORD_WORDS), np.uint64)
    allsums = np.zeros((ny * nx, K * K, 3), np.uint64)
    gap = np.zeros(ny * nx)
    for j in range(ny):
        for i in range(nx):
            sa, saa, ba, bb, sums = tile_sums(A, B, y0 + j * step_y, x0 + i * step_x, T, S, valid_min, valid_max)
            t = j * nx + i
            recs[t] = record(sa, saa, ba, bb, sums, T)
            allsums[t] = sums.reshape(K * K, 3).astype(np.uint64)
            sc = np.sort(scores(sa, saa, sums, T).reshape(-1))
            gap[t] = sc[-1] - sc[-2]
    return recs, allsums, gap


def _subpixel(l, c, r):
    if l <= NO_SCORE or r <= NO_SCORE or c <= NO_SCORE:
        return 0.0
    den = l - 2.0 * c + r
    if not den < 0.0:
        return 0.0
    return float(min(0.5, max(-0.5, (l - r) / (2.0 * den))))


def peak(rec, T, S, min_score=0.5):
    """-> (dx, dy, score, flags) of one record: the integer peak plus, per axis, the vertex of the parabola through the peak and
    its two neighbours, f = (l - r) / (2 (l - 2 c + r)) clamped to +-0.5 -- only where the peak is off the range's border on that
    axis, both neighbours have a score and the denominator is negative; else f = 0"""
    rec = np.asarray(rec, np.uint64).astype(np.int64)
    sa, saa, bad_a, bad_b, pk = (int(v) for v in rec[:5])
    K = 2 * S + 1
    j, i = divmod(pk, K)
    sc = scores(sa, saa, rec[5:20].reshape(5, 3), T)
    c, l, r, u, d = (float(v) for v in sc)
    fx = _subpixel(l, c, r) if 0 < i < K - 1 else 0.0
    fy = _subpixel(u, c, d) if 0 < j < K - 1 else 0.0
    flags = 0
    if bad_a + bad_b > 0:
        flags |= NODATA
    if c <= NO_SCORE:
        flags |= FLAT
    if abs(i - S) == S or abs(j - S) == S:
        flags |= EDGE
    if c < min_score:
        flags |= WEAK
    return (i - S) + fx, (j - S) + fy, c, flags


def summary(dx, dy, flags):
    """over the tiles whose flags are 0: (count, mean dx, mean dy, std dx, std dy (population), RMS of the radial error
    sqrt(dx^2 + dy^2), its nearest-rank 90th percentile (CE90: the ceil(0.9 count)-th smallest), its maximum); zeros if none"""
    dx, dy, flags = np.asarray(dx, np.float64), np.asarray(dy, np.float64), np.asarray(flags)
    ok = flags == 0
    n = int(ok.sum())
    if n == 0:
        return np.zeros(8)
    x, y = dx[ok], dy[ok]
    r = np.sort(np.sqrt(x * x + y * y))
    ce90 = r[(9 * n + 9) // 10 - 1]                              # ceil(0.9 n) in integers
    return np.array([n, x.mean(), y.mean(), x.std(), y.std(), np.sqrt((r * r).mean()), ce90, r[-1]])


# ---- the textures ------------------------------------------------------------------------------------------------------------
def texture(h, w, margin, seed):
    """(h + 2 margin, w + 2 margin) in [0, 1]: seeded normal noise, box-blurred with radius 2 in both directions (a 5 x 5 mean),
    then scaled to its own range"""
    rng = np.random.default_rng(seed)
    H, W = h + 2 * margin, w + 2 * margin
    x = rng.standard_normal((H + 4, W + 4))
    c = np.cumsum(np.pad(x, ((1, 0), (0, 0))), axis=0)
    x = (c[5:] - c[:-5]) / 5.0
    c = np.cumsum(np.pad(x, ((0, 0), (1, 0))), axis=1)
    x = (c[:, 5:] - c[:, :-5]) / 5.0
    assert x.shape == (H, W)
    return (x - x.min()) / (x.max() - x.min())


def pair(h, w, shift, seed, margin=16):
    """A = 200 + 3500 x and B = 100 + 0.7 * 3500 (x shifted by shift = (dx, dy)) + N(0, 8), both (h, w) uint16: A's content at
    (y, x) is found in B at (y + dy, x + dx).  A in [200, 3700], B in about [60, 2600]: no sample is no data."""
    dx, dy = shift
    assert abs(dx) <= margin and abs(dy) <= margin
    x = texture(h, w, margin, seed)
    rng = np.random.default_rng(seed + 7919)
    A = 200.0 + 3500.0 * x[margin:margin + h, margin:margin + w]
    B = 100.0 + 0.7 * 3500.0 * x[margin - dy:margin - dy + h, margin - dx:margin - dx + w] + rng.normal(0.0, 8.0, (h, w))
    return np.rint(A).astype(np.uint16), np.clip(np.rint(B), 1, 65535).astype(np.uint16)


PAIRS = [(8, 1), (8, 3), (16, 4), (64, 4), (128, 16)]           # (T, S) of the texture cases


def shifts(S):
    return [(0, 0), (S - 1, -(S - 1)), (-1, 1)]


def step_of(T):
    return max(T // 2, 5)
