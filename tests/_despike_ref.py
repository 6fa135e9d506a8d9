"""Restatement of `oip despike` in numpy / plain Python: the column repair and the conditional 3 x 3 median of
include/oip_c.h (oip_despike_u16) in int64 with padding by index clamping and a sort of the nine neighbours, the column
table (oip_despike_column_table) and the list file (oip_load_column_list), each in the order the header states."""
import numpy as np


def repair_columns(img, coltab, valid_min):
    """step 1: (L, W) -> (L, W) int64, every column x replaced by the interpolation between columns Lx and Rx"""
    src = np.asarray(img).astype(np.int64)
    tab = np.asarray(coltab, dtype=np.int64).reshape(-1, 2)
    assert tab.shape[0] == src.shape[1]
    out = src.copy()
    for x, (lx, rx) in enumerate(tab):
        D = rx - lx
        if D == 0:
            out[:, x] = src[:, lx]
            continue
        a, b = src[:, lx], src[:, rx]
        both = (a * (rx - x) + b * (x - lx) + D // 2) // D
        out[:, x] = np.where((a < valid_min) | (b < valid_min), np.where(a >= valid_min, a, b), both)
    return out


def despike(img, thr_abs, thr_rel_q8, valid_min, spp=1, groups=1, coltab=None):
    """img: (L, W * spp) uint16, pixel-interleaved.  Returns (out (L, W * spp) uint16, counts (W * spp,) uint64)."""
    img = np.asarray(img)
    L = img.shape[0]
    assert groups in (1, 4) and spp in (1, 4) and (groups == 1 or spp == 1)
    if coltab is not None:
        assert spp == 1
        c = repair_columns(img, coltab, valid_min)
    else:
        c = img.astype(np.int64)
    c = c.reshape(L, -1, spp)
    W = c.shape[1]
    assert W % groups == 0
    gw = W // groups
    ys, xs = np.arange(L), np.arange(W)
    g0 = (xs // gw) * gw
    nine = []
    for j in range(3):
        rows = np.clip(ys + j - 1, 0, L - 1)
        for i in range(3):
            cols = np.clip(xs + i - 1, g0, g0 + gw - 1)
            n = c[rows][:, cols]
            nine.append(np.where(n < valid_min, c, n))
    med = np.sort(np.stack(nine), axis=0)[4]                # the 5th smallest
    T = thr_abs + ((med * thr_rel_q8) >> 8)
    rep = (np.abs(c - med) > T) & (c >= valid_min)
    out = np.where(rep, med, c)
    return out.astype(np.uint16).reshape(img.shape), rep.sum(axis=0).reshape(-1).astype(np.uint64)


def column_table(bad, w, groups=1):
    """((w, 2) int32 of (Lx, Rx), longest run of adjacent listed columns inside a group); ValueError as the library refuses"""
    if groups not in (1, 4) or w <= 0 or w % groups:
        raise ValueError("column_table: bad argument")
    bad = set(int(b) for b in bad)
    if any(b < 0 or b >= w for b in bad):
        raise ValueError("column_table: column outside [0, %d)" % w)
    gw = w // groups
    tab = np.zeros((w, 2), np.int32)
    longest = 0
    for g in range(groups):
        good = [x for x in range(g * gw, (g + 1) * gw) if x not in bad]
        if not good:
            raise ValueError("column_table: group %d has no good column" % g)
        run = 0
        for x in range(g * gw, (g + 1) * gw):
            if x not in bad:
                tab[x] = (x, x)
                run = 0
                continue
            run += 1
            longest = max(longest, run)
            left = [u for u in good if u < x]
            right = [u for u in good if u > x]
            lx = left[-1] if left else right[0]
            rx = right[0] if right else left[-1]
            tab[x] = (lx, rx)
    return tab, longest


def parse_column_list(path, w):
    """the sorted unique columns of a list file; OSError when it cannot be read, ValueError for a malformed one"""
    with open(path, "rb") as f:
        text = f.read()
    cols = set()
    for line in text.split(b"\n"):
        for tok in line.split(b"#", 1)[0].split():          # bytes.split(): ASCII white space only
            digits = tok[1:] if tok[:1] in (b"+", b"-") else tok
            if not digits or not all(ch in b"0123456789" for ch in digits):
                raise ValueError("parse_column_list: %r is not a number" % tok)
            v = int(tok)
            if not 0 <= v < w:
                raise ValueError("parse_column_list: column %d outside [0, %d)" % (v, w))
            cols.add(v)
    return sorted(cols)
