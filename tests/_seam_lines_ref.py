"""Restatement of the along-strip seam gains (`oip stitch --balance-lines`; include/oip_c.h next to the seam block), built on
_seam_ref: the overlap totals per block of lines, a fit per block with the whole strip's pair where a block has none of its
own, the nodes interpolated to a (G, O) per line with numpy's flooring `//`, and the stitch line by line.  Images are
(L, W * spp) uint16, pixel-interleaved; `fold` and `h` are in pixels, B is block_lines."""
import numpy as np

import _seam_ref as ref


def blocks(L, B):
    """[(first line, end line)] of the nb = max(1, L // B) blocks: a short tail belongs to the last one"""
    nb = max(1, L // B)
    return [(k * B, (k + 1) * B if k < nb - 1 else L) for k in range(nb)]


def build_drifting_pair(W, L, fold, seed=7, spp=1, g=(0.90, 1.10), o=(40.0, -25.0)):
    """ref.build_pair with a gain and an offset that run linearly over the L lines: right = rint((scene - o(r)) / g(r)).
    g, o: (first, last), or one such pair per channel."""
    rng = np.random.default_rng(seed)
    scene = rng.integers(300, 3801, (L, 2 * W - 2 * fold, spp)).astype(np.float64)
    g = np.broadcast_to(np.asarray(g, np.float64), (spp, 2))
    o = np.broadcast_to(np.asarray(o, np.float64), (spp, 2))
    gr = np.stack([np.linspace(g[c, 0], g[c, 1], L) for c in range(spp)], 1)[:, None, :]
    orr = np.stack([np.linspace(o[c, 0], o[c, 1], L) for c in range(spp)], 1)[:, None, :]
    left = scene[:, :W].astype(np.uint16)
    right = np.clip(np.rint((scene[:, W - 2 * fold:] - orr) / gr), 0, 65535).astype(np.uint16)
    return left.reshape(L, W * spp), right.reshape(L, W * spp)


def block_moments(left, right, fold, spp, B, valid_min=0, valid_max=65535):
    """(nb, 6, spp) uint64: ref.moments of every block's lines"""
    return np.stack([ref.moments(left[a:b], right[a:b], fold, spp, valid_min, valid_max) for a, b in blocks(left.shape[0], B)])


def fit_blocks(acc, mode, min_count=0):
    """-> G, O, substituted: (nb, spp) int64 each; G0, O0, identity0: lists.  ref.fit on the sum of the planes (its ValueError
    is this function's), then per block: a ValueError or an identity is replaced by the whole-strip pair."""
    nb, _, spp = acc.shape
    G0, O0, ident0, _ = ref.fit(acc.sum(0, dtype=np.uint64), mode, min_count)
    G, O, sub = (np.zeros((nb, spp), np.int64) for _ in range(3))
    for k in range(nb):
        for c in range(spp):
            try:
                g, o, ident, _ = ref.fit(acc[k][:, c:c + 1], mode, min_count)
                own = not ident[0]
            except ValueError:
                own = False
            G[k, c], O[k, c], sub[k, c] = (g[0], o[0], 0) if own else (G0[c], O0[c], 1)
    return G, O, sub, G0, O0, ident0


def line_tables(G, O, L, B):
    """(L, spp) int64 tables from the (nb, spp) nodes; node k sits at line k B + B // 2"""
    G, O = np.asarray(G, np.int64), np.asarray(O, np.int64)
    nb = G.shape[0]
    assert nb == max(1, L // B)
    u = np.arange(L, dtype=np.int64) - B // 2
    k = np.clip(u // B, 0, max(nb - 2, 0))
    t = np.clip(u - k * B, 0, B)[:, None]
    k1 = np.minimum(k + 1, nb - 1)
    return tuple((V[k] * (B - t) + V[k1] * t + B // 2) // B for V in (G, O))


def stitch_lines(left, right, fold, spp, LG, LO, h, valid_min):
    """ref.stitch line by line, line r with its own LG[r], LO[r]"""
    return np.concatenate([ref.stitch(left[r:r + 1], right[r:r + 1], fold, spp, LG[r], LO[r], h, valid_min) for r in range(left.shape[0])])
