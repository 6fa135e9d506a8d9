"""GPU: oip_despike_u16 against the integer restatement (_despike_ref.py).  The arithmetic is exact, so every comparison --
pixels and counts -- is equality.

The kernel's tile is 512 samples x 16 lines INSIDE one column group (a band of a BIL line), one tile per block, no
grid-stride loop; the aligned form needs a line and a group of a multiple of 8 samples (the bases torch hands out are
16-byte aligned).  Which form a shape (W, L, spp, groups) takes and how it meets the tiles:
    (1, 7, 1, 1), (3, 1, 1, 1)  per-sample   narrower / shorter than the window: every neighbour is a replicated border sample
    (2, 2, 4, 1)                aligned      8 samples: one chunk, both horizontal neighbours of either pixel in the same chunk
    (96, 64, 1, 1)              aligned      one tile across, four down
    (521, 257, 1, 1)            per-sample   two tiles across (the second 9 samples wide), 17 down (the last a single line)
    (1024, 37, 1, 1)            aligned      two full tiles across: the halo crosses a tile edge; three down (the last 5 lines)
    (131, 100, 4, 1)            per-sample   524 samples: two tiles across (the second 12 samples wide), seven down
    (256, 300, 4, 1)            aligned      1024 samples: a pixel's neighbours 4 samples away cross the tile edge
    (148, 100, 1, 4)            per-sample   gw = 37: four one-tile groups, band borders mid-vector
    (2048, 33, 1, 4)            aligned      gw = 512: a band border exactly on a tile edge, the halo chunk beyond it is clamped
    (8, 5000, 1, 1)             aligned      one lane of a wave has work, 313 tiles down
These are the shapes of the issue unchanged: the tile is convolve.hip's."""
import functools

import numpy as np
import pytest

import _despike_ref as ref

pytestmark = pytest.mark.gpu

SHAPES = [(1, 7, 1, 1), (3, 1, 1, 1), (2, 2, 4, 1), (96, 64, 1, 1), (521, 257, 1, 1), (1024, 37, 1, 1), (131, 100, 4, 1), (256, 300, 4, 1),
          (148, 100, 1, 4), (2048, 33, 1, 4), (8, 5000, 1, 1)]
PARAMS = [(20000, 64, 1), (20000, 64, 0), (0, 0, 0), (65535, 0, 1)]            # (thr_abs, thr_rel_q8, valid_min)


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _image(W, L, spp):
    """full-range data with 3 % zeros; shared by the tests of a shape, which leave it unchanged"""
    rng = np.random.default_rng(1000 * W + L)
    img = rng.integers(0, 65536, (L, W * spp), dtype=np.uint16)
    img[rng.random(img.shape) < 0.03] = 0
    return img


@functools.lru_cache(maxsize=None)
def _want(W, L, spp, groups, params):
    return ref.despike(_image(W, L, spp), *params, spp=spp, groups=groups)


def _bad_columns(W, groups):
    """{0, 7, 8, W - 1}, both sides of every band border, a run of 3 past the middle of the first group; on two tiles both
    sides of the tile edge as well"""
    gw = W // groups
    bad = {0, 7, 8, W - 1, gw // 2 + 3, gw // 2 + 4, gw // 2 + 5}
    for b in range(1, groups):
        bad |= {b * gw - 1, b * gw}
    if gw > 512:
        bad |= {511, 512}
    return sorted(bad)


def _despike(ctx, img, W, L, spp, groups, params, coltab=None, count=True):
    """one call over the whole raster; returns (pixels, counts or None)"""
    import torch
    out = torch.zeros(L, W * spp, dtype=torch.uint16, device="cuda")
    cnt = torch.zeros(W * spp, dtype=torch.int64, device="cuda") if count else None
    tab = _cuda(coltab) if coltab is not None else None
    ctx.despike_u16(_cuda(img), out, W, L, spp, params[0], params[1], params[2], groups, tab, cnt)
    ctx.sync()
    return out.cpu().numpy(), (cnt.cpu().numpy().astype(np.uint64) if count else None)


@pytest.mark.parametrize("params", PARAMS)
@pytest.mark.parametrize("W,L,spp,groups", SHAPES)
def test_equals_restatement(ctx, W, L, spp, groups, params):
    img = _image(W, L, spp)
    want, want_cnt = _want(W, L, spp, groups, params)
    if params[0] == 20000 and img.size >= 1000:
        # the test cannot pass by never or always replacing: the restatement itself replaces a fair share
        share = float(want_cnt.sum()) / float((img >= params[2]).sum())
        print("replaced share %.4f" % share)
        assert 0.05 <= share <= 0.40
    got, cnt = _despike(ctx, img, W, L, spp, groups, params)
    assert np.array_equal(got, want)
    assert np.array_equal(cnt, want_cnt)
    if params[0] == 65535:
        assert np.array_equal(got, img) and not cnt.any()           # switched off: the input byte for byte


@pytest.mark.parametrize("W,L,spp,groups", [(96, 64, 1, 1), (131, 100, 4, 1), (148, 100, 1, 4), (1024, 37, 1, 1)])
def test_counts_add_and_are_optional(ctx, W, L, spp, groups):
    import torch
    params = PARAMS[0]
    img = _image(W, L, spp)
    want, want_cnt = _want(W, L, spp, groups, params)
    src = _cuda(img)
    out = torch.zeros(L, W * spp, dtype=torch.uint16, device="cuda")
    cnt = torch.full((W * spp,), 5, dtype=torch.int64, device="cuda")
    for _ in range(2):                                              # a second call adds, it does not overwrite
        ctx.despike_u16(src, out, W, L, spp, *params, groups, None, cnt)
    ctx.sync()
    assert np.array_equal(cnt.cpu().numpy().astype(np.uint64), 5 + 2 * want_cnt)
    got, none = _despike(ctx, img, W, L, spp, groups, params, count=False)
    assert none is None and np.array_equal(got, want)               # d_count = NULL: the same pixels


@pytest.mark.parametrize("data", ["valid", "zeros", "gap"])
@pytest.mark.parametrize("W,L,groups", [(96, 70, 1), (96, 70, 4), (148, 70, 4), (1024, 70, 1), (2048, 70, 4), (521, 70, 1)])
def test_column_table(ctx, W, L, groups, data):
    """aligned shapes take the 16-byte load where a chunk holds no listed column and the per-sample path where it does;
    (148, 70, 4) and (521, 70, 1) take the per-sample path throughout.  `gap`: a 40-line all-zero block as the de-framer
    leaves it for a missing frame -- it comes out all zero (nothing is interpolated into it) and the lines next to it are
    the restatement's (it stays out of their medians)."""
    rng = np.random.default_rng(W + groups)
    img = rng.integers(1, 65536, (L, W), dtype=np.uint16)
    if data != "valid":
        img[rng.random(img.shape) < 0.03] = 0
    if data == "gap":
        img[15:55] = 0
    bad = _bad_columns(W, groups)
    tab, run = ref.column_table(bad, W, groups)
    assert run == 3 and len(bad) >= 7
    for params in [(20000, 64, 1), (65535, 0, 1)]:                  # with the median, and column repair alone
        want, want_cnt = ref.despike(img, *params, groups=groups, coltab=tab)
        got, cnt = _despike(ctx, img, W, L, 1, groups, params, coltab=tab)
        assert np.array_equal(got, want) and np.array_equal(cnt, want_cnt)
        if data == "gap":
            assert not got[15:55].any()
    good = np.setdiff1d(np.arange(W), bad)
    assert np.array_equal(got[:, good], img[:, good])               # repair alone leaves the good columns as they are
    if data == "valid":
        assert (got[:, bad] != img[:, bad]).mean() > 0.9            # ... and fills the listed ones


def _scene(W, L, spikes, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:L, 0:W]
    clean = 1000 + 5 * x + 3 * y
    img = clean + rng.integers(-3, 4, (L, W))
    for (sy, sx), amp in spikes.items():
        img[sy, sx] += amp
    return clean, img.astype(np.uint16)


@pytest.mark.parametrize("W", [96, 1040])
def test_scene_spikes_and_nothing_else(ctx, W):
    """A ramp 1000 + 5 x + 3 y with +-3 noise and isolated +-800 spikes, no two within 2 pixels of each other: the four
    corners, the top edge, the interior, and on the wider image both sides of the tile edge between samples 511 and 512 and
    of the one between lines 15 and 16.  Threshold 100: exactly the spikes are replaced, and each by a value within 6 DN of
    the clean ramp.  Why 6: a neighbour differs from the clean centre by -8 .. 8 from the ramp plus its noise of at most 3;
    in the interior the median is the 5th of eight such values and a spike, at most |-2| + 3 or 2 + 3.  At a border the
    spike is replicated (4 copies in a corner, 2 on an edge), so the sign of each is chosen so that the 5th value is the
    neighbour nearest in value: offset 3 in the top-left corner (-800), 3 top-right (+800), -3 bottom-left (-800),
    -3 bottom-right (+800), -2 on the top edge (-800); with the noise at most 6."""
    L = 64
    spikes = {(0, 0): -800, (0, W - 1): 800, (L - 1, 0): -800, (L - 1, W - 1): 800, (0, 40): -800, (30, 50): 800, (40, 20): -800,
              (15, 70): 800, (16, 80): -800}
    if W > 512:
        spikes.update({(10, 511): 800, (20, 512): -800, (30, 513): 800, (40, 510): -800, (15, 600): -800, (16, 700): 800})
    pos = sorted(spikes)
    for i, a in enumerate(pos):
        for b in pos[i + 1:]:
            assert max(abs(a[0] - b[0]), abs(a[1] - b[1])) > 2
    clean, img = _scene(W, L, spikes, 5)
    want, want_cnt = ref.despike(img, 100, 0, 1)
    got, cnt = _despike(ctx, img, W, L, 1, 1, (100, 0, 1))
    for out, n in ((want, want_cnt), (got, cnt)):                   # the restatement does this; so does the kernel
        assert sorted(zip(*np.nonzero(out != img))) == pos
        assert int(n.sum()) == len(pos)
        print("max |out - clean| %d" % np.abs(out.astype(np.int64) - clean).max())
        assert np.abs(out.astype(np.int64) - clean).max() <= 6
    assert np.array_equal(got, want) and np.array_equal(cnt, want_cnt)


@pytest.mark.parametrize("step", [1, 5, 16, 23])
@pytest.mark.parametrize("W,L,groups,table", [(96, 64, 1, False), (148, 50, 4, True), (1024, 37, 1, True)])
def test_strip_cut_into_calls(ctx, W, L, groups, table, step):
    """each call sees exactly the lines it needs (its output lines and one halo line either side inside the image), uploaded
    to a buffer of their own, and writes at the start of a buffer of its own: together the bytes and counts of one call"""
    import torch
    params = PARAMS[0]
    img = _image(W, L, 1)
    tab = ref.column_table(_bad_columns(W, groups), W, groups)[0] if table else None
    want, want_cnt = ref.despike(img, *params, groups=groups, coltab=tab)
    d_tab = _cuda(tab) if table else None
    cnt = torch.zeros(W, dtype=torch.int64, device="cuda")
    parts = []
    for a in range(0, L, step):
        b = min(L, a + step)
        s0, s1 = max(0, a - 1), min(L, b + 1)
        out = torch.zeros(b - a, W, dtype=torch.uint16, device="cuda")
        ctx.despike_u16(_cuda(img[s0:s1]), out, W, L, 1, *params, groups, d_tab, cnt, src_row0=s0, src_rows=s1 - s0, out_row0=a, out_rows=b - a)
        parts.append(out)
    ctx.sync()
    assert np.array_equal(np.concatenate([p.cpu().numpy() for p in parts]), want)
    assert np.array_equal(cnt.cpu().numpy().astype(np.uint64), want_cnt)


def test_misaligned_bases_take_the_per_sample_kernel(ctx):
    """source and destination start one sample into 16-byte aligned buffers (the lines keep their pitch): the same bytes"""
    import torch
    W, L = 96, 64
    params = PARAMS[0]
    img = _image(W, L, 1)
    tab = ref.column_table(_bad_columns(W, 1), W, 1)[0]
    want, want_cnt = ref.despike(img, *params, coltab=tab)
    src = torch.zeros(L * W + 8, dtype=torch.uint16, device="cuda")
    src[1:1 + L * W] = _cuda(img).reshape(-1)
    out = torch.zeros(L * W + 8, dtype=torch.uint16, device="cuda")
    cnt = torch.zeros(W, dtype=torch.int64, device="cuda")
    ctx.despike_u16(src.data_ptr() + 2, out.data_ptr() + 2, W, L, 1, *params, 1, _cuda(tab), cnt)
    ctx.sync()
    got = out.cpu().numpy()
    assert np.array_equal(got[1:1 + L * W].reshape(L, W), want) and np.array_equal(cnt.cpu().numpy().astype(np.uint64), want_cnt)
    assert not got[:1].any() and not got[1 + L * W:].any()          # nothing outside the destination raster


def test_bad_arguments_and_profiler(ctx):
    import torch
    W, L = 96, 64
    img = _cuda(_image(W, L, 1))
    out = torch.zeros(L, W, dtype=torch.uint16, device="cuda")
    tab = _cuda(ref.column_table([3], W)[0])
    for kw in [dict(thr_abs=-1), dict(thr_abs=65536), dict(thr_rel_q8=-1), dict(thr_rel_q8=257), dict(valid_min=-1), dict(valid_min=65536),
               dict(spp=2), dict(spp=3), dict(groups=2), dict(groups=0), dict(groups=4, W=94), dict(W=0), dict(L=0),
               dict(src_row0=1, src_rows=L - 1),                    # output line 0 needs source line 0
               dict(src_rows=L - 1),                                # the last line is missing
               dict(out_row0=10, out_rows=20, src_row0=10, src_rows=21),        # the upper halo line is missing
               dict(out_row0=10, out_rows=20, src_row0=9, src_rows=21),         # the lower halo line is missing
               dict(out_row0=L - 4, out_rows=5),                    # output lines beyond the raster
               dict(dst=img)]:                                      # in place
        a = dict(dst=out, W=W, L=L, spp=1, thr_abs=100, thr_rel_q8=0, valid_min=1, groups=1, src_row0=0, src_rows=None, out_row0=0, out_rows=None)
        a.update(kw)
        with pytest.raises(ValueError):
            ctx.despike_u16(img, a["dst"], a["W"], a["L"], a["spp"], a["thr_abs"], a["thr_rel_q8"], a["valid_min"], a["groups"], None, None,
                            a["src_row0"], a["src_rows"], a["out_row0"], a["out_rows"])
    with pytest.raises(ValueError):
        ctx.despike_u16(img, out, 24, L, 4, 100, 0, 1, 4)           # groups 4 needs 1 sample per pixel
    with pytest.raises(NotImplementedError):
        ctx.despike_u16(img, out, 24, L, 4, 100, 0, 1, 1, tab)      # a table with 4 samples per pixel
    ctx.despike_u16(img, out, W, L, 1, 100, 0, 1, out_row0=10, out_rows=20, src_row0=9, src_rows=22)      # exactly the halo
    ctx.profile_enable(True)
    ctx.profile_reset()
    ctx.despike_u16(img, out, W, L, 1, *PARAMS[0])
    ctx.despike_u16(img, out, W, L, 1, *PARAMS[0], out_rows=0)      # no lines: no launch
    ctx.sync()
    prof = ctx.profile()
    ctx.profile_enable(False)
    assert prof["despike_u16_kernel"][1] == 1
    assert np.array_equal(out.cpu().numpy(), _want(W, L, 1, 1, PARAMS[0])[0])
