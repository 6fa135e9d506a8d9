"""GPU: oip_noise_blocks_u16 -- one key per block and channel -- against the restatement (_noise_ref.py).  The keys are exact
integer functions of the samples, so every comparison is equality: of the keys, and of oip_histogram_u16 over the key planes
with np.bincount of the restatement's keys."""
import functools

import numpy as np
import pytest

import _noise_ref as ref

pytestmark = pytest.mark.gpu
FILL = 0xABCD                                                          # what the key buffer holds before a call: no key (q = 0xCD < 255, level 0xAB)


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def _raster(rows, ws, seed, B, spp=1):
    """(rows, ws) samples: random 12-bit data (blocks of it have sigma past the 254 cap), about half of the blocks replaced by flat
    patches of small noise at a random level (real keys of every sigma), a quarter of those with a horizontal or vertical step in
    them, and one out-of-range sample in a corner of every 9th block"""
    rng = np.random.default_rng(seed)
    img = rng.integers(1, 4096, (rows, ws)).astype(np.uint16)
    k = 0
    for j in range(0, rows - B + 1, B):
        for i in range(0, ws - B * spp + 1, B * spp):
            k += 1
            if rng.random() < 0.5:
                amp = int(rng.choice([1, 2, 3, 5, 9, 17, 40, 120]))
                blk = int(rng.integers(1, 4096 - amp)) + rng.integers(0, amp, (B, B * spp))
                if rng.random() < 0.25:
                    if rng.random() < 0.5:
                        blk[:B // 2] += 3 * amp
                    else:
                        blk[:, :B * spp // 2] += 3 * amp
                img[j:j + B, i:i + B * spp] = blk
            if k % 9 == 0:
                cj, ci = [(0, 0), (0, B * spp - 1), (B - 1, 0), (B - 1, B * spp - 1)][(k // 9) % 4]
                img[j + cj, i + ci] = 0 if k % 2 else 60000
    return img


def _keys(ctx, dev, ptr_offset, pitch, w, rows, spp, B, shift, key_pitch=None, valid_min=1, valid_max=4095):
    """the key planes of a call as (spp, nby, key_pitch) uint16"""
    import torch
    nbx, nby = w // B, rows // B
    kp = nbx if key_pitch is None else key_pitch
    out = torch.full((spp, max(nby, 1), max(kp, 1)), FILL - 65536, dtype=torch.int16, device="cuda")
    ctx.noise_blocks_u16(dev.data_ptr() + 2 * ptr_offset, pitch, w, rows, spp, B, shift, out, kp, max(nby, 1) * max(kp, 1), valid_min, valid_max)
    ctx.sync()
    return out.cpu().numpy().view(np.uint16)


def _check(got, want):
    spp, nby, nbx = want.shape
    assert np.array_equal(got[:, :nby, :nbx], want), "%d of %d keys differ" % (int((got[:, :nby, :nbx] != want).sum()), want.size)
    assert (got[:, :, nbx:] == FILL).all() and (got[:, nby:] == FILL).all()            # nothing written beside the keys


def _kinds(want):
    """every kind of key occurs: no data, structured, real keys below both caps, the sigma cap"""
    real = (want & 0xFF) < 254
    return (want == ref.NODATA).any() and (want == ref.STRUCTURED).any() and real.any() and ((want & 0xFF) == 254).any()


@pytest.mark.parametrize("w,rows,B", [(264, 520, 8), (264, 520, 16), (1003, 77, 8), (1003, 77, 16)])
@pytest.mark.parametrize("shift", [0, 4, 8])
def test_keys_whole_raster(ctx, w, rows, B, shift):
    """264 x 520: more than one workgroup at B 8, a partial block column at B 16.  1003 x 77: a width and a height that leave
    partial blocks, and an odd pitch (the block-per-lane kernel).  shift 0: every mean lies past the level cap."""
    img = _raster(rows, w, w + B, B)
    want = ref.keys(img, 1, B, shift, 1, 4095)
    assert _kinds(want) and (shift != 0 or ((want >> 8) == 255).any())
    _check(_keys(ctx, _cuda(img), 0, w, w, rows, 1, B, shift), want)


@pytest.mark.parametrize("col0,w", [(3, 1000), (8, 1000), (8, 1001), (16, 2077), (1, 37)])
@pytest.mark.parametrize("B", [8, 16])
def test_keys_window(ctx, col0, w, B):
    """a window of a 4096-wide raster (pitch > w): an unaligned start; an aligned start; widths that are no multiple of 8 or of B"""
    rows, pitch = 100, 4096
    img = _raster(rows, pitch, 7, B)
    img = np.roll(img, col0, axis=1)                                   # the planted blocks line up with the window's
    want = ref.keys(img[:, col0:col0 + w], 1, B, 4, 1, 4095)
    assert _kinds(want) or w < 1000
    _check(_keys(ctx, _cuda(img), col0, pitch, w, rows, 1, B, 4), want)


@pytest.mark.parametrize("B", [8, 16])
@pytest.mark.parametrize("col0", [0, 2, 3])
def test_keys_four_samples_per_pixel(ctx, B, col0):
    """130 pixels x 40 lines of 4 samples, whole (pitch 520) and as windows of a 160-pixel raster that start 16 bytes and 24 bytes
    in (the second is not 16-byte aligned); a key pitch larger than the blocks per line"""
    rows, px = 40, 130
    pitch = px * 4 if col0 == 0 else 160 * 4
    img = np.roll(_raster(rows, pitch, 11 + B, B, 4), col0 * 4, axis=1)
    want = ref.keys(img[:, col0 * 4:(col0 + px) * 4], 4, B, 4, 1, 4095)
    assert want.shape == (4, rows // B, px // B) and _kinds(want)
    assert len({want[c].tobytes() for c in range(4)}) == 4             # the channels differ
    _check(_keys(ctx, _cuda(img), col0 * 4, pitch, px, rows, 4, B, 4, key_pitch=px // B + 5), want)


def test_key_pitch_and_valid_range(ctx):
    """a key pitch larger than the blocks per line at spp 1, and a valid range of its own: [100, 3000] at one call, all of
    0..65535 at another (no block is no data)"""
    img = _raster(64, 256, 3, 8)
    dev = _cuda(img)
    for vmin, vmax in ((100, 3000), (0, 65535), (1, 65535)):
        want = ref.keys(img, 1, 8, 4, vmin, vmax)
        assert (want == ref.NODATA).any() == (vmin > 0)
        _check(_keys(ctx, dev, 0, 256, 256, 64, 1, 8, 4, key_pitch=40, valid_min=vmin, valid_max=vmax), want)


def test_more_than_65535_lines_of_blocks(ctx):
    """8 samples x 560000 lines: one block per line of blocks, 70000 of them"""
    rows = 8 * 70000
    rng = np.random.default_rng(2)
    img = (rng.integers(300, 3800, (70000, 1, 1)) + rng.integers(0, 7, (70000, 8, 8))).reshape(rows, 8).astype(np.uint16)
    img[rng.integers(0, rows, 500), rng.integers(0, 8, 500)] = 0
    want = ref.keys(img, 1, 8, 4)
    assert want.shape == (1, 70000, 1) and len(np.unique(want)) > 500
    _check(_keys(ctx, _cuda(img), 0, 8, 8, rows, 1, 8, 4, valid_max=65535), want)


@functools.lru_cache(maxsize=None)
def _variance_edges(B):
    """blocks whose floor(16 D / (n (n - 1))) lands on r^2 and on r^2 - 1, found by a seeded search among noise blocks of the
    fitting amplitude and of every density (a share p of the samples deviates, p another for every block): [(block, t)]"""
    n = B * B
    rng = np.random.default_rng(B)
    out = []
    for r in (1, 2, 7, 31, 100, 254, 255):
        amp = int(round(0.866 * r)) + 1
        found = {}
        for _ in range(200):
            x = rng.integers(0, amp + 1, (20000, n)) * (rng.random((20000, n)) < rng.uniform(0.02, 1.0, (20000, 1)))
            S1, S2 = x.sum(1), (x * x).sum(1)
            t = (16 * (n * S2 - S1 * S1)) // (n * (n - 1))
            for target in (r * r, r * r - 1):
                hit = np.flatnonzero(t == target)
                if target not in found and hit.size:
                    found[target] = x[hit[0]].reshape(B, B)
            if len(found) == 2:
                break
        assert len(found) == 2, (B, r)
        out += [(1000 + blk, tt) for tt, blk in sorted(found.items())]
    return out


def _threshold_blocks(B):
    """blocks with E (n - 4) == 12 (D - E) exactly, just above and just below: quadrant 0 one DN above the others (E = 3 (n / 4)^2),
    and +-e pairs inside quadrants, which add 2 n e^2 each to D alone.  n = 64: D = 6 E needs sum e^2 = 30; n = 256: D = 22 E
    needs 504."""
    es = {8: ((5, 2, 1), (5, 2), (5, 2, 1, 1)), 16: ((22, 4, 2), (22, 4, 1), (22, 4, 2, 1))}[B]
    out = []
    for e in es:
        blk = np.full((B, B), 1000, np.int64)
        blk[:B // 2, :B // 2] += 1
        for i, v in enumerate(e):                                      # pair i in quadrant i % 4
            j0, i0 = (i % 4 // 2) * (B // 2), (i % 4 % 2) * (B // 2)
            blk[j0 + 1, i0 + 1] += v
            blk[j0 + 2, i0 + 2] -= v
        out.append(blk)
    return out


@pytest.mark.parametrize("B", [8, 16])
def test_crafted_blocks(ctx, B):
    """the ends of the arithmetic: values near 65535 (the 64-bit products, E (n - 4) close to 2^56 at B 16), variances on r^2
    and r^2 - 1 for r up to the cap, and the F test at equality, just above and just below"""
    n, h = B * B, B // 2
    rng = np.random.default_rng(B)
    blocks, expect = [], []
    half = np.zeros((B, B), np.int64)
    half[:, :h] = 65535                                                # the largest E a block can have
    blocks += [np.full((B, B), 65535), half, half.T, rng.integers(65000, 65536, (B, B)), rng.integers(0, 65536, (B, B)),
               65535 - (rng.random((B, B)) < 0.5) * 65535, np.zeros((B, B), np.int64)]
    expect += [255 << 8, ref.STRUCTURED, ref.STRUCTURED, None, None, None, 0]
    for blk, t in _variance_edges(B):
        r = int(np.sqrt(t + 1))
        assert t in (r * r, r * r - 1)
        blocks.append(blk)
        expect.append(None)
        key = ref.key_of_block(blk, 4, 0, 65535)
        assert key == ref.STRUCTURED or key & 0xFF == min(254, r if t == r * r else r - 1)
    tb = _threshold_blocks(B)
    for blk, above in zip(tb, (False, True, False)):
        v = [[int(x) for x in row] for row in blk]
        S1, S2 = sum(map(sum, v)), sum(x * x for row in v for x in row)
        Sq = [sum(v[j][i] for j in range(j0, j0 + h) for i in range(i0, i0 + h)) for j0 in (0, h) for i0 in (0, h)]
        D, E = n * S2 - S1 * S1, 4 * sum(s * s for s in Sq) - S1 * S1
        assert (E * (n - 4) > 12 * (D - E)) == above and (blk is not tb[0] or E * (n - 4) == 12 * (D - E))
        blocks.append(blk)
        expect.append(ref.STRUCTURED if above else None)
    img = np.concatenate([np.asarray(b, dtype=np.int64) for b in blocks], axis=1).astype(np.uint16)
    img = np.concatenate([img, img[:, ::-1], img[::-1]], axis=0)       # mirrored: the other quadrants carry the structure
    for shift in (0, 4, 8):
        want = ref.keys(img, 1, B, shift, 0, 65535)
        for i, e in enumerate(expect):
            assert e is None or want[0, 0, i] == e, (i, hex(int(want[0, 0, i])))
            assert ref.key_of_block(img[:B, i * B:(i + 1) * B], shift, 0, 65535) == want[0, 0, i]
        assert sum(1 for k in want[0, 0] if k & 0xFF not in (0, 254, 255)) >= 10
        _check(_keys(ctx, _cuda(img), 0, img.shape[1], img.shape[1], img.shape[0], 1, B, shift, valid_min=0, valid_max=65535), want)


@pytest.mark.parametrize("spp,B", [(1, 8), (1, 16), (4, 8)])
def test_three_calls_give_the_bytes_of_one(ctx, spp, B):
    """a raster cut at lines that are multiples of B, the calls in another order than the lines"""
    import torch
    rows, px = 10 * B + 5, 200 // spp
    img = _raster(rows, px * spp, 21, B, spp)
    dev = _cuda(img)
    nbx, nby = px // B, rows // B
    one = _keys(ctx, dev, 0, px * spp, px, rows, spp, B, 4)
    _check(one, ref.keys(img, spp, B, 4, 1, 4095))
    out = torch.full((spp, nby, nbx), FILL - 65536, dtype=torch.int16, device="cuda")
    cuts = [(3 * B, rows), (0, B), (B, 3 * B)]                         # (first line, end)
    for a, b in cuts:
        ctx.noise_blocks_u16(dev.data_ptr() + 2 * a * px * spp, px * spp, px, b - a, spp, B, 4, out.data_ptr() + 2 * (a // B) * nbx, nbx, nby * nbx, 1, 4095)
    ctx.sync()
    assert out.cpu().numpy().view(np.uint16).tobytes() == one.tobytes()


@pytest.mark.parametrize("spp", [1, 4])
def test_histogram_of_the_key_planes(ctx, spp):
    """oip_histogram_u16 over each key plane is np.bincount of the restatement's keys, the two sentinel counts included, and is
    additive over calls"""
    import torch
    rows, px, B = 208, 1040 // spp, 8
    img = _raster(rows, px * spp, 31, B, spp)
    want = ref.keys(img, spp, B, 4, 1, 4095)
    nbx, nby = px // B, rows // B
    keys = torch.zeros((spp, nby, nbx), dtype=torch.int16, device="cuda")
    ctx.noise_blocks_u16(_cuda(img), px * spp, px, rows, spp, B, 4, keys, nbx, nby * nbx, 1, 4095)
    for c in range(spp):
        hist = torch.zeros(65536, dtype=torch.int64, device="cuda")
        ctx.histogram_u16(keys[c], nbx, nbx, nby, hist)
        ctx.sync()
        got = hist.cpu().numpy().view(np.uint64)
        assert np.array_equal(got, ref.histogram(want[c]))
        assert got[ref.NODATA] == (want[c] == ref.NODATA).sum() > 0 and got[ref.STRUCTURED] == (want[c] == ref.STRUCTURED).sum() > 0
        ctx.histogram_u16(keys[c], nbx, nbx, nby // 2, hist)
        ctx.sync()
        assert np.array_equal(hist.cpu().numpy().view(np.uint64), ref.histogram(want[c]) + ref.histogram(want[c][:nby // 2]))


def test_invalid_arguments(ctx):
    import torch
    img = _cuda(_raster(32, 64, 1, 8))
    keys = torch.full((4, 4, 8), FILL - 65536, dtype=torch.int16, device="cuda")

    def call(pitch=64, w=64, rows=32, spp=1, B=8, shift=4, vmin=1, vmax=65535, kp=8, src=img, dst=keys):
        ctx.noise_blocks_u16(src, pitch, w, rows, spp, B, shift, dst, kp, 32, vmin, vmax)
    for bad in (dict(B=4), dict(B=12), dict(B=32), dict(spp=2), dict(spp=3), dict(spp=0), dict(shift=-1), dict(shift=9), dict(vmin=-1), dict(vmax=65536),
                dict(vmin=5, vmax=4), dict(pitch=63), dict(spp=4, w=16, pitch=63), dict(w=-8), dict(rows=-1), dict(kp=7), dict(src=None), dict(dst=None),
                dict(src=img.data_ptr() + 1)):
        with pytest.raises(ValueError):
            call(**bad)
    # no whole block: a no-op
    for nothing in (dict(rows=7), dict(w=7), dict(rows=0), dict(w=0), dict(B=16, w=15)):
        call(**nothing)
    ctx.sync()
    assert (keys.cpu().numpy().view(np.uint16) == FILL).all()
    call()
    ctx.sync()
    assert (keys.cpu().numpy().view(np.uint16)[0] != FILL).all()


def test_profiler_sees_the_kernels(ctx):
    import torch
    img = _cuda(_raster(64, 520, 1, 8))
    keys = torch.zeros((4, 8, 65), dtype=torch.int16, device="cuda")
    ctx.profile_enable(True)
    ctx.profile_reset()
    ctx.noise_blocks_u16(img, 520, 520, 64, 1, 8, 4, keys, 65, 0)
    ctx.noise_blocks_u16(img, 520, 520, 64, 1, 16, 4, keys, 65, 0)
    ctx.noise_blocks_u16(img, 520, 130, 64, 4, 8, 4, keys, 65, 8 * 65)
    ctx.noise_blocks_u16(img.data_ptr() + 2, 520, 512, 64, 1, 8, 4, keys, 65, 0)
    ctx.sync()
    prof = ctx.profile()
    ctx.profile_enable(False)
    assert prof["noise_blocks_u16_kernel"][1] == 3 and prof["noise_blocks_u16_any_kernel"][1] == 1
