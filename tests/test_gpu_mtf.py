"""GPU: oip_mtf_tiles_u16 (one record per slanted-edge tile and channel) and oip_mtf_esf_u16 (the edge-spread sums of listed
tiles) against the restatement (_mtf_ref.py).  Both are exact integer functions of the samples, so every comparison is equality.
The rasters are fields of 32 x 32 cells planted to end in every status 0..7, with both polarities and with tiles that pass the
integer tests and give no value on the host (EMPTYBIN)."""
import functools

import numpy as np
import pytest

import _mtf_ref as ref
import opticalimageprocessor_amd as oip

pytestmark = pytest.mark.gpu
FILL = 0x5A5A5A5A                                                      # what the record buffer holds before a call: no status
KW = dict(contrast_min=200, tv_slack=ref.FIELD_SLACK, valid_min=1, valid_max=60000)


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


@functools.lru_cache(maxsize=None)
def _field(rows, w, axis, seed, spp=1):
    return ref.field(rows, w, axis, seed, spp)


def _records(ctx, dev, ptr_offset, pitch, w, rows, spp, axis, rec_pitch=None, **kw):
    """the record planes of a call as (spp, nty + 1, rec_pitch, 4) int32: one line and some columns more than the tiles"""
    import torch
    nty, ntx = ref.tile_counts(w, rows, axis)
    rp = ntx + 3 if rec_pitch is None else rec_pitch
    out = torch.full((spp, nty + 1, max(rp, 1), 4), FILL, dtype=torch.int32, device="cuda")
    ctx.mtf_tiles_u16(dev.data_ptr() + 2 * ptr_offset, pitch, w, rows, spp, axis, out, rp, (nty + 1) * max(rp, 1), **dict(KW, **kw))
    ctx.sync()
    return out.cpu().numpy()


def _check(got, want):
    spp, nty, ntx, _ = want.shape
    assert np.array_equal(got[:, :nty, :ntx], want), "%d of %d records differ" % (int((got[:, :nty, :ntx] != want).any(-1).sum()), want[..., 0].size)
    assert (got[:, :, ntx:] == FILL).all() and (got[:, nty:] == FILL).all()            # nothing written beside the records


def _esf(ctx, dev, ptr_offset, pitch, w, rows, spp, axis, entries, **kw):
    import torch
    n = len(entries)
    lst = torch.from_numpy(np.ascontiguousarray(entries, dtype=np.int32)).cuda()
    out = torch.full((n + 1, 128), FILL, dtype=torch.int32, device="cuda")
    s0 = torch.full((n + 1,), FILL, dtype=torch.int32, device="cuda")
    ctx.mtf_esf_u16(dev.data_ptr() + 2 * ptr_offset, pitch, w, rows, spp, axis, lst, n, out, s0, **dict(KW, **kw))
    ctx.sync()
    out, s0 = out.cpu().numpy(), s0.cpu().numpy()
    assert (out[n] == FILL).all() and s0[n] == FILL
    return out[:n].view(np.uint32), s0[:n]


def _entries(want, extra=12):
    """the status-0 tiles in (channel, ty, tx) order, and some tiles of other statuses after them"""
    ok = ref.ok_list(want)
    other = np.argwhere(want[..., 0] != 0).astype(np.int32)[:: max(1, int((want[..., 0] != 0).sum()) // extra)]
    return np.concatenate([ok, other]), len(ok)


def _kinds(img, want, spp, axis, esf, n_ok, entries):
    """every status, both polarities, and a status-0 tile without a value on the host"""
    status = set(want[..., 0].ravel().tolist())
    pol = set(want[..., 1][want[..., 0] == 0].ravel().tolist())
    vals = [oip.mtf_tile(want[tuple(e)][1], x[:64], x[64:]) for e, x in zip(entries[:n_ok], esf[:n_ok])]
    return status == set(range(8)) and pol == {1, -1} and any(v is None for v in vals) and any(v is not None for v in vals)


def _whole(ctx, img, dev, ptr_offset, pitch, w, rows, spp, axis, need_kinds=True, **kw):
    win = img[:, ptr_offset:ptr_offset + w * spp]
    p = dict(KW, **kw)
    want = ref.records(win, spp, axis, **p)
    _check(_records(ctx, dev, ptr_offset, pitch, w, rows, spp, axis, **kw), want)
    entries, n_ok = _entries(want)
    got, s0 = _esf(ctx, dev, ptr_offset, pitch, w, rows, spp, axis, entries, **kw)
    assert np.array_equal(got, ref.esf(win, spp, axis, entries, **p))
    assert not got[n_ok:].any() and not s0[n_ok:].any() and (n_ok == 0 or got[:n_ok, 64:].all())
    pl = ref.planes(win, spp)
    for e, s in zip(entries[:n_ok], s0[:n_ok]):
        assert s == ref.analyse(ref.tiles(pl[e[0]], axis)[e[1], e[2]], **p)[2] > 0
    if need_kinds:
        assert _kinds(win, want, spp, axis, got, n_ok, entries)
    return want


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("w,rows", [(80, 70), (1003, 77), (1003, 200), (100, 600)])
def test_records_and_esf_whole_raster(ctx, axis, w, rows):
    """80 x 70: four staggered x tiles per tile line, two tile lines, remainders both ways.  1003 x 77: an odd pitch (sample
    loads), several runs per line block.  1003 x 200 and 100 x 600: more than one workgroup on either axis and, on y, runs of
    more than 16 tiles down the columns."""
    img = _field(rows, w, axis, w + axis)
    want = _whole(ctx, img, _cuda(img), 0, w, w, rows, 1, axis, need_kinds=w > 80)
    assert want.shape[1:3] == ref.tile_counts(w, rows, axis)
    if (w, rows) == (80, 70):
        assert want.shape[1:3] == ((2, 4) if axis == 0 else (3, 2))


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("col0,w", [(3, 1000), (8, 1000), (8, 1001), (16, 47)])
def test_records_window(ctx, axis, col0, w):
    """a window of a 4096-wide raster (pitch > w): a start that is not 16-byte aligned, one that is, widths that leave a remainder"""
    rows, pitch = 100, 4096
    img = np.roll(_field(rows, pitch, axis, 7 + axis), col0, axis=1)    # the planted cells line up with the window's tiles
    _whole(ctx, img, _cuda(img), col0, pitch, w, rows, 1, axis, need_kinds=w >= 1000)


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("col0", [0, 2, 3])
def test_records_four_samples_per_pixel(ctx, axis, col0):
    """250 pixels x 100 lines of 4 samples, whole and as windows of a 300-pixel raster that start 16 and 24 bytes in"""
    rows, px = 100, 250
    pitch = px * 4 if col0 == 0 else 300 * 4
    img = np.roll(_field(rows, pitch // 4, axis, 11 + axis, 4), col0 * 4, axis=1)
    want = _whole(ctx, img, _cuda(img), col0 * 4, pitch, px, rows, 4, axis)
    assert len({want[c].tobytes() for c in range(4)}) == 4             # the channels differ


def test_parameters_change_the_records(ctx):
    """the four parameters reach the kernel: each of them moves tiles between statuses"""
    img = _field(200, 1003, 0, 1003)
    dev = _cuda(img)
    seen = set()
    for kw in (dict(), dict(tv_slack=0), dict(tv_slack=65535), dict(contrast_min=1), dict(contrast_min=3000), dict(valid_min=0, valid_max=65535),
               dict(valid_min=1000, valid_max=3000)):
        want = ref.records(img, 1, 0, **dict(KW, **kw))
        _check(_records(ctx, dev, 0, 1003, 1003, 200, 1, 0, **kw), want)
        seen.add(want.tobytes())
    assert len(seen) == 7


@pytest.mark.parametrize("axis,spp", [(0, 1), (1, 1), (1, 4)])
def test_two_calls_give_the_records_of_one(ctx, axis, spp):
    """a strip cut at a multiple of 32 lines; on y the second call starts 16 lines before the first one's last tile ends.  The
    calls run in the other order than the lines."""
    import torch
    rows, px = 200, 200 // spp
    img = _field(rows, px, axis, 21 + axis, spp)
    dev = _cuda(img)
    nty, ntx = ref.tile_counts(px, rows, axis)
    want = ref.records(img, spp, axis, **KW)
    out = torch.full((spp, nty, ntx, 4), FILL, dtype=torch.int32, device="cuda")
    cut = 96
    first2, ty2 = (cut, cut // 32) if axis == 0 else (cut - 16, (cut - 32) // 16 + 1)
    for line0, lines, ty0 in ((first2, rows - first2, ty2), (0, cut, 0)):
        ctx.mtf_tiles_u16(dev.data_ptr() + 2 * line0 * px * spp, px * spp, px, lines, spp, axis, out.data_ptr() + 16 * ty0 * ntx, ntx, nty * ntx, **KW)
    ctx.sync()
    assert np.array_equal(out.cpu().numpy(), want)


def test_invalid_arguments(ctx):
    import torch
    img = _field(64, 96, 0, 5)
    dev = _cuda(img)
    rec = torch.full((4, 2, 5, 4), FILL, dtype=torch.int32, device="cuda")
    lst = torch.tensor([[0, 1, 4]], dtype=torch.int32, device="cuda")
    esf = torch.full((2, 128), FILL, dtype=torch.int32, device="cuda")

    def tiles(pitch=96, w=96, rows=64, spp=1, axis=0, rp=5, src=dev, dst=rec, **kw):
        ctx.mtf_tiles_u16(src, pitch, w, rows, spp, axis, dst, rp, 10, **dict(KW, **kw))

    def bins(pitch=96, w=96, rows=64, spp=1, axis=0, entries=lst, n=1, src=dev, dst=esf, **kw):
        ctx.mtf_esf_u16(src, pitch, w, rows, spp, axis, entries, n, dst, None, **dict(KW, **kw))
    common = (dict(axis=2), dict(axis=-1), dict(spp=2), dict(spp=0), dict(spp=3), dict(contrast_min=0), dict(contrast_min=-5), dict(tv_slack=-1),
              dict(tv_slack=65536), dict(valid_min=-1), dict(valid_max=65536), dict(valid_min=9, valid_max=8), dict(pitch=95),
              dict(spp=4, w=24, pitch=95), dict(w=-1), dict(rows=-1), dict(src=None), dict(src=dev.data_ptr() + 1))
    for bad in common + (dict(rp=4), dict(dst=None), dict(axis=1, rp=2)):
        with pytest.raises(ValueError):
            tiles(**bad)
    for bad in common + (dict(dst=None), dict(entries=None), dict(n=-1)):
        with pytest.raises(ValueError):
            bins(**bad)
    # an entry outside the channels or the 2 x 5 tiles (x) / 3 x 3 tiles (y) of the window: refused before anything is launched
    for entry, axis in (([1, 0, 0], 0), ([-1, 0, 0], 0), ([0, 2, 0], 0), ([0, 0, 5], 0), ([0, -1, 0], 0), ([0, 0, -1], 0), ([0, 3, 0], 1), ([0, 0, 3], 1)):
        with pytest.raises(ValueError, match="outside"):
            bins(entries=torch.tensor([[0, 0, 0], entry], dtype=torch.int32, device="cuda"), n=2, axis=axis)
    # no whole tile, or an empty list: a no-op
    for nothing in (dict(rows=31), dict(w=31), dict(rows=0), dict(w=0)):
        tiles(**nothing)
    bins(n=0)
    with pytest.raises(ValueError):
        bins(rows=31)                                                   # the window holds no tile: the entry lies outside it
    ctx.sync()
    assert (rec.cpu().numpy() == FILL).all() and (esf.cpu().numpy() == FILL).all()
    tiles()
    bins()
    ctx.sync()
    got = rec.cpu().numpy()
    assert (got[0, :, :5] != FILL).all() and (got[1:] == FILL).all() and (esf.cpu().numpy()[0] != FILL).all()


def test_profiler_sees_the_kernels(ctx):
    import torch
    img = _field(64, 520, 0, 1)
    dev = _cuda(img)
    rec = torch.zeros((4, 4, 40, 4), dtype=torch.int32, device="cuda")
    ctx.profile_enable(True)
    ctx.profile_reset()
    ctx.mtf_tiles_u16(dev, 520, 520, 64, 1, 0, rec, 40, 160)
    ctx.mtf_tiles_u16(dev, 520, 520, 64, 1, 1, rec, 40, 160)
    ctx.mtf_tiles_u16(dev.data_ptr() + 2, 520, 512, 64, 1, 0, rec, 40, 160)
    ctx.mtf_tiles_u16(dev, 520, 130, 64, 4, 0, rec, 40, 160)
    ctx.sync()
    prof = ctx.profile()
    ctx.profile_enable(False)
    assert prof["mtf_tiles_u16_kernel"][1] == 1 and prof["mtf_tiles_u16_any_kernel"][1] == 3
