"""GPU: oip_mtf_tiles_u16 and oip_mtf_esf_u16 at addresses past 2^31 samples, where the lines of a real strip live, on the probe
raster of tests/_bigraster.py (32760 x 65600 = 2 149 056 000 samples: one constant on every line but a head and a tail band), with
the bands planted with the edge cells of _mtf_ref.field on the tile grid.  On the constant lines every record is FLAT; the tile
lines that touch a band -- the tail band's source lines from 65553 on lie wholly past 2^31 samples -- hold the restatement's
records, and the status-0 tiles among them give the restatement's edge-spread sums.  A kernel that computed `line * pitch` in 32
bits reads the head of the raster for the tail band; the CPU twin at the bottom (not `gpu`) shows on _bigraster.SMALL that the
check rejects that."""
import gc

import numpy as np
import pytest

import _bigraster as br
import _mtf_ref as ref

KW = dict(contrast_min=200, tv_slack=ref.FIELD_SLACK, valid_min=1, valid_max=60000)
FLAT = np.array([ref.FLAT, 0, 0, 0], np.int32)


def _bands(geo, axis, spp):
    """the two bands as [head, tail] 'noises' of _bigraster: cells of every kind on the 32-line grid of the raster, repeated along
    the line every 2048 pixels"""
    out = []
    px = geo.W // spp
    for k, (a, b) in enumerate((geo.head, geo.tail)):
        a0 = a // 32 * 32
        f = ref.field(-(-(b - a0) // 32) * 32, min(px, 2048), axis, 50 + 2 * axis + k, spp)
        f = np.tile(f.reshape(f.shape[0], -1, spp), (1, -(-px // 2048), 1))[:, :px].reshape(f.shape[0], px * spp)
        out.append(np.ascontiguousarray(f[a - a0:b - a0]))
    return out


def _windows(geo, axis):
    """per band the lines [lo, hi) whose tiles can touch it, lo a multiple of 32, and the tile lines [t0, t1) they hold"""
    step = 32 if axis == 0 else 16
    out = []
    for a, b in (geo.head, geo.tail):
        lo, hi = max(0, a // 32 * 32 - 32), min(geo.L, -(-b // 32) * 32 + 32)
        out.append((lo, hi, lo // step, lo // step + ref.tile_counts(geo.W, hi - lo, axis)[0]))
    return out


def _expected(geo, noises, axis, spp):
    """[(t0, t1, records (spp, t1 - t0, ntx, 4), window)] per band"""
    out = []
    for k, (lo, hi, t0, t1) in enumerate(_windows(geo, axis)):
        win = br.band_input(geo, k, noises[k], lo, hi)
        out.append((t0, t1, ref.records(win, spp, axis, **KW), win))
    return out


def _check(rec, expected):
    """rec (spp, nty, ntx, 4), numpy or torch: the restatement inside the windows, FLAT everywhere else"""
    is_np = isinstance(rec, np.ndarray)
    pos = 0
    for t0, t1, want, _ in expected + [(rec.shape[1], rec.shape[1], None, None)]:
        if pos < t0:
            blk = rec[:, pos:t0]
            if is_np:
                ok = bool((blk == FLAT).all())
            else:
                import torch
                ok = bool((blk == torch.from_numpy(FLAT).to(blk.device)).all())
            assert ok, "a tile of constant lines in tile lines [%d, %d) is not FLAT" % (pos, t0)
        if want is not None:
            got = rec[:, t0:t1] if is_np else rec[:, t0:t1].cpu().numpy()
            assert np.array_equal(got, want), "tile lines [%d, %d): %d records differ from the restatement" % (t0, t1, int((got != want).any(-1).sum()))
        pos = max(pos, t1)


@pytest.mark.gpu
@pytest.mark.parametrize("axis,spp", [(0, 1), (1, 1), (1, 4)])
def test_records_and_esf_whole_raster(ctx, axis, spp):
    """peak device memory: 4.3 GB (the raster) + 67 MB (the records)"""
    import torch
    geo = br.BIG
    f = geo.assert_crosses()
    assert f * geo.W >= br.TWO31 and geo.tail[0] < f < geo.L
    noises = _bands(geo, axis, spp)
    src = br.device_raster(geo, noises)
    px = geo.W // spp
    nty, ntx = ref.tile_counts(px, geo.L, axis)
    rec = torch.full((spp, nty, ntx, 4), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    ctx.mtf_tiles_u16(src, geo.W, px, geo.L, spp, axis, rec, ntx, nty * ntx, **KW)
    ctx.sync()
    expected = _expected(geo, noises, axis, spp)
    _check(rec, expected)
    # the status-0 tiles of the tail window whose lines lie wholly past 2^31 samples
    t0, t1, want, win = expected[1]
    step = 32 if axis == 0 else 16
    local = ref.ok_list(want)
    local = local[(t0 + local[:, 1]) * step >= f]
    assert len(local) >= 20 and set(want[tuple(local.T)][:, 1].tolist()) == {1, -1} and set(local[:, 0].tolist()) == set(range(spp))
    local = local[:: max(1, len(local) // 200)]
    entries = torch.from_numpy(np.ascontiguousarray(local + np.array([0, t0, 0], np.int32))).cuda()
    esf = torch.zeros((len(local), 128), dtype=torch.int32, device="cuda")
    ctx.mtf_esf_u16(src, geo.W, px, geo.L, spp, axis, entries, len(local), esf, None, **KW)
    ctx.sync()
    got = esf.cpu().numpy().view(np.uint32)
    assert np.array_equal(got, ref.esf(win, spp, axis, local, **KW)) and got[:, 64:].all()
    del src, rec, esf
    gc.collect()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("axis", [0, 1])
def test_check_rejects_a_wrapped_read(axis):
    """the same check on the host at _bigraster.SMALL (64 x 240, offsets wrap at element 192 * 64 + 8): the restatement of the
    whole raster passes; the raster read through a wrapping offset does not"""
    geo = br.SMALL
    noises = _bands(geo, axis, 1)
    x = br.host_raster(geo, noises)
    expected = _expected(geo, noises, axis, 1)
    truth = ref.records(x, 1, axis, **KW)
    _check(truth, expected)
    assert len(set(truth[..., 0].ravel().tolist())) >= 4                # (64 samples wide: two cells a line, of several kinds)
    wrapped = ref.records(br.wrapped_read(x, geo.wrap), 1, axis, **KW)
    with pytest.raises(AssertionError):
        _check(wrapped, expected)
    bad = truth.copy()
    bad[0, -1, -1, 3] ^= 1
    with pytest.raises(AssertionError):
        _check(bad, expected)
