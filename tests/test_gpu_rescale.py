"""GPU: oip_rescale_u16 against the numpy restatement in _rescale_ref.py, fed with the library's own tables (their equality with
the restatement's is test_rescale_cpu.py's).  Exact integers: every comparison is equality of all samples.  Rasters are 517 x 203
at one sample per pixel (a line of 517 samples: 2-byte loads) and 130 x 203 at four (a line of 520: 16-byte loads); output lines
are multiples of 8 samples in some cases and not in others, and tiles end ragged on both axes.  Every case is run as one call
and as three windows whose first lines are odd (never a tile boundary) on exactly the lines oip_rescale_src_range states."""
import numpy as np
import pytest

import _rescale_ref as ref

pytestmark = pytest.mark.gpu
FILL = 5000
L = 203
WIDTH = {1: 517, 4: 130}
# (name, lines out, pixels out per spp, crop): the ratio pairs (x, y) of the module's cases
CASES = {
    "same": (203, {1: 517, 4: 130}, None),
    "y152_x2": (152, {1: 1034, 4: 260}, None),
    "quarter": (51, {1: 130, 4: 33}, None),                     # K = 24 on both axes: the largest LDS footprint
    "x4": (812, {1: 2068, 4: 520}, None),
    "x16_crop33": (203, {1: 528, 4: 528}, 33),
    "y51": (51, {1: 517, 4: 130}, None),
}
KINDS = [("lanczos", name) for name in CASES] + [(k, name) for k in ("cubic", "linear") for name in ("y152_x2", "quarter")]


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _filled(shape):
    import torch
    return torch.full(shape, FILL, dtype=torch.int16, device="cuda").view(torch.uint16)


@pytest.fixture(scope="module")
def rasters():
    rng = np.random.default_rng(2026)
    out = {}
    for spp, w in WIDTH.items():
        img = rng.integers(0, 65536, (L, w * spp)).astype(np.uint16)
        img[3, 5:9] = 0
        img[100, 40:44] = 65535
        img[L - 1, -4:] = 65535
        out[spp] = img
    return out


class Tables:
    def __init__(self, kind, W, Wo, Ls, Lo):
        from opticalimageprocessor_amd import capi
        self.fx, self.tx = capi.rescale_taps(kind, W, Wo)
        self.fy, self.ty = capi.rescale_taps(kind, Ls, Lo)
        self.Kx, self.Ky = self.tx.shape[1], self.ty.shape[1]
        self.dev = [_cuda(a) for a in (self.fx, self.tx, self.fy, self.ty)]


def _run(ctx, img, spp, Wo, Lo, t, valid_min=0, windows=None, src_offset=0, dst_offset=0):
    """the whole output from one call or from the (out_row0, out_rows) windows, each on its own copy of exactly the source lines
    oip_rescale_src_range states; *_offset: samples by which the device rasters are moved off their 16-byte boundary"""
    from opticalimageprocessor_amd import capi
    Ls, W = img.shape[0], img.shape[1] // spp
    out = _filled((Lo * Wo * spp + 8,))
    keep = []
    for y0, n in windows or [(0, Lo)]:
        s0, sn = capi.rescale_src_range(Ls, Lo, t.Ky, y0, n)
        assert (s0, sn) == ref.src_range(Ls, Lo, t.Ky, y0, n)
        host = np.full(sn * W * spp + 8, FILL, np.uint16)
        host[src_offset:src_offset + sn * W * spp] = img[s0:s0 + sn].reshape(-1)
        buf = _cuda(host)
        keep.append(buf)
        ctx.rescale_u16(buf.data_ptr() + 2 * src_offset, s0, sn, W, Ls, spp, out.data_ptr() + 2 * (dst_offset + y0 * Wo * spp), y0, n, Wo, Lo,
                        t.dev[0], t.dev[1], t.Kx, t.dev[2], t.dev[3], t.Ky, valid_min)
    ctx.sync()
    flat = out.cpu().numpy()
    assert (flat[:dst_offset] == FILL).all() and (flat[dst_offset + Lo * Wo * spp:] == FILL).all()
    return flat[dst_offset:dst_offset + Lo * Wo * spp].reshape(Lo, Wo * spp)


def _three(Lo):
    a, b = (Lo // 3) | 1, (2 * Lo // 3) | 1
    return [(0, a), (a, b - a), (b, Lo - b)]


@pytest.mark.parametrize("spp", [1, 4])
@pytest.mark.parametrize("kind,case", KINDS)
def test_equals_restatement_whole_and_in_windows(ctx, rasters, kind, case, spp):
    Lo, wo, crop = CASES[case]
    img = rasters[spp] if crop is None else np.ascontiguousarray(rasters[spp][:, :crop * spp])
    W, Wo = img.shape[1] // spp, wo[spp]
    t = Tables(kind, W, Wo, L, Lo)
    want = ref.rescale(img, spp, Wo, Lo, t.fx, t.tx, t.fy, t.ty)
    got = _run(ctx, img, spp, Wo, Lo, t)
    assert np.array_equal(got, want), (np.argwhere(got != want)[:5], got[got != want][:5], want[got != want][:5])
    if case == "same":
        assert np.array_equal(got, img)
    cut = _run(ctx, img, spp, Wo, Lo, t, windows=_three(Lo))
    assert np.array_equal(cut, want), np.argwhere(cut != want)[:5]


@pytest.mark.parametrize("spp", [1, 4])
def test_bases_off_the_16_byte_boundary(ctx, rasters, spp):
    """lines that are multiples of 8 samples on bases that are not: the 2-byte loads and stores, the same bytes"""
    img = np.ascontiguousarray(rasters[spp][:, :512])           # 512 samples a line
    W, Wo, Lo = 512 // spp, 384 // spp, 152
    t = Tables("lanczos", W, Wo, L, Lo)
    want = ref.rescale(img, spp, Wo, Lo, t.fx, t.tx, t.fy, t.ty)
    for so, do in ((0, 0), (1, 0), (0, 3), (5, 1)):
        assert np.array_equal(_run(ctx, img, spp, Wo, Lo, t, src_offset=so, dst_offset=do), want), (so, do)


@pytest.mark.parametrize("spp", [1, 4])
@pytest.mark.parametrize("case", ["y152_x2", "quarter", "same"])
def test_no_data_takes_the_nearest_sample(ctx, rasters, case, spp):
    """a zero-filled border of 7 columns and 5 lines and a few isolated zeros at valid_min = 1: the restatement's bytes, zeros
    along the border stay zeros; the plain raster gives the bytes of valid_min 0"""
    Lo, wo, _ = CASES[case]
    W, Wo = WIDTH[spp], wo[spp]
    img = np.maximum(rasters[spp], 1).reshape(L, W, spp).copy()
    clean = img.reshape(L, W * spp).copy()
    img[:5] = 0
    img[-5:] = 0
    img[:, :7] = 0
    img[:, -7:] = 0
    for y, x, c in ((50, 60, 0), (51, 61, spp - 1), (120, 20, 0), (190, 100, spp // 2)):
        img[y, x, c] = 0
    img = img.reshape(L, W * spp)
    t = Tables("lanczos", W, Wo, L, Lo)
    want = ref.rescale(img, spp, Wo, Lo, t.fx, t.tx, t.fy, t.ty, valid_min=1)
    got = _run(ctx, img, spp, Wo, Lo, t, valid_min=1)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert np.array_equal(_run(ctx, img, spp, Wo, Lo, t, valid_min=1, windows=_three(Lo)), want)
    ny, nx = ref.nearest(L, Lo), ref.nearest(W, Wo)
    border = ((ny < 5) | (ny >= L - 5))[:, None] | ((nx < 7) | (nx >= W - 7))[None, :]
    g = got.reshape(Lo, Wo, spp)
    assert (g[border] == 0).all() and border.any()
    # without such samples the rule changes nothing
    assert np.array_equal(_run(ctx, clean, spp, Wo, Lo, t, valid_min=1), _run(ctx, clean, spp, Wo, Lo, t, valid_min=0))


def test_too_few_resident_lines_are_refused(ctx, rasters):
    from opticalimageprocessor_amd import capi
    img = rasters[1]
    W, Wo, Lo = 517, 1034, 152
    t = Tables("lanczos", W, Wo, L, Lo)
    s0, sn = capi.rescale_src_range(L, Lo, t.Ky, 41, 60)
    src, dst = _cuda(img[s0:s0 + sn]), _filled((60, Wo))
    args = lambda a, n: (src, a, n, W, L, 1, dst, 41, 60, Wo, Lo, t.dev[0], t.dev[1], t.Kx, t.dev[2], t.dev[3], t.Ky, 0)
    for a, n in ((s0 + 1, sn - 1), (s0, sn - 1), (s0 + 1, sn)):
        with pytest.raises(ValueError, match="source lines .* needed, .* resident"):
            ctx.rescale_u16(*args(a, n))
    ctx.rescale_u16(*args(s0, sn))
    ctx.sync()
    assert np.array_equal(dst.cpu().numpy(), ref.rescale(img, 1, Wo, Lo, t.fx, t.tx, t.fy, t.ty, rows=(41, 60)))


def test_invalid_arguments(ctx, rasters):
    img = rasters[1]
    t = Tables("linear", 517, 517, L, L)
    src, dst = _cuda(img), _filled((L, 517))
    ok = dict(src=src, src_row0=0, src_rows=L, W=517, L=L, spp=1, dst=dst, out_row0=0, out_rows=L, Wo=517, Lo=L, first_x=t.dev[0], taps_x=t.dev[1],
              Kx=t.Kx, first_y=t.dev[2], taps_y=t.dev[3], Ky=t.Ky, valid_min=0)
    ctx.rescale_u16(**ok)
    ctx.rescale_u16(**dict(ok, out_rows=0))                     # a no-op
    ctx.sync()
    assert np.array_equal(dst.cpu().numpy(), img)
    for bad in (dict(spp=2), dict(W=0), dict(Wo=0), dict(L=0), dict(Lo=0), dict(Kx=3), dict(Kx=26), dict(Ky=0), dict(valid_min=-1), dict(valid_min=65536),
                dict(dst=src), dict(src=None), dict(taps_x=None), dict(first_y=None), dict(out_row0=1), dict(out_rows=-1), dict(src_rows=L + 1),
                dict(Wo=129), dict(Wo=517 * 16 + 1), dict(Lo=50), dict(src=src.data_ptr() + 1)):
        with pytest.raises(ValueError):
            ctx.rescale_u16(**dict(ok, **bad))
