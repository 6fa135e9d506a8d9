"""Host proof that the checks of test_gpu_beyond_2g.py bite, at a scaled-down geometry with the same band layout
(_bigraster.SMALL: 64 x 240, offsets "wrap" at element 192 * 64 + 8 instead of 2^31; 47 lines lie wholly beyond it, as in the
device geometry).  Nothing here mutates a kernel: what a 32-bit offset would have produced is simulated on the restatement's
own result -- loads that wrap (a tail band computed from the lines at index - wrap) and, separately, stores that wrap (the tail
lands on the head, the tail keeps what the buffer held).  The checker the GPU tests use must pass the true result and reject
both.  Also here: the column-slab argument the GPU resampling test relies on, shown on the oracle alone."""
import numpy as np
import pytest

import _bigraster as br

GEO = br.SMALL
NAMES = ["rrc", "mss_split_rrc", "stitch_rows_f4", "stitch_rows_f3", "permute", "convolve_9x9_spp1", "convolve_3x3_spp1",
         "convolve_9x9_spp4", "convolve_3x3_spp4", "despike_spp1", "despike_spp4", "stitch_balanced_spp1_h4",
         "stitch_balanced_spp4_h0", "stitch_balanced_spp1_h0", "stitch_balanced_spp4_h1", "stitch_balanced_lines_spp1_h4",
         "stitch_balanced_lines_spp4_h0", "stitch_balanced_lines_spp1_h0", "stitch_balanced_lines_spp4_h1",
         "stitch_balanced_spp1_h3_scalar", "stitch_balanced_lines_spp1_h3_scalar"]


@pytest.fixture(scope="module")
def small_probes(oracle_mod):
    P = br.probes(GEO, oracle_mod, folds=(4, 3))
    assert sorted(P) == sorted(NAMES)
    return P


def test_geometries_cross_the_boundary_the_same_way():
    assert br.BIG.assert_crosses() == 65553 and br.BIG.W * br.BIG.L > br.TWO31
    assert 65552 * br.BIG.W < br.TWO31 < 65553 * br.BIG.W                      # line 65552 straddles 2^31
    assert br.SMALL.assert_crosses() == 193
    assert br.BIG.L - br.BIG.first_line_beyond == br.SMALL.L - br.SMALL.first_line_beyond == 47
    assert br.BIG.head == br.SMALL.head and br.BIG.L - br.BIG.tail[0] == br.SMALL.L - br.SMALL.tail[0]


@pytest.mark.parametrize("name", NAMES)
def test_checker_passes_the_truth_and_rejects_wrapped_offsets(small_probes, name):
    p = small_probes[name]
    xs = p.host_inputs()
    truth = p.ref(0, *xs)                                     # the restatement on the whole raster: affordable here
    bands, row = p.bands(), p.const_row()
    br.check_rows(truth, bands, row)                          # bands + halo + constant rows describe the whole output
    beyond = slice(GEO.assert_crosses(), GEO.L)
    # loads that wrap: every input's elements from `wrap` on are those at index - wrap
    wrapped = p.ref(0, *[br.wrapped_read(x, GEO.wrap) for x in xs])
    assert br.rejects(wrapped, bands, row)
    differ = float((wrapped[beyond] != truth[beyond]).mean())
    assert differ >= 0.5, differ                              # a condition on the seeds, not a measurement
    # stores that wrap (the output's own element index; a stitched line is wider than an input line)
    wrap_out = GEO.wrap * truth.shape[1] // GEO.W
    assert br.rejects(br.wrapped_store(truth, wrap_out, 0xABCD), bands, row)       # the buffer held a sentinel
    assert br.rejects(br.wrapped_store(truth, wrap_out, truth), bands, row)        # ... or, by bad luck, the right answer
    # the checker's other half -- tensors, compared where they live -- holds the same line (on the CPU here)
    import torch
    as_t = lambda a: torch.from_numpy(a.view(np.int16)).view(torch.uint16)      # noqa: E731
    br.check_rows(as_t(truth), bands, row, chunk=50)
    assert br.rejects(as_t(wrapped), bands, row) and br.rejects(as_t(br.wrapped_store(truth, wrap_out, truth)), bands, row)
    # a single wrong sample anywhere is enough
    for r in (GEO.head[1] + 5, GEO.L - 1, 0):
        bad = truth.copy()
        bad[r, -1] ^= 1
        assert br.rejects(bad, bands, row) and br.rejects(as_t(bad), bands, row)


# ---- the checks that do not go through check_rows: the same two questions, asked of what the GPU test compares ------------------
@pytest.mark.parametrize("spp", [1, 4])
def test_seam_moments_expectation_is_exact_and_a_wrapped_read_misses_it(spp):
    """br.expected_block_moments (closed form + band lines), which the GPU test holds the device totals to, equals
    _seam_lines_ref.block_moments of the whole rasters; the totals of rasters read through a wrapping offset differ in the last
    block -- the one that lies beyond `wrap` -- and in the strip's totals"""
    import _seam_lines_ref
    fold, B = 4 // spp, 40
    ins = br.seam_inputs(GEO, spp)
    left, right = (br.host_raster(GEO, n, c) for n, c in ins)
    want = br.expected_block_moments(GEO, ins, fold, spp, B, 1, 65534)
    nb = GEO.L // B
    assert (nb - 1) * B >= GEO.first_line_beyond and want.shape == (nb, 6, spp)
    assert np.array_equal(_seam_lines_ref.block_moments(left, right, fold, spp, B, 1, 65534), want)
    for wl, wr in ((br.wrapped_read(left, GEO.wrap), right), (left, br.wrapped_read(right, GEO.wrap))):
        got = _seam_lines_ref.block_moments(wl, wr, fold, spp, B, 1, 65534)
        assert not np.array_equal(got[-1], want[-1])
        assert not np.array_equal(got.sum(0, dtype=np.uint64), want.sum(0, dtype=np.uint64))


def test_merge_check_rejects_wrapped_offsets(oracle_mod):
    """the merge check: tiles cut from the probe raster must come back as the probe raster.  The oracle's merge of
    br.merge_tiles passes the checker; tiles read through a wrapping offset, or an output stored through one, do not."""
    vp, hp, sl, sc = 8, 2, 30, 32
    noises = [br.band_noise(GEO, k, 50) for k in (0, 1)]
    x = br.host_raster(GEO, noises)
    tiles = br.merge_tiles(x, vp, hp, sl, sc)
    bands = [(GEO.head[0], GEO.head[1], noises[0]), (GEO.tail[0], GEO.tail[1], noises[1])]
    truth = oracle_mod.merge_subimages_be16(tiles)
    br.check_rows(truth, bands, br.CONST)
    wrapped = oracle_mod.merge_subimages_be16(br.wrapped_read(tiles.reshape(GEO.L, GEO.W), GEO.wrap).reshape(tiles.shape))
    assert br.rejects(wrapped, bands, br.CONST)
    beyond = slice(GEO.assert_crosses(), GEO.L)
    assert float((wrapped[beyond] != truth[beyond]).mean()) >= 0.5
    assert br.rejects(br.wrapped_store(truth, GEO.wrap, 0xABCD), bands, br.CONST)
    assert br.rejects(br.wrapped_store(truth, GEO.wrap, truth), bands, br.CONST)


def test_lzw_check_rejects_wrapped_offsets():
    """the LZW check compares the strips of br.lzw_lines with _tiff.lzw_encode and the decoded payload with the image.  A coder
    that read its lines through a wrapping offset writes other bytes for every compared line from the straddling one on; a
    decoder that stored through one leaves an image that differs from the original."""
    import _tiff
    noises = [br.band_noise(GEO, k, 90) for k in (0, 1)]
    x = br.host_raster(GEO, noises)
    w = br.wrapped_read(x, GEO.wrap)
    lines = br.lzw_lines(GEO)
    assert lines == (0, 192, 193, 239) and br.lzw_lines(br.BIG) == (0, 65552, 65553, 65599)

    def strip(img, r, spp=4):
        d = img[r:r + 1].copy()
        d[:, spp:] = (img[r:r + 1, spp:].astype(np.int32) - img[r:r + 1, :-spp].astype(np.int32)).astype(np.uint16)
        return _tiff.lzw_encode(d.astype("<u2").tobytes())
    assert strip(w, lines[0]) == strip(x, lines[0])
    for r in lines[1:]:
        assert strip(w, r) != strip(x, r), r
    assert not np.array_equal(br.wrapped_store(x, GEO.wrap, 0xABCD), x) and not np.array_equal(br.wrapped_store(x, GEO.wrap, x), x)


@pytest.mark.parametrize("ky,kx,spp,valid_min", [(9, 9, 1, 1), (3, 3, 4, 1), (5, 7, 1, 300), (3, 9, 4, 0), (9, 3, 1, 65535)])
def test_fast_convolve_is_the_yardstick(ky, kx, spp, valid_min):
    """br.convolve, which the probes use on the 32760-wide bands, against _mtfc_ref.convolve: taps at the 32767 bound, no data
    and saturated samples, images shorter than the kernel (the replicate border on both sides at once)"""
    import _mtfc_ref
    rng = np.random.default_rng(ky * 10 + kx + spp)
    for lines in (1, 3, 40):
        img = rng.integers(0, 65536, (lines, 24 * spp), dtype=np.uint16)
        img[rng.random(img.shape) < 0.1] = 0
        for taps in (_mtfc_ref.random_taps(ky, kx, 3), br.dc_taps(9, 1)[:ky, :kx]):
            assert np.array_equal(br.convolve(img, taps, valid_min, spp), _mtfc_ref.convolve(img, taps, valid_min, spp))


def test_wrapped_models():
    x = np.arange(20, dtype=np.uint16).reshape(4, 5)
    assert br.wrapped_read(x, 12).reshape(-1).tolist() == list(range(12)) + list(range(8))
    assert br.wrapped_store(x, 12, 99).reshape(-1).tolist() == list(range(12, 20)) + [8, 9, 10, 11] + [99] * 8


@pytest.mark.parametrize("dx,dy", [(3.3828125, -1.6171875), (-2.2578125, 2.3984375)])
def test_resampler_on_column_slabs_equals_the_whole(oracle_mod, dx, dy):
    """oracle.prestitch of a 300-wide image against itself on three 96-column slabs (sections of 300 lines, three of them):
    equal on the columns br.slab_columns keeps, through the image's own edges.  The shifts are multiples of 1/128, so x + dx is
    exact in fp32 at any column under 32768: a slab's local column index changes no phase."""
    W, L = 300, 700
    rng = np.random.default_rng(17)
    src = rng.integers(0, 4096, (L, W)).astype(np.uint16)
    src[::97] = 65535
    whole, _ = oracle_mod.prestitch(src, dx, dy, 300, 327)
    assert np.count_nonzero(whole) > whole.size // 2
    for c0, c1 in br.slabs(W):
        a, b = br.slab_columns(c0, c1, W, dx)
        part, _ = oracle_mod.prestitch(np.ascontiguousarray(src[:, c0:c1]), dx, dy, 300, 327)
        assert np.array_equal(part[:, a - c0:b - c0], whole[:, a:b]), (c0, c1)
        # and the margin is needed on the side the taps reach over: without it the slab's border shows
        if dx > 0 and c1 < W:
            assert not np.array_equal(part[:, -2:], whole[:, c1 - 2:c1])
        if dx < 0 and c0 > 0:
            assert not np.array_equal(part[:, :2], whole[:, c0:c0 + 2])
    assert br.slabs(W)[1][0] % 8 != 0
