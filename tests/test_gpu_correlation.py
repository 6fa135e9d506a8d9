"""GPU parity of the correlation path: window conversion, cv::resize cubic, cv::phaseCorrelate
and the two reference drivers (CalcSttParameters, CalcInterBandCorrelation), through the C ABI.

Tolerances.  Window conversion and resize follow OpenCV's f32 operation order and must be
bit-exact against the oracle.  phaseCorrelate's FFT is a different factorisation from both
OpenCV's and numpy's, so shifts are compared at SHIFT_TOL px and responses at RESP_TOL
(PARITY UNPINNED for these: OpenCV is absent; the oracle restates its published algorithm).
Round 3: the bars are about 10x what the MI355X measures (5e-5 px / 5e-6 on full scenes; every test logs its
own measured maximum through `parity_log`), far above float32 FFT rounding and 10-20x below round 2's bars;
the units a response mask leaves out of a shift comparison are counted and the count is asserted.
"""
import numpy as np
import pytest

import _synth

pytestmark = pytest.mark.gpu

SHIFT_TOL = 2e-4     # px, |GPU - oracle| on dx, dy
RESP_TOL = 1e-4      # absolute, on the response
# How many units each test's response mask (oracle response < 0.1 or < 0.05: no usable peak, the arg-max is decided by
# rounding noise) may leave out of the SHIFT comparison -- the counts the synthetic scenes produce, asserted so that a
# change which silently masks more units fails.  Responses are compared on every unit.
MASKED = {"interband_small": 11, "12288_wide": 0, "reference_unit_shape": 0, "spectral_route_64": 0, "spectral_route_400": 0,
          "straddling": 2}          # measured on the MI355X (profiles/r03_parity_deltas.jsonl)


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_window_u16_to_f32(ctx, oracle_mod):
    import torch
    rng = np.random.default_rng(5)
    img = rng.integers(0, 65536, (300, 517), dtype=np.uint16)
    out = torch.zeros(120, 200, dtype=torch.float32, device="cuda")
    ctx.window_u16_to_f32(_cuda(img), 517, 33, 317, 120, 200, out)
    ctx.sync()
    assert np.array_equal(out.cpu().numpy(), oracle_mod.window_u16_to_f32(img, 33, 317, 120, 200))


@pytest.mark.parametrize("sw,sh,dw,dh", [(307, 400, 1228, 1600), (75, 60, 300, 240), (341, 50, 1365, 200), (8, 8, 32, 32), (100, 30, 250, 45)])
def test_resize_cubic_bit_exact(ctx, oracle_mod, sw, sh, dw, dh):
    import torch
    rng = np.random.default_rng(sw + dh)
    src = rng.uniform(0, 4095, (sh, sw)).astype(np.float32)
    dst = torch.zeros(dh, dw, dtype=torch.float32, device="cuda")
    ctx.resize_cubic_f32(_cuda(src), sw, sh, dst, dw, dh)
    ctx.sync()
    want = oracle_mod.resize_cubic(src, dw, dh)
    got = dst.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.abs(got - want).max()


PC_SHAPES = [
    (400, 200, (5, 3)),        # no padding, single x pass
    (1600, 200, (-4, 7)),      # 1600 = 40*40 two column passes
    (250, 307, (3, -2)),       # padded to 250 x 320
    (16000, 200, (3, -1)),     # the stitch geometry (stitcher.h:175-180)
    (4000, 1250, (-6, 5)),     # 1250 = 2*5^4 rows
    (3000, 100, (0, 0)),       # identical images: peak at the centre
    (243, 125, (2, 1)),        # odd sizes both ways (3^5 x 5^3)
    (1600, 3000, (3, -1)),     # 3000-point rows, one spectrum; 801 line pairs: some workgroups take a second pair
]


@pytest.mark.parametrize("rows,cols,shift", PC_SHAPES)
def test_phase_correlate_matches_oracle(ctx, oracle_mod, parity_log, rows, cols, shift):
    from oracle import phasecorr as pc
    sx, sy = shift
    pad = 16
    sc = _synth.scene(rows + 2 * pad, cols + 2 * pad, seed=(rows + cols) % 97)
    a = np.ascontiguousarray(sc[pad:pad + rows, pad:pad + cols], dtype=np.float32)
    b = np.ascontiguousarray(sc[pad - sy:pad - sy + rows, pad - sx:pad - sx + cols], dtype=np.float32)
    (wdx, wdy), wr = pc.phase_correlate(a, b)
    (gdx, gdy), gr = ctx.phase_correlate_f32(_cuda(a), _cuda(b), rows, cols)
    parity_log(shift_px=max(abs(gdx - wdx), abs(gdy - wdy)), response=abs(gr - wr), shift_bar=SHIFT_TOL, response_bar=RESP_TOL)
    assert abs(gdx - wdx) < SHIFT_TOL and abs(gdy - wdy) < SHIFT_TOL, ((gdx, gdy), (wdx, wdy))
    assert abs(gr - wr) < RESP_TOL, (gr, wr)
    # ground truth: the peak is at the true integer shift; the 5x5 centroid around it is a
    # biased sub-pixel estimate (part of the behaviour to reproduce), so allow one pixel
    assert abs(gdx - sx) < 1.0 and abs(gdy - sy) < 1.0


def test_phase_correlate_constant_images(ctx, oracle_mod):
    """degenerate input: the spectrum is zero everywhere but DC, the surface is rounding noise
    around 0 and the peak position is arbitrary -- like the oracle, the result must be finite
    with a vanishing response (so the reference's threshold test rejects it)"""
    from oracle import phasecorr as pc
    a = np.full((120, 100), 7.0, np.float32)
    (_, _), wr = pc.phase_correlate(a, a)
    (gdx, gdy), gr = ctx.phase_correlate_f32(_cuda(a), _cuda(a), 120, 100)
    assert np.isfinite([gdx, gdy, gr]).all()
    assert abs(gr) < 1e-4 and abs(wr) < 1e-4


def test_stt_correlate_matches_oracle(ctx, oracle_mod, parity_log):
    from oracle import phasecorr as pc
    L, W, ov = 9000, 512, 200
    pan1, pan2 = _synth.ccd_pair(L, W, ov, (3, -2))
    table, mean = pc.calc_stt_parameters(pan1, pan2, sections=4, lines_per_section=1600, overlap_cols=ov, edge_cols=4)
    got = ctx.stt_correlate(_cuda(pan1), _cuda(pan2), W, L, 0, L, 4, 1600, ov, 4)
    tab = np.array([r[1:4] for r in table])
    parity_log(shift_px=np.abs(got[:, :2] - tab[:, :2]).max(), response=np.abs(got[:, 2] - tab[:, 2]).max(),
               shift_bar=SHIFT_TOL, response_bar=RESP_TOL)
    for s, row in enumerate(table):
        assert abs(got[s, 0] - row[1]) < SHIFT_TOL and abs(got[s, 1] - row[2]) < SHIFT_TOL, (s, got[s], row)
        assert abs(got[s, 2] - row[3]) < RESP_TOL
    # b = PAN2 cols [edge, ov) is the PAN1 window displaced by (sx - edge, sy) = (-1, -2)
    assert abs(got[:, 0].mean() + 1) < 0.6 and abs(got[:, 1].mean() + 2) < 0.6
    # a rank that holds only part of the strip reports NaN for the sections it does not own
    half = ctx.stt_correlate(_cuda(pan1[:4500]), _cuda(pan2[:4500]), W, L, 0, 4500, 4, 1600, ov, 4)
    assert np.allclose(half[:2], got[:2], atol=0, rtol=0) and np.isnan(half[2:]).all()
    with pytest.raises(ValueError, match="less than sections"):            # stitcher.h:75-77
        ctx.stt_correlate(_cuda(pan1), _cuda(pan2), W, L, 0, L, 10, 1600, ov, 0)


def test_interband_correlate_and_fit_match_oracle(ctx, oracle_mod, parity_log):
    import opticalimageprocessor_amd as oip
    from oracle import phasecorr as pc
    Lp, W, slices, sections, corr = 2400, 1280, 8, 2, 800
    shifts_true = [(2, -1), (1, 1), (-1, -2), (-2, 1)]
    pan, bands = _synth.pan_mss(Lp, W, shifts_true)
    want = pc.calc_interband_correlation(pan, bands, slices, sections, corr)
    planes = _cuda(np.stack(bands, 0))
    got = ctx.interband_correlate(_cuda(pan), Lp, 0, Lp, planes, bands[0].size, 0, Lp // 4, W, slices, sections, corr)
    assert got.shape == want.shape
    # Un-windowed phase correlation of a low-passed band against PAN has a broad peak that
    # competes with the border-induced peak at zero shift; where the response is tiny the
    # arg-max is decided by rounding noise.  Shifts are compared where the surface has a
    # usable peak; responses everywhere.
    ok = want[..., 2] >= 0.1
    d = np.abs(got[..., :2] - want[..., :2])[ok]
    dr = np.abs(got[..., 2] - want[..., 2]).max()
    parity_log(shift_px=d.max(), response=dr, units=int(ok.size), masked_out=int((~ok).sum()), shift_bar=SHIFT_TOL, response_bar=RESP_TOL)
    assert (~ok).sum() <= MASKED["interband_small"], (int((~ok).sum()), want[..., 2])
    assert d.max() < SHIFT_TOL, d.max()
    assert dr < RESP_TOL
    assert np.array_equal(got[..., 3], want[..., 3])
    thr = 0.1                      # --ibc-threshold for this small synthetic scene
    cx, cy = oip.filter_and_fit(got, thr, 5)
    wcx, wcy = pc.filter_and_fit(got, thr, 5)
    # compare the fitted polynomials where they are used: over the line, in pixels
    xs = np.linspace(0, W, 50)
    for b in range(4):
        assert np.abs((cx[b, 0] + cx[b, 1] * xs) - (wcx[b, 0] + wcx[b, 1] * xs)).max() < 1e-9
        assert np.abs((cy[b, 0] + cy[b, 1] * xs + cy[b, 2] * xs * xs) - (wcy[b, 0] + wcy[b, 1] * xs + wcy[b, 2] * xs * xs)).max() < 1e-9


def test_interband_argument_errors(ctx):
    import torch
    pan = torch.zeros(100 * 64, dtype=torch.uint16, device="cuda")
    with pytest.raises(ValueError, match="at lease 8 slice"):      # preproc.h:228-230
        ctx.interband_correlate(pan, 100, 0, 100, pan, 400, 0, 25, 64, slices=4, sections=1)
    with pytest.raises(ValueError, match="too many sections"):     # preproc.h:234-237
        ctx.interband_correlate(pan, 100, 0, 100, pan, 400, 0, 25, 64, slices=8, sections=5)


def _interband_vs_oracle(ctx, parity_log, Lp, W, slices, sections, corr, masked, min_resp=0.1):
    from oracle import phasecorr as pc
    shifts_true = [(2, -1), (1, 1), (-1, -2), (-2, 1)]
    pan, bands = _synth.pan_mss(Lp, W, shifts_true, seed=9)
    want = pc.calc_interband_correlation(pan, bands, slices, sections, corr)
    planes = _cuda(np.stack(bands, 0))
    got = ctx.interband_correlate(_cuda(pan), Lp, 0, Lp, planes, bands[0].size, 0, Lp // 4, W, slices, sections, corr)
    assert got.shape == want.shape and np.isfinite(got).all()
    ok = want[..., 2] >= min_resp
    d = np.abs(got[..., :2] - want[..., :2])[ok]
    dr = np.abs(got[..., 2] - want[..., 2]).max()
    parity_log(shift_px=d.max(), response=dr, units=int(ok.size), masked_out=int((~ok).sum()), shift_bar=SHIFT_TOL, response_bar=RESP_TOL)
    assert (~ok).sum() <= masked, (int((~ok).sum()), want[..., 2])
    assert d.max() < SHIFT_TOL, (d.max(), got[..., :3], want[..., :3])
    assert dr < RESP_TOL
    assert np.array_equal(got[..., 3], want[..., 3])
    return got


def test_interband_reference_unit_shape_matches_oracle(ctx, oracle_mod, parity_log):
    """The BASELINE unit shape itself -- 16000 x 3000 windows, x4 up-sampled 4000 x 750 bands -- through the
    specialised path: column transforms of the band windows themselves (4000 x 750, four side by side), the row stage
    that applies the x4 up-sampling of both axes to the band spectra (corr_rows_up_kernel), peak pass.  Nine slices: four paired runs
    and one single unit; the oracle (2.5 s per correlation: up-samples the image, then transforms it) checks the
    first pair and the single unit."""
    from oracle import phasecorr as pc
    Lp, W, slices = 16000, 27000, 9
    shifts_true = [(2, -1), (1, 1), (-1, -2), (-2, 1)]
    pan, bands = _synth.pan_mss(Lp, W, shifts_true, seed=9)
    planes = _cuda(np.stack(bands, 0))
    got = ctx.interband_correlate(_cuda(pan), Lp, 0, Lp, planes, bands[0].size, 0, Lp // 4, W, slices, 1, 16000)
    assert got.shape == (4, slices, 4) and np.isfinite(got).all()
    bc, sc = W // slices, W // slices // 4
    worst_s = worst_r = 0.0
    masked = 0
    for u in (0, 1, 8):
        a = oracle_mod.window_u16_to_f32(pan, 0, u * bc, Lp, bc)
        for b in range(4):
            small = oracle_mod.window_u16_to_f32(bands[b], 0, u * sc, Lp // 4, sc)
            (wdx, wdy), wr = pc.phase_correlate(a, oracle_mod.resize_cubic(small, bc, Lp))
            gdx, gdy, gr, gcx = got[b, u]
            worst_r = max(worst_r, abs(gr - wr))
            assert abs(gr - wr) < RESP_TOL, (u, b, gr, wr)
            if wr >= 0.05:
                worst_s = max(worst_s, abs(gdx - wdx), abs(gdy - wdy))
                assert abs(gdx - wdx) < SHIFT_TOL and abs(gdy - wdy) < SHIFT_TOL, (u, b, (gdx, gdy), (wdx, wdy))
            else:
                masked += 1
            assert gcx == u * bc + bc // 2
    parity_log(shift_px=worst_s, response=worst_r, units=12, masked_out=masked, shift_bar=SHIFT_TOL, response_bar=RESP_TOL)
    assert masked <= MASKED["reference_unit_shape"]


def test_spectral_upsampling_route_equals_the_image_route(ctx, oracle_mod, parity_log):
    """3000-column units take the x4 cubic up-sampling of the bands on their spectra (DFT_N(R s) = H DFT_n(s) + sum
    G_j s_j along an axis, exact): OIP_SPECTRAL_UP=2 (default) on both axes, =1 on the horizontal axis only (vertical
    taps as an image kernel), =0 keeps both in the image domain (vertical kernel + loader of the first FFT pass).
    All routes against each other (rounding only: 1e-4 px; measured 4e-6) and the default against the oracle, on a
    pair plus a single unit, at two line counts (64: one sweep of the row kernel; 400: several sweeps)."""
    import os
    from oracle import phasecorr as pc
    for rows, seed in ((64, 4), (400, 5)):
        W = 9000
        pan, bands = _synth.pan_mss(rows, W, [(2, -1), (1, 1), (-1, -2), (-2, 1)], seed=seed)
        dpan, dplanes = _cuda(pan), [_cuda(b) for b in bands]
        pp = [dpan[:, 3000 * u:] for u in range(3)]
        bp = [[dplanes[b][:, 750 * u:] for b in range(4)] for u in range(3)]
        res = {}
        try:
            for mode in ("0", "1", "2"):
                os.environ["OIP_SPECTRAL_UP"] = mode
                res[mode] = ctx.interband_correlate_units(pp, [W] * 3, bp, [W // 4] * 3, rows, 3000)
        finally:
            os.environ.pop("OIP_SPECTRAL_UP", None)
        default = ctx.interband_correlate_units(pp, [W] * 3, bp, [W // 4] * 3, rows, 3000)
        assert np.array_equal(default, res["2"])
        for mode in ("1", "2"):
            assert np.isfinite(res[mode]).all()
            d = np.abs(res[mode] - res["0"])
            assert d[..., :2].max() < 1e-4 and d[..., 2].max() < 1e-4, (rows, mode, d.max(axis=(0, 1)))
            assert d.max() > 0, "two routes gave identical bits: the switch did not switch"
        assert np.abs(res["2"] - res["1"]).max() > 0
        worst_s = worst_r = 0.0
        masked = 0
        for u in range(3):
            a = oracle_mod.window_u16_to_f32(pan, 0, 3000 * u, rows, 3000)
            for b in range(4):
                small = oracle_mod.window_u16_to_f32(bands[b], 0, 750 * u, rows // 4, 750)
                (wdx, wdy), wr = pc.phase_correlate(a, oracle_mod.resize_cubic(small, 3000, rows))
                gdx, gdy, gr = res["2"][u, b]
                worst_r = max(worst_r, abs(gr - wr))
                assert abs(gr - wr) < RESP_TOL, (rows, u, b, gr, wr)
                if wr >= 0.05:
                    worst_s = max(worst_s, abs(gdx - wdx), abs(gdy - wdy))
                    assert abs(gdx - wdx) < SHIFT_TOL and abs(gdy - wdy) < SHIFT_TOL, (rows, u, b, (gdx, gdy), (wdx, wdy))
                else:
                    masked += 1
        parity_log(rows=rows, shift_px=worst_s, response=worst_r, units=12, masked_out=masked,
                   routes_px=float(np.abs(res["2"] - res["0"])[..., :2].max()), shift_bar=SHIFT_TOL, response_bar=RESP_TOL)
        assert masked <= MASKED["spectral_route_%d" % rows]


def test_spectral_route_with_unaligned_windows(ctx):
    """window pointers that are not 16-byte (PAN) / 4-byte (bands) aligned take the generic loaders of the first PAN pass
    and of the band pack kernel: same results as the image-domain route on the same windows"""
    import os
    rows, W = 64, 9016
    pan, bands = _synth.pan_mss(rows, W, [(2, -1), (1, 1), (-1, -2), (-2, 1)], seed=6)
    dpan, dplanes = _cuda(pan), [_cuda(b) for b in bands]
    pp = [dpan[:, 3000 * u + 5:] for u in range(2)]                      # odd pixel offsets
    bp = [[dplanes[b][:, 750 * u + 1:] for b in range(4)] for u in range(2)]
    res = {}
    try:
        for mode in ("0", "2"):
            os.environ["OIP_SPECTRAL_UP"] = mode
            res[mode] = ctx.interband_correlate_units(pp, [W] * 2, bp, [W // 4] * 2, rows, 3000)
    finally:
        os.environ.pop("OIP_SPECTRAL_UP", None)
    d = np.abs(res["2"] - res["0"])
    assert np.isfinite(res["2"]).all() and 0 < d.max() < 1e-4, d.max(axis=(0, 1))


def test_interband_12288_wide_shape_matches_oracle(ctx, oracle_mod, parity_log):
    """slice width 1228 -> 1250-point rows (the reference's 12288-pixel strips): fused row stage for 1250"""
    _interband_vs_oracle(ctx, parity_log, 4000, 9824, 8, 1, 4000, MASKED["12288_wide"])


def test_vertical_spectral_route_of_the_12288_geometry(ctx, oracle_mod, parity_log):
    """1228-column units (the reference's 12288-wide strips, 1250-point padded rows): the horizontal taps run in the image
    domain on the band rows, the vertical x4 up-sampling is applied to the column transforms of the bands
    (corr_rows_v_kernel).  OIP_SPECTRAL_V=0 keeps the image-domain route (vertical kernel + FFT loader): the two routes
    against each other (rounding only) and the default against the oracle, which up-samples the image first -- on a pair
    plus a single unit at 64 and 400 lines, and on a pair at the full 16000 lines (oracle on the second unit)."""
    import os
    from oracle import phasecorr as pc
    for rows, nun, check in ((64, 3, (0, 1, 2)), (400, 3, (0, 1, 2)), (16000, 2, (1,))):
        W = 1228 * nun
        pan, bands = _synth.pan_mss(rows, W, [(2, -1), (1, 1), (-1, -2), (-2, 1)], seed=7 + rows % 5)
        dpan, dplanes = _cuda(pan), [_cuda(b) for b in bands]
        pp = [dpan[:, 1228 * u:] for u in range(nun)]
        bp = [[dplanes[b][:, 307 * u:] for b in range(4)] for u in range(nun)]
        try:
            os.environ["OIP_SPECTRAL_V"] = "0"
            image = ctx.interband_correlate_units(pp, [W] * nun, bp, [W // 4] * nun, rows, 1228)
        finally:
            os.environ.pop("OIP_SPECTRAL_V", None)
        got = ctx.interband_correlate_units(pp, [W] * nun, bp, [W // 4] * nun, rows, 1228)
        assert np.isfinite(got).all()
        d = np.abs(got - image)
        # shifts are compared where the surface has a usable peak: the 5x5 centroid divides by the window sum, so a unit with
        # a vanishing response (64-line units of this scene) amplifies the last-bit differences of the two routes
        usable = image[..., 2] >= 0.05
        assert usable.sum() >= usable.size // 2, image[..., 2]
        assert d[..., :2][usable].max() < 1e-4 and d[..., 2].max() < 1e-4, (rows, d.max(axis=(0, 1)), image[..., 2])
        assert d.max() > 0, "two routes gave identical bits: the switch did not switch"
        worst_s = worst_r = 0.0
        masked = 0
        for u in check:
            a = oracle_mod.window_u16_to_f32(pan, 0, 1228 * u, rows, 1228)
            for b in range(4):
                small = oracle_mod.window_u16_to_f32(bands[b], 0, 307 * u, rows // 4, 307)
                (wdx, wdy), wr = pc.phase_correlate(a, oracle_mod.resize_cubic(small, 1228, rows))
                gdx, gdy, gr = got[u, b]
                worst_r = max(worst_r, abs(gr - wr))
                assert abs(gr - wr) < RESP_TOL, (rows, u, b, gr, wr)
                if wr >= 0.05:
                    worst_s = max(worst_s, abs(gdx - wdx), abs(gdy - wdy))
                    assert abs(gdx - wdx) < SHIFT_TOL and abs(gdy - wdy) < SHIFT_TOL, (rows, u, b, (gdx, gdy), (wdx, wdy))
                else:
                    masked += 1
        parity_log(rows=rows, shift_px=worst_s, response=worst_r, units=4 * len(check), masked_out=masked,
                   routes_px=float(d[..., :2][usable].max()), routes_masked_out=int((~usable).sum()), shift_bar=SHIFT_TOL, response_bar=RESP_TOL)
        assert masked <= 4 * len(check) // 2


def test_vertical_upsampling_kernels_agree(ctx):
    """the sliding-window x4 vertical kernel and the generic one feed the FFT identical images: the whole
    correlation table must come out bit for bit the same"""
    import os
    Lp, W, slices = 3200, 2560, 8
    pan, bands = _synth.pan_mss(Lp, W, [(2, -1), (1, 1), (-1, -2), (-2, 1)], seed=3)
    planes = _cuda(np.stack(bands, 0))
    args = (_cuda(pan), Lp, 0, Lp, planes, bands[0].size, 0, Lp // 4, W, slices, 1, 3200)
    try:
        os.environ["OIP_V_GENERIC"] = "1"
        a = ctx.interband_correlate(*args)
    finally:
        os.environ.pop("OIP_V_GENERIC", None)
    b = ctx.interband_correlate(*args)
    assert np.array_equal(a, b)


# ---- parity evidence that can be had without OpenCV (PARITY UNPINNED stays) ---------------
def _straddling_scene(seed=21, W=2560, Lp=3200, sections=2):
    """PAN + four bands whose slices carry increasing noise: the unit responses spread over 0.0 .. 1.0, eight to
    eleven of sixteen per band above the reference's 0.4 threshold (IBCV_DEF_THRESHOLD), none within 0.01 of it.
    (seed 23, W 24000, Lp 1600, one section: the same on 3000-column slices -- the spectral up-sampling route --
    with five or six of eight units per band above the threshold, none within 0.007 of it.)"""
    slices, corr = 8, 1600
    pan, bands = _synth.pan_mss(Lp, W, [(2, -1), (1, 1), (-1, -2), (-2, 1)], seed=seed)
    rng = np.random.default_rng(seed)
    bw = W // 4 // slices
    amps = [0, 60, 140, 240, 360, 500, 650, 800]
    out = []
    for b in range(4):
        a = bands[b].astype(np.float64)
        for i in range(slices):
            a[:, i * bw:(i + 1) * bw] += rng.normal(0, amps[(i + 3 * b) % 8], (a.shape[0], bw))
        out.append(np.clip(np.rint(a), 0, 65535).astype(np.uint16))
    return pan, out, (Lp, W, slices, sections, corr)


def test_gpu_against_float32_and_float64_oracles(ctx, oracle_mod, parity_log):
    """Three implementations of the same algorithm on the same units: the GPU (f32, own mixed-radix FFT), the oracle
    with a float32 FFT (scipy.fft, single precision throughout like cv::dft) and the oracle with a float64 FFT.  The
    deltas are printed side by side: the GPU must sit as close to either oracle as the two oracles sit to each other,
    up to a small factor -- i.e. the tolerance brackets 'any float32 FFT', not a GPU defect."""
    from oracle import phasecorr as pc
    pan, bands, (Lp, W, slices, sections, corr) = _straddling_scene()
    w64 = pc.calc_interband_correlation(pan, bands, slices, sections, corr)
    w32 = pc.calc_interband_correlation(pan, bands, slices, sections, corr, fft="f32")
    planes = _cuda(np.stack(bands, 0))
    got = ctx.interband_correlate(_cuda(pan), Lp, 0, Lp, planes, bands[0].size, 0, Lp // 4, W, slices, sections, corr)
    ok = w64[..., 2] >= 0.1                      # units with a usable peak (see the note in the test above)
    d = lambda a, b: (np.abs(a[..., :2] - b[..., :2])[ok].max(), np.abs(a[..., 2] - b[..., 2]).max())
    g32, g64, o = d(got, w32), d(got, w64), d(w32, w64)
    print("\nshift / response deltas:  GPU vs f32 oracle %.2e px / %.2e   GPU vs f64 oracle %.2e px / %.2e   "
          "f32 oracle vs f64 oracle %.2e px / %.2e" % (g32 + g64 + o))
    parity_log(shift_px=g32[0], response=g32[1], vs_f64_shift_px=g64[0], vs_f64_response=g64[1], oracles_shift_px=o[0],
               oracles_response=o[1], units=int(ok.size), masked_out=int((~ok).sum()), shift_bar=SHIFT_TOL, response_bar=RESP_TOL)
    assert (~ok).sum() <= MASKED["straddling"]
    assert g32[0] < SHIFT_TOL and g64[0] < SHIFT_TOL and g32[1] < RESP_TOL and g64[1] < RESP_TOL
    # the GPU is not an outlier among float32 implementations: within 20x of the spread between the two oracles,
    # or under 1e-4 px / 1e-4 absolutely
    assert g64[0] < max(20 * o[0], 1e-4) and g64[1] < max(20 * o[1], 1e-4), (g64, o)


@pytest.mark.parametrize("scene", [dict(), dict(seed=23, W=24000, Lp=1600, sections=1)], ids=["image-route", "spectral-route"])
def test_valid_set_straddling_the_reference_threshold(ctx, oracle_mod, scene):
    """The reference keeps a unit when its response reaches 0.4 (preproc.h:492-512).  On a scene whose responses
    straddle that threshold the GPU and the oracle must keep the SAME units, and the polynomials fitted to the two
    kept sets must give maps that agree to 1/64 px over the whole line (half a 1/32-px phase step).  Once on
    320-column slices (up-sampling in the image domain) and once on 3000-column slices (up-sampling on the spectra)."""
    import opticalimageprocessor_amd as oip
    from oracle import phasecorr as pc
    pan, bands, (Lp, W, slices, sections, corr) = _straddling_scene(**scene)
    want = pc.calc_interband_correlation(pan, bands, slices, sections, corr)
    assert np.abs(want[..., 2] - 0.4).min() > 5e-3              # the scene itself keeps clear of the threshold
    planes = _cuda(np.stack(bands, 0))
    got = ctx.interband_correlate(_cuda(pan), Lp, 0, Lp, planes, bands[0].size, 0, Lp // 4, W, slices, sections, corr)
    thr = 0.4
    vg, vw = got[..., 2] >= thr, want[..., 2] >= thr
    assert np.array_equal(vg, vw)
    assert 5 <= vw.sum(1).min() and vw.sum(1).max() < slices * sections      # some kept, some dropped, in every band
    cx, cy = oip.filter_and_fit(got, thr, 5)
    wcx, wcy = pc.filter_and_fit(want, thr, 5)
    xs = np.arange(0, W, 4, dtype=np.float64)
    worst = 0.0
    for b in range(4):
        worst = max(worst, np.abs((cx[b, 0] + cx[b, 1] * xs) - (wcx[b, 0] + wcx[b, 1] * xs)).max() / 4,
                    np.abs((cy[b, 0] + cy[b, 1] * xs + cy[b, 2] * xs * xs) - (wcy[b, 0] + wcy[b, 1] * xs + wcy[b, 2] * xs * xs)).max() / 4)
    print("\nlargest map difference over the line: %.2e MSS px" % worst)
    assert worst < 1.0 / 64


def test_fast_cross_power_is_bounded_against_the_unfused_route(ctx):
    """The fused row stage forms interior cross-power bins with the hardware reciprocal and square root
    (cross_power_bin_fast); OIP_FUSED_ROWS=0 runs the same correlations through cross_power_kernel and cross_power_bin
    (correctly rounded double divisions, the reference's operation order), with separate row passes.  Same column
    transforms; the forward and inverse row transforms differ too (fused kernel against pass kernels): the difference in
    shift and response is what the approximation and the other row transforms cost."""
    import os
    pan, bands, (Lp, W, slices, sections, corr) = _straddling_scene(22, W=1600)      # 200-point rows: a fused row-stage shape
    planes = _cuda(np.stack(bands, 0))
    dpan = _cuda(pan)
    fast = ctx.interband_correlate(dpan, Lp, 0, Lp, planes, bands[0].size, 0, Lp // 4, W, slices, sections, corr)
    os.environ["OIP_FUSED_ROWS"] = "0"
    try:
        exact = ctx.interband_correlate(dpan, Lp, 0, Lp, planes, bands[0].size, 0, Lp // 4, W, slices, sections, corr)
    finally:
        del os.environ["OIP_FUSED_ROWS"]
    ok = exact[..., 2] >= 0.1
    ds = np.abs(fast[..., :2] - exact[..., :2])[ok].max()
    dr = np.abs(fast[..., 2] - exact[..., 2]).max()
    print("\ncross_power_bin_fast vs cross_power_bin: %.2e px, %.2e response" % (ds, dr))
    assert ds < 2e-4 and dr < 2e-5
    assert (fast[..., :3] != exact[..., :3]).any()          # the two paths really differ
