"""GPU parity of the correlation path on every class of plan the FFT planner (csrc/oip_fftplan.h) can emit and
test_gpu_fft_routes.py does not reach: the generic kernel with lane tiles of V = 4, 2 and 1 transforms (single-pass rows of
569 .. 4096 points, radix chains of up to seven stages), generic column factors of 156 .. 256 points (V = 16), three column
passes (46875 and 64800 rows: a middle pass with O1 > 1 and O2 > 1, inter-pass twiddle rows at two T, three digits per row
index, peak_window_kernel over a three-pass remainder) and two-pass rows of 256 * 256 points.

Every case states its class -- per pass (axis, F, kernel kind, log2 V, radix count) -- and asserts it against the product's own
statement of the plan, oip_fft_plan_describe: where the planner changes, the case fails here and the table is moved so that
every class keeps a case.  The kernels a case is there for are then asserted from the context's profile, by name and F.

Inputs, oracle, bars and conditions are those of test_gpu_fft_routes.py (its _pair, _rolled, _oracle, _compare): a is uniform
noise and b = roll(a, (sy, sx)); each case runs on that near-delta pair and on the blurred pair (_rolled(broad=True)), whose
four neighbours carry 0.3 of the peak, so that a cell error of 1e-3 moves the centroid by about 1e-3 px instead of 1e-8.  The
peak is kept two cells off every border (border peaks: test_border_peak_matches_oracle).  _oracle asserts on the reference alone
that the peak is at the intended cell and the response above 0.9.  Bars: 2e-4 px and 1e-4 response against the float64 oracle;
on the blurred pair also the GPU within 20x of the float32 oracle's distance from the float64 one, or under 1e-4.
Oracle float32 against float64 on these cases: at most 1.5e-7 px (near-delta), 1.3e-5 px (blurred, worst at 3750 columns), 2.4e-7
response.  Shapes of fewer than 6 rows or columns are left out: the oracle's own response on them is 0.2 .. 0.6.
"""
import functools

import numpy as np
import pytest

import _synth
from test_gpu_fft_routes import CT, GEN, RESP_TOL, SHIFT_TOL, _assert_ran, _compare, _cuda, _oracle, _pair, _profiled, _rolled

pytestmark = pytest.mark.gpu

G, C = "generic", "ct"
_COL16 = ("x", 16, G, 5, 2)         # the 16-point row pass of the column cases


def _rows(cls, rows, cols, shift, ycls, nradix):
    """a single-pass row case: (y pass of `rows` points, x pass of `cols` points in tile class `cls`)"""
    return ("rows-V%d" % (1 << cls), rows, cols, shift, [("y", rows) + ycls, ("x", cols, G, cls, nradix)])


# (class, rows, cols, (sy, sx), [(axis, F, kind, log2 V, radix count) per pass, forward order])
PLAN_CLASSES = [
    # rows, generic, V = 4: 10 vectors make tiles of 4, 4 and 2; 729 is six radix-3 stages
    _rows(2, 10, 576, (1, -7), (G, 5, 2), 4),
    _rows(2, 6, 729, (1, 5), (G, 5, 2), 6),
    _rows(2, 10, 1024, (-2, 9), (G, 5, 2), 4),
    # rows, generic, V = 2: 9 vectors leave a tile of one; 1458 is seven stages
    _rows(1, 9, 1080, (2, -3), (G, 5, 2), 5),
    _rows(1, 9, 1458, (-1, 8), (G, 5, 2), 7),
    _rows(1, 9, 1600, (-2, -9), (G, 5, 2), 4),
    # rows, generic, V = 1 (Vp = 1, the other branch of choose_kernel)
    _rows(0, 8, 1728, (1, 6), (G, 5, 1), 5),
    _rows(0, 8, 2187, (-1, -4), (G, 5, 1), 7),
    _rows(0, 8, 3125, (2, 9), (G, 5, 1), 5),
    _rows(0, 8, 3750, (1, -8), (G, 5, 1), 6),
    _rows(0, 8, 3888, (-1, 3), (G, 5, 1), 7),
    _rows(0, 8, 4050, (2, -5), (G, 5, 1), 7),
    _rows(0, 8, 4096, (1, 7), (G, 5, 1), 4),
    _rows(0, 6, 3072, (1, -9), (G, 5, 2), 5),
    # columns, generic, V = 16: 16 columns are one full lane tile, 24 a full and a partial one, 40 two full and a partial one
    ("cols-V16", 200, 16, (-7, 3), [("y", 200, G, 4, 3), _COL16]),          # 200 is a kFast factor only as a row pass
    ("cols-V16", 216, 16, (30, -2), [("y", 216, G, 4, 4), _COL16]),
    ("cols-V16", 225, 16, (-41, 4), [("y", 225, G, 4, 4), _COL16]),
    ("cols-V16", 240, 16, (55, -5), [("y", 240, G, 4, 4), _COL16]),
    ("cols-V16", 250, 16, (-100, 1), [("y", 250, G, 4, 4), _COL16]),
    ("cols-V16", 256, 16, (90, -3), [("y", 256, G, 4, 3), _COL16]),
    ("cols-V16", 162, 16, (-33, 5), [("y", 162, G, 4, 5), _COL16]),
    ("cols-V16", 192, 40, (61, -9), [("y", 192, G, 4, 3), ("x", 40, G, 5, 2)]),
    ("cols-V16", 180, 24, (-50, 7), [("y", 180, G, 4, 4), ("x", 24, G, 5, 2)]),
    # three column passes: 25 * 25 * 75 and 36 * 36 * 50, both generic -- the only two such lengths the correlation entries take:
    # they refuse more than 65535 lines (see test_taller_three_pass_plans_are_refused), and every three-pass length with a
    # specialised factor (131072 = 32 * 32 * 128, 98304 = 32 * 32 * 96) lies above that
    ("cols-3pass", 46875, 16, (-11003, 4), [("y", 25, G, 5, 2), ("y", 25, G, 5, 2), ("y", 75, G, 5, 3), _COL16]),
    ("cols-3pass", 64800, 16, (20011, -3), [("y", 36, G, 5, 3), ("y", 36, G, 5, 3), ("y", 50, G, 5, 3), _COL16]),
    # two-pass rows whose factors are both 256: a generic mode-0 row pass at V = 16
    ("rows-256x256", 8, 65536, (1, -6), [("y", 8, G, 5, 1), ("x", 256, G, 4, 3), ("x", 256, G, 4, 3)]),
]
_id = lambda c: "%s-%dx%d" % c[:3]
COLUMN_CLASSES = [c for c in PLAN_CLASSES if c[0].startswith("cols")]
FUSED_ROWS = (3000, 1250, 200)      # row lengths of the fused row stage (corr_rows_kernel): none of the cases has one


def _class_of(rows, cols):
    import opticalimageprocessor_amd as oip
    return [(p["axis"], p["F"], p["kind"], p["vshift"], len(p["radix"])) for p in oip.fft_plan_describe(rows, cols)]


def _kernels_of(passes):
    """profile name -> launches of one correlation of a pair, from the passes of its plan: the forward transform runs the column
    passes in order (the first one `_pack`), then the row passes; cross_power_kernel; the inverse runs them in reverse order
    (the last one -- the first column factor -- `_peak`); peak_window_kernel"""
    names = {"cross_power_kernel": 1, "peak_window_kernel": 1}
    first = True
    for axis, F, kind, _, _ in passes:
        fmt = CT if kind == C else GEN
        if axis == "y" and first:
            names[fmt % (F, "_pack")] = names.get(fmt % (F, "_pack"), 0) + 1
            names[fmt % (F, "_peak")] = names.get(fmt % (F, "_peak"), 0) + 1
            first = False
        else:
            names[fmt % (F, "")] = names.get(fmt % (F, ""), 0) + 2
    return names


def _stated(cls, rows, cols, passes):
    """the case's class against the product's statement of the plan; and the case really is of its class"""
    assert _class_of(rows, cols) == passes, "the planner states another plan for %d x %d: %s" % (rows, cols, _class_of(rows, cols))
    assert cols not in FUSED_ROWS
    xs, ys = [p for p in passes if p[0] == "x"], [p for p in passes if p[0] == "y"]
    if cls.startswith("rows-V"):
        assert len(xs) == 1 and xs[0][2] == G and 1 << xs[0][3] == int(cls[6:])
    elif cls == "cols-V16":
        assert len(ys) == 1 and ys[0][2] == G and ys[0][3] == 4 and 156 <= ys[0][1] <= 256
    elif cls == "cols-3pass":
        assert len(ys) == 3
    else:
        assert [p[1:4] for p in xs] == [(256, G, 4)] * 2
    return _kernels_of(passes)


@pytest.mark.parametrize("broad", [False, True], ids=["delta", "broad"])
@pytest.mark.parametrize("cls,rows,cols,shift,passes", PLAN_CLASSES, ids=[_id(c) for c in PLAN_CLASSES])
def test_plan_class_matches_oracle(ctx, oracle_mod, parity_log, cls, rows, cols, shift, passes, broad):
    from oracle import phasecorr as pc
    names = _stated(cls, rows, cols, passes)
    a = _pair(rows, cols)
    b = _rolled(a, *shift, broad=broad)
    want = _oracle(a, b, *shift)
    da, db = _cuda(a), _cuda(b)
    ((gdx, gdy), gr), prof = _profiled(ctx, lambda: ctx.phase_correlate_f32(da, db, rows, cols))
    _assert_ran(prof, names)
    extra = {}
    if broad:
        (fdx, fdy), fr = pc.phase_correlate(a, b, fft="f32")
        extra = dict(oracles_shift_px=max(abs(fdx - want[0]), abs(fdy - want[1])), oracles_response=abs(fr - want[2]))
    _compare(parity_log, (rows, cols), shift, (gdx, gdy, gr), want, plan_class=cls, broad=broad, **extra)
    if broad:       # not an outlier among float32 implementations (test_gpu_against_float32_and_float64_oracles)
        gs, gresp = max(abs(gdx - want[0]), abs(gdy - want[1])), abs(gr - want[2])
        assert gs < max(20 * extra["oracles_shift_px"], 1e-4) and gresp < max(20 * extra["oracles_response"], 1e-4), (gs, gresp, extra)


@pytest.mark.parametrize("col0", [8, 3], ids=["aligned", "odd-offset"])
@pytest.mark.parametrize("cls,rows,cols,shift,passes", COLUMN_CLASSES, ids=[_id(c) for c in COLUMN_CLASSES])
def test_plan_class_through_the_u16_loader(ctx, oracle_mod, parity_log, cls, rows, cols, shift, passes, col0):
    """the column classes with the u16 -> f32 conversion in the first pass' loader (oip_stt_correlate_windows), as
    test_route_through_the_u16_loader does it: windows of larger rasters at a 16-byte aligned and at an odd column"""
    names = _stated(cls, rows, cols, passes)
    a = _pair(rows, cols, integers=True)
    b = np.roll(a, shift, axis=(0, 1))
    want = _oracle(a, b, *shift)
    pitch = (cols + 7) // 8 * 8 + 24
    rng = np.random.default_rng(cols + col0)
    rasters = []
    for img in (a, b):
        r = rng.integers(0, 4096, (rows, pitch)).astype(np.uint16)      # what surrounds the window must not matter
        r[:, col0:col0 + cols] = img.astype(np.uint16)
        rasters.append(_cuda(r))
    wa, wb = rasters[0][:, col0:], rasters[1][:, col0:]
    assert (wa.data_ptr() % 16 == 0) == (col0 == 8) and wa.data_ptr() == rasters[0].data_ptr() + 2 * col0
    got, prof = _profiled(ctx, lambda: ctx.stt_correlate_windows([wa], [pitch], [wb], [pitch], rows, cols))
    _assert_ran(prof, names)
    _compare(parity_log, (rows, cols), shift, tuple(got[0]), want, plan_class=cls, col0=col0)


@pytest.mark.parametrize("rows", [72000, 98304, 131072])
def test_taller_three_pass_plans_are_refused(ctx, rows):
    """the planner plans these lengths (40 * 40 * 45; 32 * 32 * 96; 32 * 32 * 128, all specialised), the correlation entries
    refuse them: more than 65535 lines.  Should that limit move, these plans need cases in PLAN_CLASSES first."""
    import opticalimageprocessor_amd as oip
    assert len([p for p in oip.fft_plan_describe(rows, 16) if p["axis"] == "y"]) == 3
    a = _cuda(_pair(rows, 16))
    with pytest.raises(NotImplementedError, match="more than 65535 rows"):
        ctx.phase_correlate_f32(a, a, rows, 16)
    r = _cuda(_pair(rows, 16, integers=True).astype(np.uint16))
    with pytest.raises(NotImplementedError, match="65535 lines"):
        ctx.stt_correlate_windows([r], [16], [r], [16], rows, 16)


# ---- the new row classes under the inter-band driver ----------------------------------------------------------------------
SHIFTS = [(2, -1), (1, 1), (-1, -2), (-2, 1)]          # test_gpu_peak_prune.py's
# (W, slices, sections, lines, seed, [class of the units' plan]): 768-column units are V = 4, 2048-column units V = 1.  Oracle
# responses 0.47 .. 1.04, no unit below 0.1; oracle float32 against float64 at most 3.8e-5 px and 9.1e-6 response.
INTERBAND = [
    (6144, 8, 1, 64, 4, [("y", 64, C, 5, 2), ("x", 768, G, 2, 4)]),
    (6144, 8, 1, 400, 5, [("y", 20, G, 5, 2), ("y", 20, G, 5, 2), ("x", 768, G, 2, 4)]),
    (16384, 8, 1, 64, 4, [("y", 64, C, 5, 2), ("x", 2048, G, 0, 4)]),
]


@functools.lru_cache(maxsize=None)
def _scene(rows, W, seed):
    pan, bands = _synth.pan_mss(rows, W, SHIFTS, seed=seed)
    pan.setflags(write=False)
    for b in bands:
        b.setflags(write=False)
    return pan, bands


@pytest.mark.parametrize("W,slices,sections,rows,seed,passes", INTERBAND, ids=["%d-%dx%d" % (c[0], c[3], c[0] // c[1]) for c in INTERBAND])
def test_interband_on_the_row_classes(ctx, oracle_mod, parity_log, W, slices, sections, rows, seed, passes):
    from oracle import phasecorr as pc
    cols = W // slices
    assert _class_of(rows, cols) == passes, _class_of(rows, cols)
    pan, bands = _scene(rows, W, seed)
    want = pc.calc_interband_correlation(pan, bands, slices, sections, rows)
    assert (want[..., 2] >= 0.1).all(), want[..., 2]                # masked count 0: shifts are compared on every unit
    planes = _cuda(np.stack(bands, 0))
    dpan = _cuda(pan)
    got, prof = _profiled(ctx, lambda: ctx.interband_correlate(dpan, rows, 0, rows, planes, bands[0].size, 0, rows // 4, W, slices, sections, rows))
    assert got.shape == want.shape and np.isfinite(got).all()
    row_pass = GEN % (cols, "")                 # the driver may tag the name: a prefix
    assert any(k.startswith(row_pass) and n > 0 for k, n in prof.items()), "%s did not run; the profile has %s" % (row_pass, prof)
    ds, dr = np.abs(got[..., :2] - want[..., :2]).max(), np.abs(got[..., 2] - want[..., 2]).max()
    parity_log(rows=rows, cols=cols, shift_px=ds, response=dr, units=int(want[..., 2].size), masked_out=0, shift_bar=SHIFT_TOL, response_bar=RESP_TOL)
    assert ds < SHIFT_TOL, (ds, got[..., :3], want[..., :3])
    assert dr < RESP_TOL, dr
    assert np.array_equal(got[..., 3], want[..., 3])
