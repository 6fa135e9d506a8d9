"""GPU parity of the correlation path on the FFT plan routes and peak positions the product's own shapes never reach.

The planner (csrc/oip_fftplan.h: plan, split_axis, choose_kernel; csrc/fft.hip: launch_pass) hands out a specialised column
kernel per pass factor (kFast: F = 125, 128, 100, 160, 64, 32; plain, fused load `_pack`, fused store `_peak`), multi-pass
row transforms for rows longer than 4096 points (mode-0 row passes + cross_power_kernel with a two-digit x scramble), and
peak_window_kernel clamps its 5x5 window at the border of the surface.  test_gpu_correlation.py reaches none of these.
Here every case names the kernels it is there for and asserts, from the context's profile, that they ran.

Inputs.  a is uniform noise, b = np.roll(a, (sy, sx)); every (rows, cols) is its own optimal DFT size, so nothing is
padded, the roll is circular and the surface is a near-delta: the oracle's response is asserted > 0.9 per case and no
case is masked.  cv::phaseCorrelate returns the shift of b against a: the peak of the shifted surface is at
(py, px) = ((M >> 1) - sy mod M, (N >> 1) - sx mod N) and (dx, dy) = (N / 2 - cx, M / 2 - cy) -- for odd N that is
sx + 0.5, the reference's own convention.  The ground truth is therefore asserted on the peak cell: the oracle's arg-max
is (py, px), and round(N / 2 - dx), round(M / 2 - dy) of the GPU give the same cell.

Bars: test_gpu_correlation.py's (2e-4 px, 1e-4 response) against the float64 oracle; every case logs its measured deltas.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHIFT_TOL = 2e-4     # px, |GPU - oracle| on dx, dy
RESP_TOL = 1e-4      # absolute, on the response

CT, GEN = "fft_pass_ct_kernel_F%d%s", "fft_pass_kernel_F%d%s"


def _cuda(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()          # a copy: the shared base images are read-only


def _peak_cell(M, N, sy, sx):
    """cell of the shifted surface that holds the peak of (a, roll(a, (sy, sx)))"""
    return ((M >> 1) - sy) % M, ((N >> 1) - sx) % N


def _shift_for(M, N, py, px):
    return (M >> 1) - py, (N >> 1) - px


_PAIRS = {}


def _pair(rows, cols, integers=False):
    """the base image of a shape, made once: (host f32, device f32)"""
    key = (rows, cols, integers)
    if key not in _PAIRS:
        rng = np.random.default_rng(rows * 31 + cols)
        a = rng.integers(0, 4096, (rows, cols)).astype(np.float32) if integers else rng.uniform(0, 4095, (rows, cols)).astype(np.float32)
        a.setflags(write=False)
        _PAIRS[key] = a
    return _PAIRS[key]


def _rolled(a, sy, sx, broad=False):
    """b of the pair: a rolled by (sy, sx); broad: plus 0.4 of its four neighbouring rolls -- the cross-power spectrum keeps the
    phase of that blur only, and the surface becomes a peak whose four neighbours (circular ones included) carry weight"""
    b = np.roll(a, (sy, sx), axis=(0, 1))
    if broad:
        for oy, ox in ((0, 1), (1, 0), (0, -1), (-1, 0)):
            b = b + np.float32(0.4) * np.roll(a, (sy + oy, sx + ox), axis=(0, 1))
    return np.ascontiguousarray(b, np.float32)


def _oracle(a, b, sy, sx):
    """oracle result of the pair, after checking that the reference alone is decisive: peak where the roll puts it,
    response above 0.9"""
    from oracle import phasecorr as pc
    M, N = a.shape
    assert (pc.optimal_dft_size(M), pc.optimal_dft_size(N)) == (M, N)
    c = pc.correlation_surface(a, b)
    assert pc.surface_peak(c) == _peak_cell(M, N, sy, sx), (pc.surface_peak(c), _peak_cell(M, N, sy, sx))
    (wdx, wdy), wr = pc.centroid_of_surface(c)
    assert wr > 0.9, wr
    return wdx, wdy, wr


def _compare(parity_log, shape, shift, got, want, **extra):
    (M, N), (sy, sx) = shape, shift
    gdx, gdy, gr = got
    wdx, wdy, wr = want
    parity_log(rows=M, cols=N, sy=sy, sx=sx, shift_px=max(abs(gdx - wdx), abs(gdy - wdy)), response=abs(gr - wr),
               shift_bar=SHIFT_TOL, response_bar=RESP_TOL, **extra)
    assert abs(gdx - wdx) < SHIFT_TOL and abs(gdy - wdy) < SHIFT_TOL, ((gdx, gdy), (wdx, wdy))
    assert abs(gr - wr) < RESP_TOL, (gr, wr)
    py, px = _peak_cell(M, N, sy, sx)
    assert (round(M / 2.0 - gdy), round(N / 2.0 - gdx)) == (py, px), ((gdx, gdy), (py, px))


def _profiled(ctx, call):
    """run `call` with the context's profiler on -> (result, {kernel name: launches})"""
    ctx.profile_enable(True)
    try:
        ctx.profile_reset()
        out = call()
        prof = {k: v[1] for k, v in ctx.profile().items()}
    finally:
        ctx.profile_reset()
        ctx.profile_enable(False)
    return out, prof


def _assert_ran(prof, names):
    for name, launches in names.items():
        assert prof.get(name) == launches, "%s: %s launches expected; the profile has %s" % (name, launches, prof)


# (rows, cols, (sy, sx), {profile name: launches of one correlation}).  Column factors are split_axis(M, 256, 256), row
# factors split_axis(N, 256, 4096); kFast matches on (F, mode); the forward transform runs the column passes in factor
# order (first one `_pack`), the inverse in reverse order (last one -- the first factor -- `_peak`).
COLUMN_ROUTES = [
    # 10000 = 100 * 100
    (10000, 48, (-3, 5), {CT % (100, "_pack"): 1, CT % (100, ""): 2, CT % (100, "_peak"): 1}),
    # 25600 = 160 * 160
    (25600, 32, (4, -2), {CT % (160, "_pack"): 1, CT % (160, ""): 2, CT % (160, "_peak"): 1}),
    # 4096 = 64 * 64 (32-lane tiles: 48 columns are one full and one half tile)
    (4096, 48, (-5, -3), {CT % (64, "_pack"): 1, CT % (64, ""): 2, CT % (64, "_peak"): 1}),
    # 20000 = 125 * 160: F = 125 as the first factor
    (20000, 32, (6, 1), {CT % (125, "_pack"): 1, CT % (160, ""): 2, CT % (125, "_peak"): 1}),
    # 12800 = 100 * 128: F = 128 plain, not first
    (12800, 32, (-2, 7), {CT % (100, "_pack"): 1, CT % (128, ""): 2, CT % (100, "_peak"): 1}),
    # 16384 = 128 * 128: F = 128 first and not first; the last inverse pass is fft_col128_peak_kernel (profiled as _F128_peak)
    (16384, 32, (3, -4), {CT % (128, "_pack"): 1, CT % (128, ""): 2, CT % (128, "_peak"): 1}),
    # 640 = 20 * 32: generic first factor, F = 32 plain; 200-point rows run in the fused row stage
    (640, 200, (-7, 2), {GEN % (20, "_pack"): 1, CT % (32, ""): 2, GEN % (20, "_peak"): 1, "corr_rows_kernel": 1}),
    # 12500 = 100 * 125: F = 125 plain
    (12500, 16, (5, -1), {CT % (100, "_pack"): 1, CT % (125, ""): 2, CT % (100, "_peak"): 1}),
    # 243 x 125: one generic pass per axis, odd both ways (radix 3 only / radix 5 only); oracle bars, no route to name
    (243, 125, (-2, 3), {}),
]
# rows longer than 4096 points: two row passes per direction (the first in mode 0 with per-lane twiddles, the second over
# contiguous sub-rows) and cross_power_kernel between them, walking x by oip_pos_to_freq / oip_freq_to_pos
ROW_ROUTES = [
    # 5000 = 50 * 100 (kFast's F = 100 entry is a mode-0 kernel: the contiguous pass stays generic)
    (48, 5000, (3, -5), {GEN % (48, "_pack"): 1, GEN % (50, ""): 2, GEN % (100, ""): 2, "cross_power_kernel": 1, GEN % (48, "_peak"): 1}),
    # 8192 = 64 * 128: the mode-0 row pass is the specialised F = 64 kernel, on the x axis
    (20, 8192, (-2, 6), {GEN % (20, "_pack"): 1, CT % (64, ""): 2, GEN % (128, ""): 2, "cross_power_kernel": 1, GEN % (20, "_peak"): 1}),
    # 6000 = 75 * 80: radix 3 and 5
    (30, 6000, (4, 3), {GEN % (30, "_pack"): 1, GEN % (75, ""): 2, GEN % (80, ""): 2, "cross_power_kernel": 1, GEN % (30, "_peak"): 1}),
]
_ids = lambda routes: ["%dx%d" % r[:2] for r in routes]


@pytest.mark.parametrize("rows,cols,shift,names", COLUMN_ROUTES + ROW_ROUTES, ids=_ids(COLUMN_ROUTES + ROW_ROUTES))
def test_route_matches_oracle(ctx, oracle_mod, parity_log, rows, cols, shift, names):
    a = _pair(rows, cols)
    b = np.roll(a, shift, axis=(0, 1))
    want = _oracle(a, b, *shift)
    da, db = _cuda(a), _cuda(b)
    ((gdx, gdy), gr), prof = _profiled(ctx, lambda: ctx.phase_correlate_f32(da, db, rows, cols))
    _assert_ran(prof, dict(names, peak_window_kernel=1))
    _compare(parity_log, (rows, cols), shift, (gdx, gdy, gr), want)


@pytest.mark.parametrize("col0", [8, 3], ids=["aligned", "odd-offset"])
@pytest.mark.parametrize("rows,cols,shift,names", COLUMN_ROUTES, ids=_ids(COLUMN_ROUTES))
def test_route_through_the_u16_loader(ctx, oracle_mod, parity_log, rows, cols, shift, names, col0):
    """The same column routes with the u16 -> f32 conversion in the first pass' loader (oip_stt_correlate_windows): windows
    of larger rasters, pitch > cols.  col0 = 8 with a pitch that is a multiple of 8: 16-byte aligned rows -- the 128-point
    first pass of 16384 rows then runs fft_first_pass_up_kernel (wide loads; profiled under the same _F128_pack name);
    col0 = 3: the element-wise loader of the `_pack` kernels everywhere."""
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
    _assert_ran(prof, dict(names, peak_window_kernel=1))
    _compare(parity_log, (rows, cols), shift, tuple(got[0]), want, col0=col0)


# ---- peaks on the border of the surface --------------------------------------------------------------------------------
BORDER_SHAPES = [(400, 200), (243, 125), (1600, 3000)]       # even + fused rows; odd both ways, generic; two column passes + 3000-point rows


def _border_cells(M, N):
    """the four corners (3x3 window), the middle of the four edges (3x5 / 5x3) and the cells one and two in from every
    corner on its diagonal (4x4 and 5x5 touching the border): every way peak_window_kernel's window clamp and the wrap of
    the un-shifted row / column index at 0 and M - 1 / N - 1 can combine"""
    cells = []
    for d in (0, 1, 2):
        cells += [(d, d), (d, N - 1 - d), (M - 1 - d, d), (M - 1 - d, N - 1 - d)]
    cells += [(0, N // 2), (M - 1, N // 2), (M // 2, 0), (M // 2, N - 1)]
    return cells


def _clipped(M, N, cell):
    """cells whose 5x5 window is clipped; at 1600 x 3000 (0.6 s of oracle per case) only those on the border itself"""
    return min(cell[0], M - 1 - cell[0], cell[1], N - 1 - cell[1]) < (1 if M * N > 1000000 else 2)


# Every cell with the rolled pair alone: a near-delta, which tests the arg-max key, the wrap of the cell's own row / column
# and the cell count of the clipped window.  Its neighbours are 1e-5 of the peak, so what the window does with them hardly
# shows (measured on the oracle's surface: a centroid over a window that wraps around the surface instead of clamping moves
# by 3e-6 px at 1600 x 3000, 2e-4 .. 5e-4 at the small shapes).  The clipped windows therefore run a second time on the
# blurred pair (_rolled): its peak has neighbours of weight across the border, the reference clamps them away, and a window
# that wraps, or a cell read from the wrong side, moves the centroid by 4e-2 .. 6e-2 px and the response by 4e-2 .. 1e-1 --
# hundreds of times the bar.  Oracle float32 against float64 on these pairs: 3e-7 px, 2e-7 response; response 0.92 .. 1.04.
BORDER_CASES = [(M, N, cell, broad) for (M, N) in BORDER_SHAPES for broad in (False, True) for cell in _border_cells(M, N)
                if not broad or _clipped(M, N, cell)]


@pytest.mark.parametrize("rows,cols,cell,broad", BORDER_CASES,
                         ids=["%dx%d-y%d-x%d%s" % (m, n, c[0], c[1], "-broad" if b else "") for m, n, c, b in BORDER_CASES])
def test_border_peak_matches_oracle(ctx, oracle_mod, parity_log, rows, cols, cell, broad):
    shift = _shift_for(rows, cols, *cell)
    assert _peak_cell(rows, cols, *shift) == cell
    a = _pair(rows, cols)
    b = _rolled(a, *shift, broad=broad)
    want = _oracle(a, b, *shift)                 # asserts that the oracle's peak is `cell`: no drift into the interior
    (gdx, gdy), gr = ctx.phase_correlate_f32(_cuda(a), _cuda(b), rows, cols)
    _compare(parity_log, (rows, cols), shift, (gdx, gdy, gr), want, py=cell[0], px=cell[1], broad=broad)


# ---- degenerate surfaces on a routed shape ------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [7.0, 0.0], ids=["constant", "zero"])
def test_degenerate_pair_leaves_the_slots_empty(ctx, oracle_mod, value):
    """constant and all-zero pairs at 10000 x 48 (F = 100 column kernels): finite results with a vanishing response, like
    the oracle's; and the arg-max slots are left empty -- an ordinary correlation issued right behind a degenerate one
    gives the bits it gives on its own.  The response bar is test_phase_correlate_constant_images' 1e-4.  The constant case
    found a radix-5 butterfly that left rounding noise where five equal inputs cancel (GPU response 1.47e-4; the oracle's
    float32 form has the same effect, 1.2e-4; its float64 form 2e-18): bf5 (csrc/oip_fft_dev.h) is exact on equal inputs
    since, and the transform of a constant image is DC alone."""
    from oracle import phasecorr as pc
    rows, cols, shift = 10000, 48, (-3, 5)
    a = _pair(rows, cols)
    da, db = _cuda(a), _cuda(np.roll(a, shift, axis=(0, 1)))
    alone = ctx.phase_correlate_f32(da, db, rows, cols)
    flat = np.full((rows, cols), value, np.float32)
    (_, _), wr = pc.phase_correlate(flat, flat)
    dflat = _cuda(flat)
    (gdx, gdy), gr = ctx.phase_correlate_f32(dflat, dflat, rows, cols)
    after = ctx.phase_correlate_f32(da, db, rows, cols)
    print("\ndegenerate pair %g: GPU %r, oracle response %.3e" % (value, ((gdx, gdy), gr), wr))
    assert after == alone, (value, after, alone)
    assert np.isfinite([gdx, gdy, gr]).all(), (value, gdx, gdy, gr)
    assert abs(gr) < 1e-4 and abs(wr) < 1e-4, (value, gr, wr)
