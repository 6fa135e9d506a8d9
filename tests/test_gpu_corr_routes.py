"""GPU: an inter-band call takes the route its planner states (csrc/oip_corrroute.h; oip_corr_route_describe).

Every case runs three 64-line units (a pair and a single one: two groups) of 3000 or 1228 columns under one setting of the
switches, and asserts the route from the description, from the context's profile that the kernels the description names ran
-- by name and count -- and that those of the other routes did not, and that oip_rows_window_geometry is the description's
window.  A switch that does not switch fails here by name, not by two result arrays that happen to differ.

Counts are profile scopes: one per launch but for corr_rows_v_kernel, whose scope holds a group's launches (one per unit).
64 lines are one column pass, so the search of the H and HV routes has no col_sel_F<n> passes, only col_sel_peak.
"""
import numpy as np
import pytest

import _synth
from test_gpu_fft_routes import _cuda, _profiled

pytestmark = pytest.mark.gpu

ROWS, UNITS, GROUPS = 64, 3, 2
SHIFTS = [(2, -1), (1, 1), (-1, -2), (-2, 1)]

# (columns, switches, route, window radius): the 64-line rows of the table of tests/cpp/corrroute_test.cpp
CASES = [
    (3000, {}, "HV", 8),
    (3000, {"OIP_ROWS_WINDOW": "0"}, "HV", -1),
    (3000, {"OIP_PEAK_PRUNE": "0"}, "HV", -1),
    (3000, {"OIP_SPECTRAL_UP": "1"}, "H", -1),
    (3000, {"OIP_SPECTRAL_UP": "0"}, "image", -1),
    (1228, {}, "V", -1),
    (1228, {"OIP_SPECTRAL_V": "0"}, "image", -1),
    (1228, {"OIP_SPECTRAL_UP": "0"}, "image", -1),
]
ROW_KERNELS = ("corr_rows_up_kernel", "corr_rows_v_kernel", "corr_rows_kernel", "cross_power_kernel")
PACK_KERNELS = ("pack_bands_kernel", "hpack_bands_kernel", "resize_cubic_v_kernel")

_SCENES = {}


def _units(cols):
    """the windows of the three units of a width, uploaded once: (PAN pointers, band pointers, pitches)"""
    if cols not in _SCENES:
        W = cols * UNITS
        pan, bands = _synth.pan_mss(ROWS, W, SHIFTS, seed=4 if cols == 3000 else 11)
        dpan, dplanes = _cuda(pan), [_cuda(b) for b in bands]
        pp = [dpan[:, cols * u:] for u in range(UNITS)]
        bp = [[dplanes[b][:, cols // 4 * u:] for b in range(4)] for u in range(UNITS)]
        _SCENES[cols] = (pp, bp, W, (dpan, dplanes))
    return _SCENES[cols][:3]


@pytest.mark.parametrize("cols,env,route,window", CASES, ids=["%d-%s" % (c, "-".join("%s=%s" % kv for kv in e.items()) or "default") for c, e, _, _ in CASES])
def test_call_takes_the_described_route(ctx, monkeypatch, cols, env, route, window):
    import torch
    import opticalimageprocessor_amd as oip
    for k in ("OIP_SPECTRAL_UP", "OIP_SPECTRAL_V", "OIP_FUSED_ROWS", "OIP_PEAK_PRUNE", "OIP_ROWS_WINDOW", "OIP_ROWS_WINDOW_POISON", "OIP_V_GENERIC"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    plan = oip.corr_route_describe(ROWS, cols, torch.cuda.get_device_properties(0).multi_processor_count)
    assert (plan["route"], plan["window"]) == (route, window), plan
    assert plan["row_kernel"] == {"HV": "corr_rows_up_kernel", "H": "corr_rows_up_kernel", "V": "corr_rows_v_kernel", "image": "corr_rows_kernel"}[route]
    assert plan["pack_kernel"] == {"HV": "pack_bands_kernel", "H": "resize_cubic_v_kernel", "V": "hpack_bands_kernel", "image": "resize_cubic_v_kernel"}[route]
    pp, bp, W = _units(cols)
    ctx.rows_window_stats()
    got, prof = _profiled(ctx, lambda: ctx.interband_correlate_units(pp, [W] * UNITS, bp, [W // 4] * UNITS, ROWS, cols))
    assert np.isfinite(got).all()
    assert ctx.rows_window_geometry() == (plan["tile_cols"], plan["tiles"], plan["window"])
    pairs, rerun = ctx.rows_window_stats()
    assert (pairs, rerun) == ((GROUPS, rerun) if window >= 0 else (0, 0)) and rerun <= GROUPS
    runs = GROUPS + rerun                       # a group that missed the stored window ran again in the same call
    # the row stage: once per group on the spectral routes, once per unit (per pair of output arrays) on the image route
    want = {k: 0 for k in ROW_KERNELS + PACK_KERNELS}
    want[plan["row_kernel"]] = UNITS if route == "image" else runs
    want[plan["pack_kernel"]] = runs
    for name, launches in want.items():
        assert prof.get(name, 0) == launches, "%s: %d launches expected; the profile has %s" % (name, launches, prof)
    tagged = lambda tag: sum(v for k, v in prof.items() if k.endswith(tag))
    # the band transforms: one column pass over the four side-by-side arrays of a group (HV, V), or one over each of a
    # group's quarter-width arrays, two per unit (H)
    assert tagged("_band") == (runs if route in ("HV", "V") else 0), prof
    assert tagged("_quarter") == (2 * UNITS if route == "H" else 0), prof
    # the peak search over tile lists belongs to the H and HV routes: select, peak pass, select, peak pass -- or, with
    # OIP_PEAK_PRUNE=0, everything in the first round
    searched = route in ("H", "HV")
    assert plan["lists"] == searched
    rounds = 1 if env.get("OIP_PEAK_PRUNE") == "0" else 2
    assert prof.get("col_sel_first_kernel", 0) == (runs if searched else 0), prof
    assert prof.get("col_sel_second_kernel", 0) == (runs if searched else 0), prof
    assert prof.get("col_sel_peak", 0) == (runs * rounds if searched else 0), prof
    assert prof.get("peak_window_kernel", 0) == (UNITS if route == "image" else runs), prof
