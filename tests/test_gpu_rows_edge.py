"""GPU: the row stage of the spectral correlation evaluates the exact formulas of its two edge columns (kx = 0 and N / 2:
divSpectrums' double-precision divisions and square root) in four lanes side by side instead of in series in one lane
("Edge columns in parallel lanes") -- and changes no bit of any result.

Every lane runs the statements of the serial block on the same operands, so the results must equal what the parent commit
returned for the same calls: they are constants below.  Scenes and helpers are those of tests/test_gpu_rows_window.py
(3000 columns).  Ordinary scenes cannot tell the exact formulas from the fast ones of the interior bins (1e-7 in 2 of 3000
bins per line): the banded scene below can."""
import functools

import numpy as np
import pytest

from test_gpu_correlation import RESP_TOL, SHIFT_TOL
from test_gpu_rows_window import N, _scene, _units_of, _with_env

pytestmark = pytest.mark.gpu

# One switch per instance of corr_rows_up_kernel: <512, true, true> as built, <512, true, false> with every column stored,
# <512, false, false> with the vertical taps in the image domain.
MODES = {"built": None, "window0": ("OIP_ROWS_WINDOW", "0"), "up1": ("OIP_SPECTRAL_UP", "1")}

# interband_correlate_units on three units (a pair and a single) of the scene, [unit][band][dx, dy, response] as float64
# hex, printed by the parent commit 148e434 for the same calls.  The single unit run alone returned the bits of row 2, and
# "window0" those of "built", in the parent as well.  Equality is expected: if a value differs, find out why before
# touching the constant.
PARENT = {
    (64, 4, "built"):
        "0x1.d5635a85e3000p+0 -0x1.1e34b7ddf1740p-1 0x1.868504bf258bfp-1 0x1.f1f8c37a74000p-2 0x1.f4b48c11fc580p-2 0x1.9c42c9fbe76c9p-1 "
        "-0x1.10404fb057800p-1 -0x1.186e2f61198a0p+0 0x1.2a468289e60f0p-1 -0x1.110cecf017c00p+0 0x1.dcc84b5ad4040p-2 0x1.3448e16041893p-1 "
        "0x1.1d40b4a4e9800p+0 -0x1.f7b3ae25c9700p-2 0x1.297422f72015ep-1 0x1.0bab429c9b800p-1 0x1.0f05aee604080p-1 0x1.94db717e4b17ep-1 "
        "-0x1.1811b2a426000p-1 -0x1.0f3c861476740p+0 0x1.25732170a3d71p-1 -0x1.19e47f1a66c00p+0 0x1.15b8cb79351e0p-1 0x1.2c642885cd7b9p-1 "
        "0x1.014371a9ad800p+0 -0x1.1b188662fb940p-1 0x1.320607fa89e61p-1 0x1.0ab51d75c8000p-1 0x1.fd8fd88a457c0p-2 0x1.98f603d194238p-1 "
        "-0x1.093d24349c000p-1 -0x1.152810bfdb2e0p+0 0x1.2aedf59f0fb39p-1 -0x1.b044e03cabc00p+0 0x1.d797bb38ffd80p-2 0x1.fdce15bfd44f3p-1",
    (64, 4, "up1"):
        "0x1.d5635b76ac400p+0 -0x1.1e34b8b586840p-1 0x1.868504131d5adp-1 0x1.f1f8bca8a1000p-2 0x1.f4b487791ab00p-2 0x1.9c42ca740da74p-1 "
        "-0x1.10404bec9f800p-1 -0x1.186e302b0fec0p+0 0x1.2a468369d036ap-1 -0x1.110cecfa10c00p+0 0x1.dcc849e4ca540p-2 0x1.3448e0fdf3b64p-1 "
        "0x1.1d40b2f591c00p+0 -0x1.f7b3a8104db80p-2 0x1.2974240aec33ep-1 0x1.0bab42184f000p-1 0x1.0f05ad798f4e0p-1 0x1.94db703c131d6p-1 "
        "-0x1.1811b3cbd3800p-1 -0x1.0f3c8a3f23d40p+0 0x1.25732067c3ecep-1 -0x1.19e4827dd3800p+0 0x1.15b8ceb29f1e0p-1 0x1.2c64272dbd194p-1 "
        "0x1.0143712b7d000p+0 -0x1.1b18894fcf040p-1 0x1.320608805761ap-1 0x1.0ab51d2f90000p-1 0x1.fd8fd6e8d6000p-2 0x1.98f6039581062p-1 "
        "-0x1.093d240f78800p-1 -0x1.15280ea4f9420p+0 0x1.2aedf54a69217p-1 -0x1.b044e240fe800p+0 0x1.d797bc7fefe40p-2 0x1.fdce14057619fp-1",
    (1600, 5, "built"):
        "0x1.ce4375cf4e400p+0 -0x1.01386225fe800p-1 0x1.03753727136a4p+0 0x1.0508ee68a2800p-1 0x1.0823836ea7400p-1 0x1.ba89bb31abbb5p-1 "
        "-0x1.fbe2977f6e000p-2 -0x1.14dd330cd6c00p+0 0x1.42e5a9f788f16p-1 -0x1.0eba9cb52a400p+0 0x1.036e9c8c0f000p-1 0x1.4357d3ec02f30p-1 "
        "0x1.155683c6e7400p+0 -0x1.01b8b0d1e5000p-1 0x1.4369ef227d029p-1 0x1.06507c6c87800p-1 0x1.0536d8f2be400p-1 0x1.b872808fbe06fp-1 "
        "-0x1.01526bf1a3000p-1 -0x1.12a30a33f9c00p+0 0x1.42b4133e8f403p-1 -0x1.1294d12fbf000p+0 0x1.fe6aa562e7000p-2 0x1.434d63a53b8e5p-1 "
        "0x1.131feb6819400p+0 -0x1.06a94194ff400p-1 0x1.43d392cc170c0p-1 0x1.06b560f538800p-1 0x1.0091c44eee000p-1 0x1.b904e384e6cbcp-1 "
        "-0x1.f39fae512f000p-2 -0x1.15670e4502000p+0 0x1.42cdc61c2038dp-1 -0x1.0f7066932e800p+0 0x1.f881bd2d60800p-2 0x1.43c25802d7034p-1",
    (1600, 5, "up1"):
        "0x1.ce43757443000p+0 -0x1.01385de27dc00p-1 0x1.037535b813016p+0 0x1.0508ef4a56800p-1 0x1.082385efb6400p-1 0x1.ba89bb4784231p-1 "
        "-0x1.fbe2988504000p-2 -0x1.14dd360b37a00p+0 0x1.42e5ac6d8de9bp-1 -0x1.0eba9eaeb9400p+0 0x1.036ea23107c00p-1 0x1.4357d3c21187ep-1 "
        "0x1.155681d514400p+0 -0x1.01b8cd13cb000p-1 0x1.4369ed527e521p-1 0x1.065079bd68000p-1 0x1.0536d46333000p-1 0x1.b8728235cb4c5p-1 "
        "-0x1.01526c0890000p-1 -0x1.12a30bbfe3800p+0 0x1.42b41288ce704p-1 -0x1.1294d588dd000p+0 0x1.fe6ab3a8ab800p-2 0x1.434d61d29dc72p-1 "
        "0x1.131fe9712e800p+0 -0x1.06a93fa3e6400p-1 0x1.43d39190a4b6cp-1 0x1.06b55df436000p-1 0x1.0091c9221d800p-1 0x1.b904e1b5c7cd9p-1 "
        "-0x1.f39fa843ba000p-2 -0x1.15670cdd56000p+0 0x1.42cdc66586b43p-1 -0x1.0f70662be0c00p+0 0x1.f881b43b6e800p-2 0x1.43c25729b280fp-1",
}


def _in_mode(mode, f):
    return f() if MODES[mode] is None else _with_env(MODES[mode][0], MODES[mode][1], f)


def _parent(rows, seed, mode):
    key = (rows, seed, "built" if mode == "window0" else mode)
    return np.array([float.fromhex(h) for h in PARENT[key].split()]).reshape(3, 4, 3)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("rows,seed", [(64, 4), (1600, 5)])
def test_same_bits_as_the_parent(ctx, rows, seed, mode):
    """64 lines: one line pair per workgroup, ky = 0 and ky = M / 2 (the real-only bins) among them; 1600 lines: three or
    four iterations per workgroup.  A pair plus a single unit (four and two outputs), and the single unit alone."""
    pan, bands = _scene(rows, seed)
    pp, qp, bp, qb, keep = _units_of(pan, bands, 3)
    run = lambda k: _in_mode(mode, lambda: ctx.interband_correlate_units(pp[k:], qp[k:], bp[k:], qb[k:], rows, N))
    gots = {k: run(k) for k in (0, 2)}                  # pair + single, single alone
    for k, got in gots.items():
        print("rows %d seed %d %s units %d..2: %s" % (rows, seed, mode, k, " ".join(float(v).hex() for v in got.ravel())))
    want = _parent(rows, seed, mode)
    for k, got in gots.items():
        assert got.shape == want[k:].shape, got.shape
        assert np.array_equal(got.astype(np.float64), want[k:]), np.abs(got - want[k:]).max(axis=(0, 1))
        exhaustive = _with_env("OIP_PEAK_PRUNE", "0", lambda: run(k))
        assert np.array_equal(exhaustive, got)


# ---- a scene that separates the exact formulas from the fast ones ----------------------------------------------------

BAND_ROWS, BAND_SEED, BAND_A = 400, 5, 30000.0
FAST_LIMIT = 1.8e19         # sqrt(FLT_MAX): above it mag * mag is inf in float and the fast formulas return inf * 0 = NaN


@functools.lru_cache(maxsize=None)
def _banded_scene():
    """the 400-line scene of the other row-stage tests plus a banding that is constant along rows: PAN rows get
    a (1 + cos(2 pi y / 16)) / 2, band rows the same with period 4 (period 16 once up-sampled), a = 30000 (no pixel
    clips: the scene stays below 4000).  Its energy falls in column kx = 0 -- lines ky = 0 and +-25 -- and leaves every
    interior bin alone."""
    pan, bands = _scene(BAND_ROWS, BAND_SEED)
    stripe = lambda n, period: BAND_A * (1 + np.cos(2 * np.pi * np.arange(n)[:, None] / period)) / 2
    put = lambda img, period: np.clip(np.rint(img + stripe(img.shape[0], period)), 0, 65535).astype(np.uint16)
    panb, bandsb = put(pan, 16), [put(b, 4) for b in bands]
    panb.setflags(write=False)
    for b in bandsb:
        b.setflags(write=False)
    return panb, bandsb


@functools.lru_cache(maxsize=None)
def _banded_oracle():
    """[unit][band] -> (dx, dy, response) of the oracle (pc.phase_correlate on the up-sampled band), computed once for
    both cases, after confirming that the scene does what it is for"""
    import oracle
    from oracle import phasecorr as pc
    oracle.lib()
    pan, bands = _banded_scene()
    want = np.zeros((3, 4, 3))
    for u in range(3):
        a = oracle.window_u16_to_f32(pan, 0, N * u, BAND_ROWS, N)
        for b in range(4):
            small = oracle.window_u16_to_f32(bands[b], 0, N // 4 * u, BAND_ROWS // 4, N // 4)
            up = oracle.resize_cubic(small, N, BAND_ROWS)
            # bin (ky = 25, kx = 0) of the two spectra: the column-0 bin is the transform of the row sums
            A, B = (np.fft.fft(img.sum(axis=1, dtype=np.float64))[BAND_ROWS // 16] for img in (a, up))
            assert abs(A) * abs(B) > FAST_LIMIT, (u, b, abs(A) * abs(B))
            (dx, dy), r = pc.phase_correlate(a, up)
            want[u, b] = dx, dy, r
    want.setflags(write=False)
    return want


@pytest.mark.parametrize("mode", ["built", "window0"])
def test_edge_column_bins_beyond_the_range_of_the_fast_formulas(ctx, mode):
    """At (ky = +-25, kx = 0) of the banded scene |A conj(B)| is 7.97e19 for all twelve (unit, band) (measured with the
    oracle's windows on the CPU; 64 lines would reach 2e18 only): the fast formulas of the interior bins give NaN there,
    divSpectrums' double-precision ones a finite value.  The oracle's responses are 0.60 .. 1.06: it masks none of the
    twelve.  A pair plus a single unit, through the windowed and the full-store instance."""
    pan, bands = _banded_scene()
    want = _banded_oracle()
    assert (want[..., 2] >= 0.05).all(), want[..., 2]
    pp, qp, bp, qb, keep = _units_of(pan, bands, 3)
    got = _in_mode(mode, lambda: ctx.interband_correlate_units(pp, qp, bp, qb, BAND_ROWS, N))
    d = np.abs(got - want)
    print("%s: |GPU - oracle| shifts %.3g px, response %.3g" % (mode, d[..., :2].max(), d[..., 2].max()))
    assert np.isfinite(got).all(), got
    assert d[..., 2].max() < RESP_TOL, (d[..., 2], got[..., 2], want[..., 2])
    ok = want[..., 2] >= 0.05
    assert d[..., :2][ok].max() < SHIFT_TOL, (d[..., :2], got[..., :2], want[..., :2])
