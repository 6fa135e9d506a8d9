"""CPU suite, part 2: the product's host logic and the C-ABI surface (no compute calls)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import opticalimageprocessor_amd as oip


def test_library_loads_and_exports_every_declared_symbol():
    lib = oip.load_library()
    declared = oip.declared_symbols()
    assert len(declared) >= 30
    for name in declared:
        assert hasattr(lib, name), "include/oip_c.h declares %s but liboipgpu.so lacks it" % name
    assert lib.oip_version() == 0x0101
    exported = subprocess.run(["nm", "-D", "--defined-only", oip.library_path()], capture_output=True, text=True).stdout
    assert "oip_rrc_u16" in exported


def test_no_gpu_means_no_context():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    with pytest.raises(oip.OipError):
        oip.Context(0)          # no CPU fallback: creation must fail loudly


def test_product_never_imports_the_oracle():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "opticalimageprocessor_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".cpp", ".h", "Makefile")):
                text = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "oip_oracle" not in text and "import oracle" not in text and "from oracle" not in text, f


# ---- RRC parameter file (imageop.h:140-192) ----------------------------------------------------
def _write(p, text):
    p.write_text(text)
    return str(p)


def test_load_rrc_param_file(tmp_path, oracle_mod):
    good = _write(tmp_path / "a.csv", "1\n3\n0\n1.000001 , -7.25\n0.9,8\n  1.1   ,   0\n")
    kb = oip.load_rrc_param_file(good, 3)
    assert np.array_equal(kb, oracle_mod.load_rrc_param_file(good, 3))
    assert np.array_equal(kb, [[1.000001, -7.25], [0.9, 8], [1.1, 0]])
    with pytest.raises(OSError, match="open RRC Param file failed"):
        oip.load_rrc_param_file(str(tmp_path / "missing.csv"), 3)
    with pytest.raises(RuntimeError, match="expected 4 lines while 3 found"):
        oip.load_rrc_param_file(good, 4)
    short = _write(tmp_path / "b.csv", "1\n3\n0\n1,0\n1,0\n")
    with pytest.raises(RuntimeError, match="3 lines of param expected, 2 lines parsed"):
        oip.load_rrc_param_file(short, 3)
    blank = _write(tmp_path / "c.csv", "1\n2\n0\n1,0\n1,0\n\n")       # trailing blank line: App.B-9
    with pytest.raises(RuntimeError, match="line #2 .* found invalid"):
        oip.load_rrc_param_file(blank, 2)
    bad = _write(tmp_path / "d.csv", "1\n2\n0\n1;0\n1,0\n")
    with pytest.raises(RuntimeError, match="line #0"):
        oip.load_rrc_param_file(bad, 2)
    empty = _write(tmp_path / "e.csv", "1\n")
    with pytest.raises(OSError, match=r"\[2\]"):
        oip.load_rrc_param_file(empty, 2)


# ---- polynomial fit (preproc.h:514-550) ----------------------------------------------------------
# Two fits: "reference" (the default) restates NumCpp's Poly1d::fit as the reference calls it --
# inv(A^T A) A^T y, raw abscissa, NumCpp's own Gauss-Jordan inverse -- and must equal the oracle's
# operation-for-operation restatement bit for bit; "lstsq" solves the same problem by QR.
@pytest.mark.parametrize("fit", ["reference", "lstsq"])
def test_polyfit_exact_polynomials(fit):
    x = np.array([614., 1842, 3070, 4298, 5526, 6754, 7982, 9210, 10438, 11666])
    c1 = oip.polyfit(x, 3.25 - 1.5e-4 * x, 1, fit)
    assert np.allclose(c1, [3.25, -1.5e-4], rtol=1e-9, atol=1e-12)
    c2 = oip.polyfit(x, -2.0 + 3e-4 * x - 2.5e-8 * x * x, 2, fit)
    tol = 1e-10 if fit == "lstsq" else 1e-5          # the normal equations keep ~5 digits of the curvature
    assert np.allclose(c2, [-2.0, 3e-4, -2.5e-8], rtol=tol, atol=1e-9 if fit == "reference" else 1e-12)


def test_polyfit_reference_equals_the_numcpp_restatement_bitwise():
    from oracle import phasecorr as pc
    rng = np.random.default_rng(7)
    for width in (12288, 30000):
        for trial in range(20):
            n = int(rng.integers(5, 51))
            x = (rng.integers(0, 10, n) * (width // 10) + width // 20).astype(np.float64)
            if len(set(x)) < 3:
                continue
            y = rng.normal(0, 2, n)
            for deg in (1, 2):
                got = oip.polyfit(x, y, deg, "reference")
                want = pc.polyfit_numcpp(x, y, deg)
                assert np.array_equal(got, want), (width, n, deg, got, want)


def _phase_flips(width, c_a, c_b, rows=(0, 5000, 19999)):
    """output pixels of a 1/32-px bicubic map whose integer 1/32-px position differs between two fits
    of dy(cx) (preproc.h:447-448: mapY = (cY2 xx xx + cY1 xx + cY0 + yy) / 4, xx = 4 x)"""
    x = np.arange(width // 4, dtype=np.float64) * 4.0
    flips = 0
    for yrel in rows:
        yy = float(yrel * 4)
        m_a = (((c_a[2] * x) * x + c_a[1] * x) + c_a[0] + yy) / 4.0
        m_b = (((c_b[2] * x) * x + c_b[1] * x) + c_b[0] + yy) / 4.0
        s_a = np.rint(m_a.astype(np.float32) * np.float32(32.0))
        s_b = np.rint(m_b.astype(np.float32) * np.float32(32.0))
        flips += int((s_a != s_b).sum())
    return flips, len(rows) * (width // 4)


def test_polyfit_modes_differ_by_counted_phase_flips_at_30000_columns():
    """The two fits are different functions of the same data.  On the 30000-wide geometry the fitted dy
    curves differ by up to ~1e-2 px, which moves some output pixels to the neighbouring 1/32-px phase;
    the count is printed (pytest -s) and bounded.  `oip` uses the reference formulation by default
    because a drop-in must produce the reference's maps, not better ones."""
    from oracle import phasecorr as pc
    rng = np.random.default_rng(2)
    x = np.tile(np.arange(10) * 3000.0 + 1500, 5)
    y = 1.7 + 2e-5 * x - 3e-9 * x * x + rng.normal(0, 0.05, x.size)
    ref = oip.polyfit(x, y, 2, "reference")
    qr = oip.polyfit(x, y, 2, "lstsq")
    want = pc.polyfit(x, y, 2, "lstsq")
    xs = np.linspace(0, 30000, 200)
    ev = lambda c: c[0] + c[1] * xs + c[2] * xs * xs
    assert np.abs(ev(qr) - ev(want)).max() < 1e-10
    drift = np.abs(ev(ref) - ev(want)).max()
    assert drift < 5e-2
    flips, total = _phase_flips(30000, ref, qr)
    print("\nfit reference vs lstsq at W=30000: curve drift %.3g px, %d of %d sampled output pixels change 1/32-px phase"
          % (drift, flips, total))
    assert flips <= total               # counted, not required to be zero
    # at the reference's own width the two agree far better
    x12 = np.tile(np.arange(10) * 1228.0 + 614, 5)
    y12 = 1.7 + 2e-5 * x12 - 3e-9 * x12 * x12 + rng.normal(0, 0.05, x12.size)
    f12, t12 = _phase_flips(12288, oip.polyfit(x12, y12, 2, "reference"), oip.polyfit(x12, y12, 2, "lstsq"))
    print("fit reference vs lstsq at W=12288: %d of %d sampled output pixels change 1/32-px phase" % (f12, t12))


def test_polyfit_rejects_underdetermined():
    for fit in ("reference", "lstsq"):
        with pytest.raises((ValueError, RuntimeError)):
            oip.polyfit([1.0, 2.0], [1.0, 2.0], 2, fit)
    with pytest.raises((ValueError, RuntimeError)):
        oip.polyfit([5.0, 5.0, 5.0, 5.0], [1.0, 2.0, 3.0, 4.0], 2, "lstsq")      # degenerate abscissae


def test_filter_and_fit():
    from oracle import phasecorr as pc
    rng = np.random.default_rng(5)
    n = 20
    s = np.zeros((4, n, 4))
    for b in range(4):
        cx = np.tile(np.arange(10) * 1228 + 614, 2)
        s[b, :, 3] = cx
        s[b, :, 0] = b + 1e-4 * cx + rng.normal(0, 0.01, n)
        s[b, :, 1] = -b + 2e-4 * cx - 1e-8 * cx * cx + rng.normal(0, 0.01, n)
        s[b, :, 2] = rng.uniform(0.41, 0.9, n)
    s[1, :6, 2] = 0.1                         # filtered out
    s[1, :6, 0] = 99.0
    s[2, 3, :3] = np.nan                      # a section another rank owns
    cx, cy = oip.filter_and_fit(s, 0.4, 5)                         # reference formulation: bit-exact
    wcx, wcy = pc.filter_and_fit(s, 0.4, 5, "numcpp")
    assert np.array_equal(cx, wcx) and np.array_equal(cy, wcy)
    cx, cy = oip.filter_and_fit(s, 0.4, 5, "lstsq")
    wcx, wcy = pc.filter_and_fit(s, 0.4, 5, "lstsq")
    assert np.allclose(cx, wcx, rtol=1e-8, atol=1e-10) and np.allclose(cy, wcy, rtol=1e-6, atol=1e-10)
    s[3, :, 2] = 0.39
    s[3, :4, 2] = 0.5
    with pytest.raises(RuntimeError, match="band#4: 4 valid values found, 5 expected"):
        oip.filter_and_fit(s, 0.4, 5)


def test_stt_mean_follows_the_reference_filter():
    t = np.array([[1.0, 2.0, 0.5], [3.0, 9.0, 0.9], [5.0, 6.0, 0.6], [np.nan, np.nan, np.nan], [7.0, 1.0, 0.39]])
    assert oip.stt_mean(t, 0.4, 0.0) == (3.0, (2.0 + 9.0 + 6.0) / 3, (0.5 + 0.9 + 0.6) / 3, 3)
    assert oip.stt_mean(t, 0.4, 6.5) == (3.0, 4.0, 0.55, 2)          # |dy| <= maxDeltaY drops the 9.0 row
    with pytest.raises(RuntimeError, match="No valid delta value"):
        oip.stt_mean(t, 0.95)


# ---- halo ranges of the row-block shards -----------------------------------------------------------
def test_remap_src_range_is_tight_superset(oracle_mod):
    W, L, dy, sr, guard = 8, 1500, 3.3, 300, 327
    src = (np.arange(L, dtype=np.uint16)[:, None] + 1).repeat(W, 1)     # line y holds value y+1
    dst, _ = oracle_mod.prestitch(src, 0.0, dy, sr, guard)
    for o0, o1 in [(0, 500), (500, 1000), (1000, 1500), (290, 310), (1490, 1500), (0, 1500)]:
        s0, s1 = oip.remap_shift_src_range(o0, o1 - o0, L, dy, sr)
        assert 0 <= s0 <= s1 <= L
        # recompute the window from only those lines: identical to the full result
        masked = np.zeros_like(src); masked[s0:s1] = src[s0:s1]
        part, _ = oracle_mod.prestitch(masked, 0.0, dy, sr, guard)
        assert np.array_equal(part[o0:o1], dst[o0:o1]), (o0, o1, s0, s1)
        assert s1 - s0 <= (o1 - o0) + 2 * int(abs(dy)) + 8 + (sr if o1 > L - 310 else 0)


def test_align_src_range_is_superset(oracle_mod):
    Wb, Lm, lps, ovl, minl = 40, 1200, 400, 52, 150
    rng = np.random.default_rng(1)
    bands = [rng.integers(0, 4096, (Lm, Wb), dtype=np.uint16) for _ in range(4)]
    cx = np.zeros((4, 2)); cy = np.zeros((4, 3))
    for b in range(4):
        cy[b] = (rng.uniform(-9, 9), rng.uniform(-4, 4) / (4 * Wb), rng.uniform(-8, 8) / (4 * Wb) ** 2)
    want, _ = oracle_mod.align_mss(bands, cx, cy, lps, 0, ovl, False, minl)
    R = want.shape[0]
    for o0, o1 in [(0, 300), (300, 700), (700, R), (340, 360)]:
        s0, s1 = oip.align_mss_src_range(o0, o1 - o0, Lm, cy, Wb, lps, 0, ovl, False, minl)
        assert 0 <= s0 <= s1 <= Lm
        masked = [np.zeros_like(b) for b in bands]
        for m, b in zip(masked, bands):
            m[s0:s1] = b[s0:s1]
        part, _ = oracle_mod.align_mss(masked, cx, cy, lps, 0, ovl, False, minl)
        assert np.array_equal(part[o0:o1], want[o0:o1]), (o0, o1, s0, s1)


def test_upsample_operator_reproduces_the_transform_of_the_resized_image(oracle_mod):
    """The inter-band correlation transforms the band window and applies the x4 cubic up-sampling to its spectrum
    (DESIGN.md 4.3): DFT(resize(B)) = Hv Hh B^ + column / row corrections, with H, G from oip_upsample_operator.  Pinned
    here against the oracle's cv::resize restatement on both axes (float64 FFTs; the resized image itself is float32,
    so agreement is at its rounding: 1e-6 of the spectrum's peak)."""
    rng = np.random.default_rng(3)
    for m, n in ((8, 12), (25, 10), (40, 188)):
        B = rng.integers(64, 4096, (m, n)).astype(np.float64)
        U = oracle_mod.resize_cubic(B.astype(np.float32), 4 * n, 4 * m).astype(np.float64)
        ref = np.fft.fft2(U)
        opv, oph = oip.upsample_operator(m).astype(np.complex128), oip.upsample_operator(n).astype(np.complex128)
        Hv, Gv, Hh, Gh = opv[0], opv[1:], oph[0], oph[1:]
        Jv, Jh = [0, 1, m - 2, m - 1], [0, 1, n - 2, n - 1]
        ky, kx = np.arange(4 * m), np.arange(4 * n)
        B2 = np.fft.fft2(B)
        Bcol = np.fft.fft(B[:, Jh], axis=0)                       # column transforms of the four raw columns
        Brow = np.fft.fft(B[Jv, :], axis=1)                       # row transforms of the four raw rows
        got = (Hv[:, None] * Hh[None, :]) * B2[np.ix_(ky % m, kx % n)]
        got += (Hv[:, None] * Bcol[ky % m, :]) @ Gh
        got += Gv.T @ (Hh[None, :] * Brow[:, kx % n] + B[np.ix_(Jv, Jh)] @ Gh)
        assert np.abs(got - ref).max() < 2e-6 * np.abs(ref).max(), (m, n, np.abs(got - ref).max() / np.abs(ref).max())
    with pytest.raises(ValueError):
        oip.upsample_operator(4)


def test_fft_index_helpers_under_sanitizers(tmp_path):
    """csrc/oip_fft.h on the CPU (tests/cpp/fft_index_test.cpp; ASan + UBSan): oip_pos_to_freq / oip_freq_to_pos are mutual
    inverses, permutations of [0, L) and the header's definition recomputed independently, for every factor list the planner
    emits for the tested shapes; oip_peak_pack / oip_peak_key keep the value order (negative, denormal, zero, positive, inf),
    -0 == +0, NaN = the empty slot, ties to the smallest key (0 and 2^32 - 2 included), and the key round-trips."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "tests", "cpp", "fft_index_test.cpp")
    inc = os.path.join(root, "opticalimageprocessor_amd", "csrc")
    rocm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")          # oip_fft.h takes float2 from the HIP headers
    exe = tmp_path / "fft_index"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-D__HIP_PLATFORM_AMD__", "-I" + rocm, "-I" + inc, src, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and " checks, 0 bad" in r.stdout and "FAILED" not in r.stdout, r.stdout + r.stderr


def test_fft_planner_under_sanitizers(tmp_path):
    """csrc/oip_fftplan.h on the CPU (tests/cpp/fftplan_test.cpp; ASan + UBSan): for every 2^a 3^b 5^c row length up to 2^20 and
    column length from 2 to 2^18 a plan exists; its factors multiply to the length and keep their limits (256 leading, 256 last
    column, 4096 last row); at most 16 radices that multiply to F; a generic tile within kMaxTileElems and, with the static
    arrays, within 160 KiB of LDS; O1, O2 <= 65535 and inter-pass twiddle rows within 16 MiB (nothing the launcher refuses);
    oip_pos_to_freq / oip_freq_to_pos inverse to each other with the plan's digits.  And what the planner gives today: at most
    7 radices up to 4096 points, 46875 the first three-pass column length, no four-pass length, the tile class per factor,
    the lines and refusals of oip_fft_plan_describe."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "tests", "cpp", "fftplan_test.cpp")
    inc = os.path.join(root, "opticalimageprocessor_amd", "csrc")
    rocm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")          # oip_fft.h takes float2 from the HIP headers
    exe = tmp_path / "fftplan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-D__HIP_PLATFORM_AMD__", "-I" + rocm, "-I" + inc, src, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and " checks, 0 bad" in r.stdout and "FAILED" not in r.stdout, r.stdout + r.stderr


def test_fft_plan_describe_is_the_planner(tmp_path):
    """oip_fft_plan_describe through capi: the lines of the product's own shapes, a generic class, and a refusal's text"""
    got = oip.fft_plan_describe(16000, 3000)
    assert [(p["axis"], p["F"], p["mode"], p["kind"], p["vshift"], p["Vp"], p["radix"]) for p in got] == [
        ("y", 128, 0, "ct", 4, 17, (8, 8, 2)), ("y", 125, 0, "ct", 4, 17, (5, 5, 5)), ("x", 3000, 1, "ct", 1, 2, (3, 8, 5, 5, 5))]
    got = oip.fft_plan_describe(243, 3750)
    assert [(p["axis"], p["F"], p["kind"], p["vshift"], p["Vp"], p["radix"], p["lds"]) for p in got] == [
        ("y", 243, "generic", 4, 17, (3,) * 5, 8 * (2 * 243 * 17 + 243)), ("x", 3750, "generic", 0, 1, (3, 2, 5, 5, 5, 5), 8 * 3 * 3750)]
    with pytest.raises(ValueError, match="14 x 16 is not 2\\^a3\\^b5\\^c"):
        oip.fft_plan_describe(14, 16)
    with pytest.raises(ValueError, match="fewer than 2 rows"):
        oip.fft_plan_describe(1, 16)
