"""CPU: the f32 bits that tests/golden/bicubic_forms.json records are the oracle's bits, not only the kernels' own.

The file holds SHA-256 digests of what the 8-pixels-per-lane bicubic kernels gave for the inputs of tests/_bicubic_forms.py
(test_gpu_bicubic_golden.py checks the kernels against it).  Here the oracle runs on the same inputs: oracle.prestitch for
the three shifts, laid out as each form lays its raster out -- the plain raster; the window forms with the columns from the
fold on at offset W - fold of a 2 (W - fold) wide raster whose left half stays zero; the RRC-on-load forms on oracle.rrc of
the raw strip -- and oracle.align_mss for the inter-band align.  Every digest must equal the recorded f32 one (the fp16
accumulate forms have no reference: the tolerance tests bound them)."""
import json
import os

import numpy as np
import pytest

import _bicubic_forms as bf

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bicubic_forms.json")) as _f:
    GOLDEN = json.load(_f)


def _window(plain, fold):
    out = np.zeros((bf.L, 2 * (bf.W - fold)), np.uint16)
    out[:, bf.W - fold:] = plain[:, fold:]
    return out


@pytest.fixture(scope="module")
def inputs():
    assert bf.input_hashes() == GOLDEN["inputs"], "input generation changed"
    return bf.inputs()


@pytest.mark.parametrize("shift", bf.SHIFTS)
def test_recorded_remap_bits_are_the_oracles(oracle_mod, inputs, shift):
    want = GOLDEN["outputs"][bf.remap_key(shift, False)]
    plain, _ = oracle_mod.prestitch(inputs["src"], shift[0], shift[1], bf.SECTION_ROWS, bf.ROW_GUARD)
    corrected, _ = oracle_mod.prestitch(oracle_mod.rrc(inputs["raw"], inputs["kb"]), shift[0], shift[1], bf.SECTION_ROWS, bf.ROW_GUARD)
    got = {"plain": bf.sha(plain)}
    for fold in bf.FOLDS:
        got["window fold=%d" % fold] = bf.sha(_window(plain, fold))
        got["rrc window fold=%d" % fold] = bf.sha(_window(corrected, fold))
    assert set(got) == set(want)
    assert got == want, sorted(k for k in want if got[k] != want[k])


def test_recorded_align_bits_are_the_oracles(oracle_mod, inputs):
    Wb, Lm, lps, off, ovl, keep, minl = bf.align_case()
    dst, _ = oracle_mod.align_mss(list(inputs["align_bands"]), inputs["align_cx"], inputs["align_cy"], lps, off, ovl, keep, minl)
    assert bf.sha(dst) == GOLDEN["outputs"]["align"]["align_mss"]
