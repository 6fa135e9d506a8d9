"""The 8-pixels-per-lane bicubic kernels, bit for bit: every form of the constant-shift resampling (plain, window with
aligned and with scalar stores, RRC on load; f32 and fp16 accumulate) and one inter-band align on the fast path must give the
rasters whose SHA-256 tests/golden/bicubic_forms.json records (tests/golden/make_bicubic_forms.py wrote it on the MI355X at
the commit it names).  The tolerance tests bound the fp16 forms and compare them with each other; this pins their summation
order, so a refactor of the shared loop body can be shown to change no bit."""
import json
import os

import pytest

import _bicubic_forms as bf

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bicubic_forms.json")) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope="module")
def golden():
    """the recorded output hashes, handed out only when the inputs are the recorded ones"""
    got = bf.input_hashes()
    changed = sorted(k for k in GOLDEN["inputs"] if got.get(k) != GOLDEN["inputs"][k])
    assert not changed and set(got) == set(GOLDEN["inputs"]), "input generation changed: %s" % (changed or sorted(got))
    return GOLDEN["outputs"]


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("shift", bf.SHIFTS)
def test_remap_forms_match_the_recorded_bits(ctx, golden, shift, f16):
    want = golden[bf.remap_key(shift, f16)]
    got = {k: bf.sha(v) for k, v in bf.run_remap_forms(ctx, shift, f16).items()}
    assert set(got) == set(want)
    wrong = sorted(k for k in want if got[k] != want[k])
    assert not wrong, "bits differ from commit %s: %s" % (GOLDEN["commit"][:12], wrong)


def test_align_mss8_matches_the_recorded_bits(ctx, golden):
    assert bf.sha(bf.run_align(ctx)) == golden["align"]["align_mss"], "bits differ from commit %s" % GOLDEN["commit"][:12]
