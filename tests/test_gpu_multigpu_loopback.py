"""GPU: the N-GPU host (csrc/oip_multigpu.hpp: `oip --gpus N`, `oip prestitch --gpus N`) with 2, 3 and 4 ranks on ONE GPU, over the
loopback communicator (OIP_COMM=loopback, csrc/oip_loopcomm.hpp): exchange_and_correlate (post_pieces, the wait per group,
finish_pieces), exchange_lines, allgather_table, the rank-order product writes and the failure protocol all execute with peers.
Every product file must equal the plain CLI's byte for byte.  The loopback proves ordering and addressing -- not RCCL's
behaviour or any link rate.

No case is vacuous: each asserts from `oip plan` with the same numbers that window pieces move between ranks and that halo lines
do, that the run logged "with window exchange", and that the bytes and calls the loopback counted per rank for the WINDOW
exchange equal the plan's sums (pieces with src != dst: rows x cols x 2 bytes, one send per plane, four planes for an MSS
piece).  The halo share is not compared with a plan: `oip plan` takes one polynomial for all bands and the log rounds dy; the
case asserts that the plan for the logged figures moves halo lines and that the run sent bytes beyond the window share.

The protocol itself (matching, size mismatch, abort, deadline) is tested on the CPU under sanitizers in tests/test_cli_cpu.py;
tests/test_gpu_resample.py has the kernel-level companions (row windows of the align fast path, fp16 remap shards)."""
import json
import os
import re
import shutil
import subprocess
import time

import numpy as np
import pytest

import _synth

pytestmark = pytest.mark.gpu
OIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "opticalimageprocessor_amd", "lib", "oip")
W, L, OV = 1024, 33024, 64                       # 33024: a multiple of 4 N for N = 2, 3, 4, and beyond the remap row guard of 32767
INPUTS = ("S_PAN-1.RAW", "S_PAN-2.RAW", "T_PAN.RAW", "T_MSS.RAW", "PAN-1.csv", "PAN-2.csv") + tuple("MSS.B%d.csv" % (b + 1) for b in range(4))
DEFAULT_SETS = {"8x1": ["--slices", "8", "--ibc-sections", "1"], "9x2": ["--slices", "9", "--ibc-sections", "2"]}
DEFAULT_PRODUCTS = ("T_MSS.ALIGNED.TIFF",)
PRESTITCH_PRODUCTS = ("S_PAN-1.RRC.RAW", "S_PAN-2.RRC.RAW", "S_PAN-2.RRC.PRESTT.RAW")
# the entries of a `  GPU r:` stage row; the RECEIVED_STAGES only on a rank that receives a group of units
RECEIVED_STAGES = ("exchange_wait", "correlate_received")
DEFAULT_STAGES = ["read", "rrc", "exchange_post", "correlate_resident", "exchange_wait", "correlate_received", "exchange_drain", "allgather",
                  "fit+halo", "align+download"]
PRESTITCH_STAGES = ["read", "rrc", "correlate_resident", "exchange_wait", "correlate_received", "exchange_drain", "allgather", "rrc_x2", "halo",
                    "remap", "write"]


def _csv(path, kb):
    with open(path, "w") as f:
        f.write("1\n%d\n0\n" % len(kb))
        for k, b in kb:
            f.write("%.6f , %.4f\n" % (k, b))


def _default_args(key):
    args = ["--width", str(W), "--pan", "T_PAN.RAW", "--mss", "T_MSS.RAW"] + DEFAULT_SETS[key] + \
           ["--ibc-threshold", "0", "--lines-section", "3000", "--overlap-lines", "100"]
    for b in range(4):
        args += ["--rrc-msb%d" % (b + 1), "MSS.B%d.csv" % (b + 1)]
    return args


def _prestitch_args(f16):
    return ["prestitch", "--width", str(W), "--pan1", "S_PAN-1.RAW", "--pan2", "S_PAN-2.RAW", "--rrc1", "PAN-1.csv", "--rrc2", "PAN-2.csv",
            "-s", "5", "-l", "1600", "--stitch-overlap", str(OV), "--stt-threshold", "0.05"] + (["--fp16-accumulate"] if f16 else [])


class _Strip:
    """the inputs, written once; a run gets a directory of its own with links to them (the products land beside the inputs)"""

    def __init__(self, base):
        self.base = str(base)
        self.inputs = os.path.join(self.base, "inputs")
        os.makedirs(self.inputs)
        pan1, pan2 = _synth.ccd_pair(L, W, OV, (3, -2), seed=15)
        pan, bands = _synth.pan_mss(L, W, [(2, -1), (1, 1), (-1, -2), (-2, 1)], seed=16)
        d = self.inputs
        pan1.tofile(os.path.join(d, "S_PAN-1.RAW")); pan2.tofile(os.path.join(d, "S_PAN-2.RAW"))
        pan.tofile(os.path.join(d, "T_PAN.RAW")); np.concatenate(bands, axis=1).tofile(os.path.join(d, "T_MSS.RAW"))
        _csv(os.path.join(d, "PAN-1.csv"), _synth.lut(W, 1)); _csv(os.path.join(d, "PAN-2.csv"), _synth.lut(W, 2))
        for b in range(4):
            _csv(os.path.join(d, "MSS.B%d.csv" % (b + 1)), _synth.lut(W // 4, 20 + b))
        self.plain = {}

    def run(self, name, args, extra_env=None):
        d = os.path.join(self.base, name)
        os.makedirs(d)
        for f in INPUTS:
            os.symlink(os.path.join(self.inputs, f), os.path.join(d, f))
        env = dict(os.environ, LOGFILE=os.path.join(d, "oip.log"), OIP_TIFF_COMPRESS="none")
        for k in ("OIP_COMM", "OIP_FAULT_INJECT", "OIP_LOOPBACK_DEVICE", "OIP_LOOPBACK_TIMEOUT_S", "OIP_LINK_GBS"):
            env.pop(k, None)
        env.update(extra_env or {})
        t0 = time.time()
        r = subprocess.run([OIP] + args, cwd=d, env=env, capture_output=True, text=True, timeout=120)
        return d, r, time.time() - t0


@pytest.fixture(scope="module")
def strip(tmp_path_factory):
    s = _Strip(tmp_path_factory.mktemp("loopback"))
    # the plain CLI, once per option set
    for key in DEFAULT_SETS:
        d, r, _ = s.run("plain-" + key, _default_args(key))
        assert r.returncode == 0, r.stdout + r.stderr
        s.plain[key] = (d, r.stdout)
    for f16 in (False, True):
        d, r, _ = s.run("plain-prestitch-%d" % f16, _prestitch_args(f16))
        assert r.returncode == 0, r.stdout + r.stderr
        s.plain[f16] = (d, r.stdout)
    yield s
    shutil.rmtree(s.base, ignore_errors=True)


def _plan(args):
    r = subprocess.run([OIP, "plan"] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout)


def _window_sums(pieces, n, planes_of_kind1):
    """per rank (sent bytes, sends, received bytes, receives) of the pieces that change rank"""
    sums = [[0, 0, 0, 0] for _ in range(n)]
    for src, dst, kind, _unit, _row0, rows, _col0, cols, _dst_row in pieces:
        if src == dst:
            continue
        planes = planes_of_kind1 if kind == 1 else 1
        sums[src][0] += rows * cols * 2 * planes; sums[src][1] += planes
        sums[dst][2] += rows * cols * 2 * planes; sums[dst][3] += planes
    return sums


def _loopback_lines(out, n):
    total = re.findall(r"^loopback: GPU (\d+) sent (\d+) bytes in (\d+) sends, received (\d+) bytes in (\d+) receives$", out, re.M)
    window = re.findall(r"^loopback: GPU (\d+) window exchange alone: sent (\d+) bytes in (\d+) sends, received (\d+) bytes in (\d+) receives; "
                        r"(\d+) all-gathers of (\d+) bytes$", out, re.M)
    assert [int(t[0]) for t in total] == list(range(n)) and [int(t[0]) for t in window] == list(range(n)), out
    return [[int(v) for v in t[1:]] for t in total], [[int(v) for v in t[1:]] for t in window]


def _check_exchange(out, n, pieces, halo, planes_of_kind1, gather_bytes, stages):
    """the run was not vacuous and moved what the plan says"""
    moved = [p for p in pieces if p[0] != p[1]]
    assert moved and halo, (moved, halo)
    assert "with window exchange" in out, out
    want = _window_sums(pieces, n, planes_of_kind1)
    total, window = _loopback_lines(out, n)
    for r in range(n):
        print("GPU %d: plan's window share %s, loopback counted %s, all traffic %s" % (r, want[r], window[r][:4], total[r]))
    for r in range(n):
        assert window[r][:4] == want[r], (r, window[r], want[r])
        assert window[r][4:] == [1, gather_bytes], (r, window[r])           # one all-gather of the result table per run
    # beyond the window share only halo lines move: somebody sent some, and what was sent was received
    assert sum(t[0] for t in total) > sum(w[0] for w in want)
    assert sum(t[0] for t in total) == sum(t[2] for t in total) and sum(t[1] for t in total) == sum(t[3] for t in total)
    # the stage table has one row per GPU, its entries in the work-flow's order; a rank waits for windows and correlates received
    # units exactly when the plan moves a piece to it
    rows = re.findall(r"^  GPU (\d+): (.*)$", out, re.M)
    assert [r for r, _ in rows] == [str(r) for r in range(n)], out
    receivers = {p[1] for p in moved}
    for r, (_, row) in enumerate(rows):
        want_names = [s for s in stages if s not in RECEIVED_STAGES or r in receivers]
        print("GPU %d: stages %s" % (r, row))
        assert [e.rsplit(" ", 1)[0] for e in row.split(" | ")] == want_names, (r, row, want_names)


def _same_products(strip, plain_key, d, products):
    for f in products:
        a = open(os.path.join(strip.plain[plain_key][0], f), "rb").read()
        b = open(os.path.join(d, f), "rb").read()
        assert len(a) > 1000 and a == b, f
    shutil.rmtree(d)                               # (the strip-sized products of a dozen runs would pile up)


@pytest.mark.parametrize("key", sorted(DEFAULT_SETS))
@pytest.mark.parametrize("n", [2, 3, 4])
def test_default_action_on_n_ranks_equals_the_plain_cli(strip, n, key):
    """8 x 1: every unit's windows move at N = 2, 3, 4.  9 x 2 at N = 2: unit 9 moves while its partner unit 8 is resident -- the
    mixed pair of the pairing rule in Node::exchange_and_correlate; at N = 3, 4 all 18 units move.  The 3000-line align sections
    straddle the block boundaries (MSS line 4128 at N = 2), so the align fast path runs on row windows with src_row0 != 0."""
    d, r, _ = strip.run("node-%s-%d" % (key, n), _default_args(key) + ["--gpus", str(n)], {"OIP_COMM": "loopback"})
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    coeff = lambda text: [l.split("coeff:")[1] for l in text.splitlines() if "coeff:" in l]
    assert len(coeff(out)) == 8 and coeff(out) == coeff(strip.plain[key][1]), out
    cy0 = re.search(r"BAND 0.*\n.*deltaY coeff: \[2\] (\S+), \[1\] (\S+), \[0\] (\S+)", out)
    slices, sections = DEFAULT_SETS[key][1], DEFAULT_SETS[key][3]
    plan = _plan(["strip", "--width", W, "--lines", L, "--gpus", n, "--slices", slices, "--ibc-sections", sections, "--lines-section", 3000,
                  "--overlap-lines", 100, "--cy=%s,%s,%s" % (cy0.group(3), cy0.group(2), cy0.group(1))])
    if key == "9x2" and n == 2:
        assert plan["assign"][8] == plan["assign"][9] == 0 and {p[3] for p in plan["pieces"] if p[0] != p[1]} == {9}
    _check_exchange(out, n, plan["pieces"], plan["align_transfers"], 4, int(slices) * int(sections) * 12 * 8, DEFAULT_STAGES)
    _same_products(strip, key, d, DEFAULT_PRODUCTS)


@pytest.mark.parametrize("f16", [False, True], ids=["fp32", "fp16acc"])
@pytest.mark.parametrize("n", [2, 3, 4])
def test_prestitch_on_n_ranks_equals_the_plain_cli(strip, n, f16):
    """five sections: units [2], [1, 3] and [2] move windows at N = 2, 3 and 4 (three sections would move nothing at N = 3); the
    remap halo crosses every block boundary; the ranks append their blocks to the three product files in rank order."""
    d, r, _ = strip.run("node-prestitch-%d-%d" % (f16, n), _prestitch_args(f16) + ["--gpus", str(n)], {"OIP_COMM": "loopback"})
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    table = lambda text: [l for l in text.splitlines() if re.match(r"^\|\s*\d+ \|", l)] + [l.split("dx:")[1] for l in text.splitlines() if " dx: " in l]
    assert len(table(out)) == 6 and table(out) == table(strip.plain[f16][1]), out
    dy = re.search(r" dx: \S+ dy: (\S+),", out).group(1)
    plan = _plan(["ccd", "--width", W, "--lines", L, "--gpus", n, "--sections", 5, "--section-lines", 1600, "--stitch-overlap", OV, "--dy=%s" % dy])
    assert sorted({p[3] for p in plan["pieces"] if p[0] != p[1]}) == {2: [2], 3: [1, 3], 4: [2]}[n]
    _check_exchange(out, n, plan["pieces"], plan["remap_transfers"], 1, 5 * 3 * 8, PRESTITCH_STAGES)
    _same_products(strip, f16, d, PRESTITCH_PRODUCTS)


@pytest.mark.parametrize("point", ["exchange", "halo", "allgather"])
def test_a_failing_rank_is_the_one_reported(strip, point):
    """N = 3, rank 1 throws (a host exception, OIP_FAULT_INJECT) where its peers already sit in the blocking group end or
    all-gather that waits for it: the abort releases them, the process leaves with exit code 2 and rank 1's message -- not with
    rank 0's "ncclGroupEnd failed", which the abort caused and which run() used to prefer for its lower index -- and well inside
    the rendezvous deadline of 30 s."""
    d, r, seconds = strip.run("fault-" + point, _default_args("8x1") + ["--gpus", "3"], {"OIP_COMM": "loopback", "OIP_FAULT_INJECT": "1:" + point})
    out = r.stdout + r.stderr
    print("%s: exit %d after %.2f s" % (point, r.returncode, seconds))
    assert r.returncode == 2, out
    assert [l.split("[ERROR] ")[1] for l in out.splitlines() if "[ERROR]" in l] == ["injected failure on GPU 1 at %s." % point], out
    assert "timed out" not in out and "ncclGroupEnd failed" not in out and "ncclAllGather failed" not in out, out
    assert seconds < 15.0, seconds
    shutil.rmtree(d)
