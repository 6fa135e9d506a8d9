"""Times the four strip-streaming raster tools end to end, one `oip` binary against another (the parent commit's against this
tree's), and prints one JSON line (to be kept as profiles/raster_tools_cli.json and quoted in DESIGN.md 4.1e).

    python profiles/raster_tools_cli_bench.py --parent PATH/TO/PARENT/oip [--new PATH/TO/oip] [--dir DIR] [--lines 60000] [--runs 5]

One RAW strip of 12288 x 60000 samples (about 1.4 GB of 12-bit sensor-like values) is generated once in DIR (a local disk;
the default is the temporary directory).  The commands:
    rrc-calib   oip rrc-calib --pan STRIP --rrc-pan OUT --force
    quicklook   oip quicklook STRIP -o OUT.TIFF --force
    mtfc        oip mtfc STRIP --mtf-x 0.3 --mtf-y 0.45 -o OUT.RAW --force
    despike     oip despike STRIP --threshold 200 -o OUT.RAW --force
Per command and binary one warm-up run is discarded (the page cache is then in the same state for both; its products are
hashed, and the two binaries' hashes must agree), then --runs timed runs per binary, parent and new alternating.  A run's
time is the tool's own closing "bytes in ... seconds" line, with the wall time of the process beside it.  Every run sits
under its own `timeout -k 10`, sized from the command's first run, and a run that fails ends the script.

These runs are bound by file I/O; the parent's own spread over its runs (max - min) is the noise floor a host-side change is
judged against: `within_parent_spread` says whether the new median is at most the parent's median plus that spread."""
import argparse
import hashlib
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 12288


def make_strip(path, lines):
    rng = np.random.default_rng(1)
    x = np.arange(W)
    with open(path, "wb") as f:
        for r in range(0, lines, 2000):
            m = min(2000, lines - r)
            y = np.arange(r, r + m)[:, None]
            img = 1500 + 200 * np.sin(x / 17.0)[None, :] + 0.01 * y + rng.integers(-20, 21, (m, W))
            hot = rng.random(img.shape) < 0.001
            img[hot] += 1500
            np.clip(img, 1, 4095).astype(np.uint16).tofile(f)


def sha(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for chunk in iter(lambda: f.read(1 << 24), b""):
            h.update(chunk)
    return h.hexdigest()


def commands(strip):
    return {
        "rrc-calib": (["rrc-calib", "--pan", strip, "--rrc-pan", "out.rrc.csv", "--force"], "out.rrc.csv"),
        "quicklook": (["quicklook", strip, "-o", "out.QL.TIFF", "--force"], "out.QL.TIFF"),
        "mtfc": (["mtfc", strip, "--mtf-x", "0.3", "--mtf-y", "0.45", "-o", "out.MTFC.RAW", "--force"], "out.MTFC.RAW"),
        "despike": (["despike", strip, "--threshold", "200", "-o", "out.DSPK.RAW", "--force"], "out.DSPK.RAW"),
    }


def run(oip, args, cwd, limit):
    env = dict(os.environ, LOGFILE=os.path.join(cwd, "oip.log"))
    t0 = time.perf_counter()
    r = subprocess.run(["timeout", "-k", "10", str(int(limit)), oip] + args, cwd=cwd, env=env, capture_output=True, text=True)
    wall = time.perf_counter() - t0
    if r.returncode != 0:
        sys.exit("%s %s: exit status %d after %.1f s\n%s%s" % (oip, " ".join(args), r.returncode, wall, r.stdout[-2000:], r.stderr[-2000:]))
    m = re.findall(r"(\d+) bytes in ([0-9.]+) seconds", r.stdout)
    if not m:
        sys.exit("%s %s: no closing line\n%s" % (oip, " ".join(args), r.stdout[-2000:]))
    return {"tool_seconds": float(m[-1][1]), "wall_seconds": wall, "bytes": int(m[-1][0])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--new", default=os.path.join(ROOT, "opticalimageprocessor_amd", "lib", "oip"))
    ap.add_argument("--dir", default=None)
    ap.add_argument("--lines", type=int, default=60000)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    binaries = {"parent": os.path.abspath(a.parent), "new": os.path.abspath(a.new)}
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        strip = os.path.join(d, "STRIP.RAW")
        make_strip(strip, a.lines)
        res = {"tool": "raster_tools_cli_bench", "W": W, "lines": a.lines, "strip_bytes": os.path.getsize(strip), "runs": a.runs, "commands": {}}
        for name, (args, product) in commands(strip).items():
            c = {"parent": [], "new": []}
            limit, hashes = 600, {}
            for which, oip in binaries.items():                     # the warm-up runs: discarded, their products compared
                first = run(oip, args, d, limit)
                limit = max(60, 5 * first["wall_seconds"])
                hashes[which] = sha(os.path.join(d, product))
                print("%s %s warm-up: %.3f s (wall %.3f s)" % (name, which, first["tool_seconds"], first["wall_seconds"]), file=sys.stderr, flush=True)
            if hashes["parent"] != hashes["new"]:
                sys.exit("%s: the products of the two binaries differ" % name)
            for i in range(a.runs):
                for which, oip in binaries.items():
                    c[which].append(run(oip, args, d, limit))
                    print("%s %s run %d: %.3f s (wall %.3f s)" % (name, which, i, c[which][-1]["tool_seconds"], c[which][-1]["wall_seconds"]), file=sys.stderr,
                          flush=True)
            out = {"product_sha256": hashes["new"], "timeout_seconds": int(limit)}
            for which in binaries:
                t = [r["tool_seconds"] for r in c[which]]
                out[which] = {"runs": c[which], "tool_seconds_median": statistics.median(t), "tool_seconds_min": min(t), "tool_seconds_max": max(t),
                              "wall_seconds_median": statistics.median(r["wall_seconds"] for r in c[which])}
            spread = out["parent"]["tool_seconds_max"] - out["parent"]["tool_seconds_min"]
            out["parent_spread_seconds"] = spread
            out["within_parent_spread"] = out["new"]["tool_seconds_median"] <= out["parent"]["tool_seconds_median"] + spread
            res["commands"][name] = out
    print(json.dumps(res))


if __name__ == "__main__":
    main()
