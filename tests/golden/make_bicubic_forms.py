#!/usr/bin/env python3
"""Records tests/golden/bicubic_forms.json: SHA-256 of every output of the 8-pixels-per-lane bicubic kernels.

Run on the MI355X, with the library built from the commit whose bits are to be pinned (it needs the GPU, not oracle/_ref):
    python tests/golden/make_bicubic_forms.py --commit <hash of that commit> [--out FILE]

The file holds the commit hash, the SHA-256 of every input array (tests/_bicubic_forms.py generates them) and of every
output raster; no rasters.  tests/test_gpu_bicubic_golden.py checks a build against it.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _bicubic_forms as bf  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="hash of the commit the loaded library was built from")
    ap.add_argument("--out", default=os.path.join(HERE, "bicubic_forms.json"))
    args = ap.parse_args()
    import torch
    import opticalimageprocessor_amd as oip
    bf.check_shift_properties()
    ctx = oip.Context(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream)
    outputs = {}
    for shift in bf.SHIFTS:
        for f16 in (False, True):
            outputs[bf.remap_key(shift, f16)] = {k: bf.sha(v) for k, v in bf.run_remap_forms(ctx, shift, f16).items()}
        # the two accumulate modes are different arithmetic, and the window forms do store
        a, b = outputs[bf.remap_key(shift, False)], outputs[bf.remap_key(shift, True)]
        assert all(a[k] != b[k] for k in a), "fp16 accumulate gave the f32 bits"
    outputs["align"] = {"align_mss": bf.sha(bf.run_align(ctx))}
    ctx.close()
    rec = {"commit": args.commit, "geometry": {"W": bf.W, "L": bf.L, "section_rows": bf.SECTION_ROWS, "row_guard": bf.ROW_GUARD,
                                               "seed": bf.SEED, "align_case": list(bf.align_case())},
           "inputs": bf.input_hashes(), "outputs": outputs}
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("recorded %d output hashes in %s" % (sum(len(v) for v in outputs.values()), args.out))


if __name__ == "__main__":
    main()
