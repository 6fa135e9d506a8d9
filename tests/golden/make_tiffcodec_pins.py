"""Records tests/golden/tiff_refusals.json and tests/golden/tiff_writer_digests.json: what tests/cpp/tiffcodec_pin.cpp reports of
the codec in the tree it is run in.  They were recorded once, from the commit before the codec was refactored, and pin it since:
do not run this again unless the codec is MEANT to read or write something else."""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import test_tiffcodec_pin_cpu as T  # noqa: E402

with tempfile.TemporaryDirectory() as d:
    exe = T.build_program(d)
    os.mkdir(os.path.join(d, "r"))
    os.mkdir(os.path.join(d, "w"))
    for name, data in (("tiff_refusals.json", T.collect_reader(exe, os.path.join(d, "r"))),
                       ("tiff_writer_digests.json", T.collect_writers(exe, os.path.join(d, "w")))):
        with open(os.path.join(HERE, name), "w") as f:
            json.dump(data, f, indent=1, sort_keys=True)
            f.write("\n")
