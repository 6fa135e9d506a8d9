"""Makes profiles/wallis_counters.json from hardware counters of profiles/wallis_bench.py, collected with rocprofv3 in processes of
their own (counters alone, no tracing beside them; one process per set, as many counters as one pass holds):

    rocprofv3 --pmc SQ_WAVES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_ACTIVE_INST_VALU SQ_INSTS_VALU SQ_WAIT_INST_ANY GRBM_GUI_ACTIVE \\
              --output-format csv -d OUT/set1 -- python profiles/wallis_bench.py --reps 2
    rocprofv3 --pmc SQ_WAVES SQ_WAVE_CYCLES SQ_WAIT_INST_LDS SQ_ACTIVE_INST_LDS SQ_LDS_BANK_CONFLICT SQ_INSTS_LDS SQ_INST_CYCLES_VMEM \\
              GRBM_GUI_ACTIVE --output-format csv -d OUT/set2 -- python profiles/wallis_bench.py --reps 2
    python profiles/wallis_counters.py OUT/set1 OUT/set2 > profiles/wallis_counters.json

Per run of the bench and counter: the mean over its dispatches (3 warm-up rounds + the repetitions) and their number.  The runs
are told apart by the kernel's name; the two runs of wallis_apply_u16_kernel<4> (B 128, then B 32 in every round of the bench)
by their order of dispatch.  The derived figures that profiles/wallis_speed.md quotes are added per run: the bench's raster is
6144 x 60000 x 4 samples, the device has 1024 SIMDs, GRBM_GUI_ACTIVE is summed over its 8 XCDs, and a wave64 instruction holds
its SIMD for 4 cycles at full rate."""
import collections
import csv
import glob
import json
import sys

SAMPLES = 6144 * 60000 * 4
SIMDS, XCDS = 1024, 8
RUNS = (("rrc_u16_flat_kernel", ("rrc",)), ("wallis_apply_u16_kernel<4>", ("apply_spp4_b128", "apply_spp4_b32")),
        ("wallis_apply_u16_kernel<1>", ("apply_spp1_b128",)), ("block_moments_u16_kernel<4, 128>", ("moments_spp4_b128",)),
        ("block_moments_u16_kernel<4, 32>", ("moments_spp4_b32",)), ("block_moments_u16_kernel<4, 256>", ("moments_spp4_b256",)),
        ("block_moments_u16_kernel<1, 128>", ("moments_spp1_b128",)), ("noise_blocks_u16_kernel<4, 8>", ("noise_spp4_b8",)))


def read_set(directory):
    """{run: {counter: (mean, dispatches)}}"""
    rows = collections.defaultdict(lambda: collections.defaultdict(dict))              # kernel key -> dispatch id -> counter -> value
    for f in glob.glob(directory + "/**/*counter_collection.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            for key, _ in RUNS:
                if key in r["Kernel_Name"]:
                    rows[key][int(r["Dispatch_Id"])][r["Counter_Name"]] = float(r["Counter_Value"])
    out = {}
    for key, names in RUNS:
        ids = sorted(rows[key])
        for k, name in enumerate(names):
            mine = ids[k::len(names)]
            if mine:
                out[name] = {c: [sum(rows[key][i][c] for i in mine) / len(mine), len(mine)] for c in sorted(rows[key][mine[0]])}
    return out


def derive(run):
    c = {k: v[0] for k, v in run.items()}
    d = {}
    if "GRBM_GUI_ACTIVE" in c:
        cycles = c["GRBM_GUI_ACTIVE"] / XCDS
        d["cycles_of_the_launch"] = cycles
        if "SQ_INSTS_VALU" in c:
            d["valu_instructions_per_sample"] = c["SQ_INSTS_VALU"] * 64 / SAMPLES
            d["valu_issue_share_at_full_rate"] = c["SQ_INSTS_VALU"] * 4 / SIMDS / cycles
        if "SQ_WAVE_CYCLES" in c:
            d["waves_resident_per_simd"] = c["SQ_WAVE_CYCLES"] * 4 / SIMDS / cycles
    if "SQ_WAVE_CYCLES" in c:
        for name, key in (("wait_any_share_of_wave_life", "SQ_WAIT_INST_ANY"), ("wait_lds_share_of_wave_life", "SQ_WAIT_INST_LDS")):
            if key in c:
                d[name] = c[key] / c["SQ_WAVE_CYCLES"]
    return d


def main():
    res = {"tool": "wallis_counters", "note": "[mean per dispatch, dispatches]; derived: see profiles/wallis_counters.py"}
    for k, directory in enumerate(sys.argv[1:]):
        s = read_set(directory)
        res["set%d" % (k + 1)] = {name: dict(counters=run, derived=derive(run)) for name, run in s.items()}
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
