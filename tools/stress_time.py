#!/usr/bin/env python3
"""Device time of the stress read-out next to the lazy macros' k_moments on LDC 256^3.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o st -- python3 tools/stress_time.py run
    python3 tools/stress_time.py summarize DIR profiles/stress_readout.json

run: REPS + 1 times (the first is a warm-up) one step, lbm_get_macros (one k_moments launch),
a whole-lattice lbm_get_stress and lbm_get_shear (wall_only = 0; k_stress, one launch per batch of
planes).  summarize: per repetition the summed kernel durations from the trace's device
timestamps, and their medians.
"""
import csv
import glob
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "lattice-boltzmann-method-gpu_amd"))
N, REPS = 256, 5


def run():
    import lbm_amd
    from lbm_amd import cases
    lbm_amd.require_gpu()
    lat = cases.ldc_device(N, N, N)
    lat.step(20, history=False)
    for _ in range(REPS + 1):
        lat.step(1, history=False)
        lat.macros()
        lat.stress()
        lat.shear(wall_only=False)
    print("n_fluid", lat.counts()["n_fluid"], "kernel_src", lbm_amd.kernel_fingerprint())
    lat.close()


def summarize(trace_dir, out_path):
    path = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"])
                   for r in csv.DictReader(open(path))), key=lambda r: r[0])
    mom = [(e - s) / 1e3 for s, e, n in rows if "k_moments" in n]
    st = [(e - s) / 1e3 for s, e, n in rows if "k_stress" in n]
    assert len(mom) == REPS + 1 and len(st) % (REPS + 1) == 0, (len(mom), len(st))
    per = len(st) // (REPS + 1)
    st_rep = [sum(st[i * per:(i + 1) * per]) for i in range(1, REPS + 1)]
    import lbm_amd
    res = {"lattice": f"LDC {N}^3 (device-generated cavity, single domain)", "reps": REPS,
           "method": "rocprofv3 --kernel-trace device timestamps, median over reps after one warm-up",
           "k_moments_us": round(statistics.median(mom[1:]), 1),
           "k_stress_launches_per_readout": per,
           "stress_plus_shear_us": round(statistics.median(st_rep), 1),
           "k_moments_us_all": [round(v, 1) for v in mom[1:]],
           "stress_plus_shear_us_all": [round(v, 1) for v in st_rep],
           "kernel_src": lbm_amd.kernel_fingerprint()}
    res["ratio"] = round(res["stress_plus_shear_us"] / res["k_moments_us"], 2)
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run()
    else:
        summarize(sys.argv[2], sys.argv[3])
