#!/usr/bin/env python3
"""Kernel figures of a traced config 15 run (keyed latest-value lookup).

  rocprofv3 --kernel-trace --output-format csv -d DIR -o c15 -- \\
      python -m mxstream.models.bench_configs --config 15 --warmup 0 --steps K [--when none] > RUN.json
  python scripts/lookup_trace.py DIR/.../c15_kernel_trace.csv RUN.json

Every kernel of the run is summed under its own name: the lookup kernels, the radix sort's passes
of the rule upsert, the event generator's, and torch's own (the yardstick composition that the
benchmark times in the same call: index gathers, compare, nonzero's select). With the bytes a
step's mask pass has to move (16 B of sample columns and one 16-B table row per sample) the mask
kernel's rate comes out as well. Prints one JSON line."""
import csv
import json
import re
import statistics
import sys


def main(trace_csv: str, run_json: str) -> int:
    run = json.loads([ln for ln in open(run_json) if ln.startswith("{")][-1])
    dur: dict[str, list[float]] = {}
    for row in csv.DictReader(open(trace_csv)):
        name = row["Kernel_Name"]
        m = re.search(r"(\w+_kernel)\b", name)
        short = m.group(1) if m else re.sub(r"^void |\(.*$", "", name)[:70]
        dur.setdefault(short, []).append(
            (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    steps, batch = run["steps"], run["samples_per_step"]
    out = {"when": run["when"], "zipf": run["zipf"], "keys": run["keys"],
           "samples_per_step": batch, "steps": steps, "kernels": {}}
    for k, d in sorted(dur.items(), key=lambda kv: -sum(kv[1])):
        out["kernels"][k] = {"launches": len(d), "total_us": round(sum(d), 1),
                             "median_us": round(statistics.median(d), 1)}
    for k, nbytes in (("lookup_mask_kernel", 32 * batch), ("lookup_gather_kernel", 64 * batch)):
        if k in dur:
            out[k + "_TBps"] = round(nbytes / statistics.median(dur[k]) / 1e6, 3)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
