#!/usr/bin/env python3
"""Interval-join kernel figures of a traced config 14 run.

  rocprofv3 --kernel-trace --output-format csv -d DIR -o c14 -- \\
      python -m mxstream.models.bench_configs --config 14 --warmup 0 --steps K [--zipf S] > RUN.json
  python scripts/interval_join_trace.py DIR/c14_kernel_trace.csv RUN.json

With --warmup 0 the run's own `pairs` is the pair total of every traced launch, so the expand
bandwidth is 32 B x pairs / the summed time of every ijoin_expand_kernel launch. The yardstick
from the same trace is the benchmark's fill of one step's bytes (the five largest fill launches).
Every other kernel of the step (the radix sort's, the event generator's, torch's own) is summed
under its own name. Prints one JSON line."""
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
        short = "fill" if "FillFunctor" in name else (m.group(1) if m else name.split("(")[0][-60:])
        dur.setdefault(short, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    pairs, steps = run["pairs"], run["pairs"] // max(1, run["pairs_per_step"])
    out = {"zipf": run["zipf"], "events_per_side_and_step": run["events_per_side_and_step"],
           "steps": steps, "pairs": pairs, "kernels": {}}
    fills = sorted(dur.pop("fill", []))[-5:]
    for k, d in sorted(dur.items(), key=lambda kv: -sum(kv[1])):
        out["kernels"][k] = {"launches": len(d), "total_us": round(sum(d), 1),
                             "us_per_step": round(sum(d) / max(1, steps), 1),
                             "median_us": round(statistics.median(d), 1)}
    exp_us = sum(dur.get("ijoin_expand_kernel", []))
    fill_us = statistics.median(fills)
    out["expand_TBps"] = round(32 * pairs / exp_us / 1e6, 3)
    out["fill_us"] = round(fill_us, 1)
    out["fill_TBps"] = round(32 * run["pairs_per_step"] / fill_us / 1e6, 3)
    out["expand_over_fill_time_per_byte"] = round(out["fill_TBps"] / out["expand_TBps"], 3)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
