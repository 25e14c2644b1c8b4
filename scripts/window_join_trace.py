#!/usr/bin/env python3
"""Join kernel figures of a traced config 13 run.

  rocprofv3 --kernel-trace --output-format csv -d DIR -o c13 -- \\
      python -m mxstream.models.bench_configs --config 13 --warmup 0 --steps K [--zipf S] > RUN.json
  python scripts/window_join_trace.py DIR/c13_kernel_trace.csv RUN.json

With --warmup 0 the run's own `pairs` is the pair total of every traced firing (the first one
holds a partial window and is small), so nothing is averaged over firings of different sizes:
expand bandwidth = 24 B x pairs / the summed time of every join_expand_kernel launch. The
yardstick from the same trace is the benchmark's fill of one firing's bytes (the five largest
fill launches). Prints one JSON line."""
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
        m = re.search(r"(\w+_kernel)\(", name)
        short = "fill" if "FillFunctor" in name else (m.group(1) if m else name)
        dur.setdefault(short, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    pairs, firings = run["pairs"], run["firings"]
    out = {"zipf": run["zipf"], "events_per_side_and_step": run["events_per_side_and_step"],
           "firings": firings, "pairs": pairs, "kernels": {}}
    for k in ("join_match_kernel", "join_tile_sums_kernel", "join_tile_scan_kernel",
              "join_tile_write_kernel", "join_expand_kernel"):
        d = dur.get(k, [])
        out["kernels"][k] = {"launches": len(d), "total_us": round(sum(d), 1),
                             "median_us": round(statistics.median(d), 1) if d else None,
                             "ps_per_pair": round(sum(d) * 1e6 / pairs, 3) if pairs else None}
    exp_us = sum(dur.get("join_expand_kernel", []))
    fills = sorted(dur.get("fill", []))[-5:]
    fill_us = statistics.median(fills)
    fill_bytes = 24 * run["pairs_per_firing"]
    out["expand_TBps"] = round(24 * pairs / exp_us / 1e6, 3)
    out["fill_us"] = round(fill_us, 1)
    out["fill_TBps"] = round(fill_bytes / fill_us / 1e6, 3)
    out["expand_over_fill_time_per_byte"] = round(out["fill_TBps"] / out["expand_TBps"], 3)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
