"""One hot key of a distinct-count window: a single long segment through K.segment_distinct
(validation, short pass, readback of the long-segment list, scratch fill, long pass) against
torch.unique on the same words; best of 5, host time around a device sync. One JSON line per
case (1 Mi and 16 Mi words; 10,000 different values, and all different)."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mxstream.ops import kernels as K  # noqa: E402

dev = torch.device("cuda", 0)
out = []
for n in (1 << 20, 1 << 24):
    for name, nvals in (("10000 values", 10_000), ("all distinct", 0)):
        g = torch.Generator(device=dev).manual_seed(5)
        if nvals:
            pool = torch.randint(-2**62, 2**62, (nvals,), device=dev, generator=g)
            w = pool[torch.randint(0, nvals, (n,), device=dev, generator=g)].contiguous()
        else:
            w = (torch.randperm(n, device=dev, generator=g) * 0x9E3779B97F4A7C15).contiguous()
        heads = torch.zeros(1, dtype=torch.int64, device=dev)
        ts = {}
        for label, fn in (("segment_distinct", lambda: K.segment_distinct(heads, w)),
                          ("torch.unique", lambda: torch.unique(w).numel())):
            r = fn()
            torch.cuda.synchronize()
            best = 1e9
            for _ in range(5):
                t0 = time.perf_counter()
                r = fn()
                torch.cuda.synchronize()
                best = min(best, time.perf_counter() - t0)
            ts[label] = (best * 1e3, int(r) if not torch.is_tensor(r) else int(r[0]))
        assert ts["segment_distinct"][1] == ts["torch.unique"][1], ts
        out.append({"n": n, "contents": name, "distinct": ts["segment_distinct"][1],
                    "segment_distinct_ms": round(ts["segment_distinct"][0], 3),
                    "torch_unique_ms": round(ts["torch.unique"][0], 3)})
        print(json.dumps(out[-1]), flush=True)
