"""Benchmarks for the other BASELINE.json configs (bench.py runs config 3, the headline).

  python -m mxstream.models.bench_configs --config 1   # chapter1 threshold alert on CPU
  python -m mxstream.models.bench_configs --config 2   # keyed ValueState counter, 10k keys, 1 GPU
  python -m mxstream.models.bench_configs --config 4   # sliding 1 min / 10 s + lateness, 10M keys
  python -m mxstream.models.bench_configs --config 5   # session alert + host-DRAM spill
  python -m mxstream.models.bench_configs --config 6   # vector-metric window avg (MFMA reduce)
  python -m mxstream.models.bench_configs --config 9   # ComputeCpuMax through env.execute (file)

Each prints one JSON line: events/s and the step time (and p50 alert latency where alerts fire).
Config 1 runs the reference's exact text path: Java-semantics split + Double.parseDouble in the
C++ runtime (csrc/runtime.cpp) and the traced `usage > 90` predicate in the C++ twin of the
filter kernel (Main.java:21-31).
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import time

import numpy as np
import torch

from ..ops import expr as E
from ..ops import kernels as K
from ..ops.native import load
from ..runtime.rolling_operator import KeyedRollingOperator
from ..runtime.session_operator import KeyedSessionOperator
from ..runtime.window_operator import KeyedWindowOperator


def _sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)


def config1(steps: int, warmup: int, lines_per_step: int = 1 << 20, device: str = "cpu",
            threads: int = 4) -> dict:
    """Text lines "ts ip cpuN usage" -> parse -> filter usage > 90 -> alerts. BASELINE config 1
    is the CPU path (C++ runtime, `threads` parse threads over newline-aligned chunks; the
    reference job runs at parallelism 4); device="cuda" runs the same job through the GPU
    parse kernel (csrc/parse_hip.hip) and the fused filter kernel."""
    m = load()
    rng = np.random.default_rng(1)
    hosts = [f"10.8.{i // 256}.{i % 256}" for i in range(1024)]
    usage = rng.uniform(0, 100, lines_per_step)
    h = rng.integers(0, len(hosts), lines_per_step)
    cpu = rng.integers(0, 64, lines_per_step)
    text = "\n".join(f"1563452056 {hosts[a]} cpu{b} {u:.1f}" for a, b, u in zip(h, cpu, usage)).encode()
    d = m.StringDict()
    prog = E.compile_expr(E.var(0) > 90)
    spec = [(1, 0), (2, 0), (3, 1)]  # host (dict id), cpu (dict id), usage (double)

    def step_cpu():
        cols, n, err_idx, err = m.parse_lines(text, spec, " ", d, 0, threads)
        x = torch.from_numpy(cols[2])
        keep = K.expr_filter(x, prog)
        return int(keep.sum())

    gspec = [(1, 0), (2, 0), (3, 1)]

    if device != "cpu":
        from ..ops.text import parse_text_gpu, pinned_text_batch

        # The socket reader fills pinned ring slots (SURVEY.md F-src); the bench hands the
        # parser one such slot per step. Every step's batch crosses PCIe (H2D DMA) inside the
        # timed loop: the copy of batch i+1 runs on a copy stream while batch i is parsed and
        # filtered (two device text buffers), as the ingest ring does.
        pinned = pinned_text_batch(text)
        gdev = torch.device(device)
        copy_stream = torch.cuda.Stream(gdev)
        dbufs = [torch.empty(len(text), dtype=torch.uint8, device=gdev) for _ in range(2)]
        up_ev, free_ev = [None, None], [None, None]
        state = {"i": 0}

        def upload(i):
            s = i & 1
            with torch.cuda.stream(copy_stream):
                if free_ev[s] is not None:
                    copy_stream.wait_event(free_ev[s])  # the parse of batch i-2 read this buffer
                dbufs[s].copy_(pinned, non_blocking=True)
                up_ev[s] = torch.cuda.Event()
                up_ev[s].record(copy_stream)

        upload(0)

    def step_gpu():
        i = state["i"]
        s = i & 1
        upload(i + 1)
        cols = parse_text_gpu(dbufs[s], gspec, " ", 0, device, ready=up_ev[s])
        # Order-preserving compaction of the alerting rows (mask/scan/write kernels), then the
        # alert rows (host, cpu, usage) gathered on the device in input order.
        idx, total = K.expr_filter_compact(cols[2], prog)
        c = int(total.item())
        # string fields are (dictionary ids, Java hashes): the alert carries the ids
        alerts = [(col[0] if isinstance(col, tuple) else col)[idx[:c]] for col in cols]
        free_ev[s] = torch.cuda.Event()
        free_ev[s].record(torch.cuda.current_stream(gdev))
        state["i"] = i + 1
        return int(alerts[2].numel())

    step = step_gpu if device != "cpu" else step_cpu
    if device == "cpu":
        # The CPU path is the C++ runtime: `threads` parse threads and as many filter threads;
        # torch's intra-op pool only adds fork/join overhead to the tiny tensor ops per step.
        torch.set_num_threads(1)
        m.cpu_set_threads(threads)

    for _ in range(warmup):
        step()
    t0 = time.perf_counter()
    alerts = 0
    for _ in range(steps):
        alerts += step()
    dt = time.perf_counter() - t0
    ev = lines_per_step * steps
    return {"config": 1, "metric": "events/sec (threshold alert: parse + filter)", "value": ev / dt,
            "unit": "events/s", "ms_per_step": dt / steps * 1e3, "alerts": alerts,
            "lines_per_step": lines_per_step,
            "threads": threads if device == "cpu" else None,
            "device": f"cpu ({threads} threads)" if device == "cpu" else
            f"{device} (pinned H2D text on a copy stream, one batch ahead + LDS-tiled GPU parse)"}


def config2(steps: int, warmup: int, batch: int = 1 << 24, keys: int = 10_000,
            device: str = "cuda", dense_keys: bool = True, sort_free: bool = True) -> dict:
    """Keyed ValueState counter: count += 1 per record, per-record post-update value; alerts
    (rows copied to the host) when a key's count crosses a multiple of 1000 (each key gets
    ~1.7K records per step at 10k keys, so every step emits: the emit compaction and its D2H are
    in the timed region). dense_keys: the
    keys are dictionary ids (as columnar ingest produces), slot = id; else hashed state."""
    dev = torch.device(device)
    dense_keys = dense_keys and dev.type == "cuda" and sort_free
    op = KeyedRollingOperator(agg=K.AGG_COUNT, device=dev, max_keys=keys, batch_capacity=batch,
                              filter_prog=E.compile_expr(E.var(E.VAR_COUNT) % 1000 == 0),
                              emit_capacity=1 << 20, dense_keys=dense_keys)
    op.sort_free = sort_free
    kt = torch.empty(batch, dtype=torch.int64, device=dev)
    tt = torch.empty_like(kt)
    vt = torch.empty_like(kt)
    step_i = [0]

    def step():
        K.gen_events(kt, tt, vt, seed=2, stream_id=0, idx0=step_i[0] * batch, nkeys=keys,
                     ts_base=0, ts_span=1000, disorder=0, val_lo=0, val_span=100)
        rows = op.process(kt, vt)
        step_i[0] += 1
        return len(rows.keys)

    for _ in range(warmup):
        step()
    _sync(dev)
    t0 = time.perf_counter()
    alerts = 0
    for _ in range(steps):
        alerts += step()
    _sync(dev)
    dt = time.perf_counter() - t0
    return {"config": 2, "keyed_state": "dense" if dense_keys else "hashed",
            "path": "sort-free" if sort_free else "radix-sort",
            "metric": f"events/sec (keyed ValueState counter, {keys // 1000}k keys)",
            "value": batch * steps / dt, "unit": "events/s", "ms_per_step": dt / steps * 1e3,
            "alerts": alerts, "keys": keys, "events_per_step": batch, "device": str(dev)}


def config11(steps: int, warmup: int, batch: int = 1 << 24, keys: int = 10_000,
             size: int = 100, slide: int | None = None, device: str = "cuda") -> dict:
    """Keyed count-window sum on the sort path, config 2's batch and key space: ``countWindow(size,
    slide)`` (the pane scan), or without `slide` the tumbling ``countWindow(size)`` on the same
    data (the segmented scan it is measured against). The fired rows stay on the device (the
    sliding window of slide 1 fires on every element); their count is read once at the end."""
    dev = torch.device(device)
    op = KeyedRollingOperator(agg=K.AGG_SUM_I64, device=dev, max_keys=keys, batch_capacity=batch,
                              count_window=size, count_slide=slide or 0)
    op.sort_free = False
    kt = torch.empty(batch, dtype=torch.int64, device=dev)
    tt = torch.empty_like(kt)
    vt = torch.empty_like(kt)
    step_i = [0]
    fired = torch.zeros(1, dtype=torch.int64, device=dev)

    def step():
        K.gen_events(kt, tt, vt, seed=2, stream_id=0, idx0=step_i[0] * batch, nkeys=keys,
                     ts_base=0, ts_span=1000, disorder=0, val_lo=0, val_span=100)
        fired.add_(op.process(kt, vt, to_host=False))
        step_i[0] += 1

    for _ in range(warmup):
        step()
    fired.zero_()
    _sync(dev)
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    _sync(dev)
    dt = time.perf_counter() - t0
    op.check()
    pane = math.gcd(size, slide) if slide else size
    return {"config": 11, "window": "sliding" if slide else "tumbling", "size": size,
            "slide": slide or size, "pane": pane, "panes_per_window": size // pane,
            "metric": f"events/sec (keyed count-window sum, {keys // 1000}k keys, radix-sort path)",
            "value": batch * steps / dt, "unit": "events/s", "ms_per_step": dt / steps * 1e3,
            "rows": int(fired.item()), "keys": keys, "events_per_step": batch,
            "device": str(dev)}


def config12(steps: int, warmup: int, batch: int = 1 << 24, keys: int = 10_000,
             size: int = 0, by: str | None = None, device: str = "cuda") -> dict:
    """Keyed rolling max (or with `size` the tumbling ``countWindow(size)`` max) on config 11's
    data and sort path; with `by` ("max" / "min") the arg-select scan of ``maxBy`` / ``minBy`` on
    the same data, which also says which record holds the extremum. val_span = 100 over 1,678
    events per key and step: ties are everywhere. Rows stay on the device; their count is read
    once at the end."""
    dev = torch.device(device)
    if by not in (None, "max", "min"):
        raise ValueError("config 12: --by max | min")
    op = KeyedRollingOperator(agg=K.AGG_MIN_I64 if by == "min" else K.AGG_MAX_I64, device=dev,
                              max_keys=keys, batch_capacity=batch, count_window=size,
                              arg_select=by is not None)
    op.sort_free = False
    kt = torch.empty(batch, dtype=torch.int64, device=dev)
    tt = torch.empty_like(kt)
    vt = torch.empty_like(kt)
    step_i = [0]
    fired = torch.zeros(1, dtype=torch.int64, device=dev)

    def step():
        K.gen_events(kt, tt, vt, seed=2, stream_id=0, idx0=step_i[0] * batch, nkeys=keys,
                     ts_base=0, ts_span=1000, disorder=0, val_lo=0, val_span=100)
        fired.add_(op.process(kt, vt, to_host=False))
        step_i[0] += 1

    for _ in range(warmup):
        step()
    fired.zero_()
    _sync(dev)
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    _sync(dev)
    dt = time.perf_counter() - t0
    op.check()
    r = {"config": 12, "scan": f"arg-select ({by}By)" if by else "value (max)",
         "window": f"countWindow({size})" if size else "rolling",
         "metric": f"events/sec (keyed {'count-window' if size else 'rolling'} "
                   f"{by or 'max'}{'By' if by else ''}, {keys // 1000}k keys, radix-sort path)",
         "value": batch * steps / dt, "unit": "events/s", "ms_per_step": dt / steps * 1e3,
         "rows": int(fired.item()), "keys": keys, "events_per_step": batch, "device": str(dev)}
    if by:
        # rows whose winner was the record already held in state, in the last step
        n = min(op.check(), op.out_src.numel())
        r["stored_winner_rows_last_step"] = int((op.out_src[:n] == -1).sum().item())
    return r


def config2_spill(steps: int, warmup: int, batch: int = 1 << 22, active: int = 500_000,
                  drift: int = 50_000, table_keys: int = 1_000_000, revisit: float = 0.01,
                  device: str = "cuda") -> dict:
    """Keyed ValueState counter (config 2's operator, hashed keys) over a key space that outgrows
    the HBM table: each step's events come from `active` consecutive ids whose window moves by
    `drift` per step, and `revisit` of the events go to keys that went idle ~10 steps ago (their
    counts live in host DRAM by then and come back before the step folds them). Reports events/s,
    spilled / promoted keys and the host tier's size."""
    dev = torch.device(device)
    op = KeyedRollingOperator(agg=K.AGG_COUNT, device=dev, max_keys=table_keys,
                              batch_capacity=batch,
                              # a key lives ~10 steps x ~8 events: every 64th count alerts,
                              # so the emit path runs inside the timed steps
                              filter_prog=E.compile_expr(E.var(E.VAR_COUNT) % 64 == 0),
                              emit_capacity=1 << 20, spill=True)
    kt = torch.empty(batch, dtype=torch.int64, device=dev)
    tt = torch.empty_like(kt)
    vt = torch.empty_like(kt)
    step_i = [0]
    stride = max(2, round(1.0 / revisit)) if revisit > 0 else 0
    rev = [None, None]

    def step():
        i = step_i[0]
        K.gen_events(kt, tt, vt, seed=2, stream_id=0, idx0=i * batch, nkeys=active, ts_base=0,
                     ts_span=1000, disorder=0, val_lo=0, val_span=100, key_base=i * drift)
        if stride and i >= 12:
            # every stride-th event: a key of the drift window 10 steps back (its own draw; a
            # strided int64 remainder_ cost milliseconds of host time per step)
            old = kt[::stride]
            if rev[0] is None or rev[0].numel() != old.numel():
                rev[0] = torch.empty(old.numel(), dtype=torch.int64, device=dev)
                rev[1] = torch.empty_like(rev[0])
            K.gen_events(rev[0], rev[1], rev[1], seed=22, stream_id=1, idx0=i * old.numel(),
                         nkeys=drift, ts_base=0, ts_span=1, disorder=0, val_lo=0, val_span=1,
                         key_base=(i - 10) * drift)
            old.copy_(rev[0])
        rows = op.process(kt, vt)
        step_i[0] += 1
        return len(rows.keys)

    for _ in range(warmup):
        step()
    _sync(dev)
    st0 = dict(op.spill_stats)
    t0 = time.perf_counter()
    alerts = 0
    for _ in range(steps):
        alerts += step()
    _sync(dev)
    dt = time.perf_counter() - t0
    return {"config": "2-spill", "metric": "events/sec (keyed ValueState counter, key space "
            "outgrowing HBM, host-DRAM tier)", "value": batch * steps / dt, "unit": "events/s",
            "ms_per_step": dt / steps * 1e3, "alerts": alerts, "events_per_step": batch,
            "table_keys": table_keys, "active_keys": active, "drift_per_step": drift,
            "revisit": revisit,
            **{k: op.spill_stats[k] - st0[k] for k in op.spill_stats},
            "host_keys": len(op.store), "host_bytes": op.host_bytes(),
            "resident_keys": op.live_keys, "device": str(dev)}


def config4(steps: int, warmup: int, batch: int = 1 << 24, keys: int = 10_000_000,
            device: str = "cuda", dense_keys: bool = True, pipeline="stream",
            latency_fire: int = 0) -> dict:
    """Sliding 1 min / 10 s event-time window sum + 30 s allowed lateness, 10M keys; 5 % of
    events arrive up to 40 s late (within lateness -> re-firings)."""
    dev = torch.device(device)
    span = 2_000
    mbps = E.var(E.VAR_RESULT) * 8.0 / 60 / 1024 / 1024
    # Alert on keys whose 1-min volume is < 70 % of the expected (Poisson tail, ~2 %).
    exp_sum = batch * (60_000 / span) / keys * 10_000
    thr = 0.7 * exp_sum * 8.0 / 60 / 1024 / 1024
    op = KeyedWindowOperator(size=60_000, slide=10_000, lateness=30_000, agg=K.AGG_SUM_I64,
                             device=dev, max_keys=keys, batch_capacity=batch, ooo_bound=5_000,
                             map_prog=E.compile_expr(mbps),
                             filter_prog=E.compile_expr(E.var(E.VAR_MAPPED) < thr),
                             dense_keys=dense_keys, pipeline=pipeline, emit="key_value",
                             latency_fire=latency_fire)
    # dense keyed state: the keys are dictionary ids (int32, as the columnar ingest emits them)
    kt = torch.empty(batch, dtype=torch.int32 if dense_keys else torch.int64, device=dev)
    tt = torch.empty(batch, dtype=torch.int64, device=dev)
    vt = torch.empty_like(tt)
    late_n = batch // 20
    step_i = [0]
    lat = []

    t_ing = {}

    def account(fired):
        # latency: ingest of the batch that triggered the firing (FireResult.seq) -> rows here
        now = time.perf_counter()
        for seq in {r.seq for r in fired}:
            if seq in t_ing:
                lat.append((now - t_ing[seq]) * 1e3)
        return sum(len(r.keys) for r in fired)

    def step():
        t_in = time.perf_counter()
        i = step_i[0]
        K.gen_events(kt, tt, vt, seed=4, stream_id=0, idx0=i * batch, nkeys=keys,
                     ts_base=i * span, ts_span=span, disorder=5_000, val_lo=0, val_span=20_000)
        if i > 20:
            tt[:late_n] -= 40_000  # late but (mostly) within the allowed lateness
        t_ing[op.metrics.steps + 1] = t_in
        fired = op.process(kt, tt, vt)
        step_i[0] += 1
        return account(fired)

    # Steady state: the first windows (started before the stream) hold a partial minute of
    # data and nearly every key of them is below the alert threshold -- an artefact of the
    # stream start, not the workload. The untimed warmup covers the first full window (60 s of
    # event time = 30 steps) and the onset of late data (step 21).
    warmup = max(warmup, 32)
    for _ in range(warmup):
        step()
    _sync(dev)
    lat.clear()
    t0 = time.perf_counter()
    alerts = 0
    for _ in range(steps):
        alerts += step()
    alerts += account(op.flush())  # pipelined: the last state half
    _sync(dev)
    dt = time.perf_counter() - t0
    return {"config": 4, "warmup": warmup, "keyed_state": "dense" if dense_keys else "hashed", "metric": "events/sec (sliding 1min/10s + lateness, 10M keys)",
            "value": batch * steps / dt, "unit": "events/s", "ms_per_step": dt / steps * 1e3,
            "p50_alert_latency_ms": statistics.median(lat) if lat else None,
            "p99_alert_latency_ms": (sorted(lat)[min(len(lat) - 1, int(0.99 * len(lat)))]
                                     if lat else None),
            "firings_measured": len(lat), "latency_fire": latency_fire,
            "latency_fire_steps": op.metrics.extra.get("latency_fires", 0), "alerts": alerts,
            "late_dropped": op.metrics.num_late_records_dropped, "keys": keys,
            "events_per_step": batch, "state_bytes": op.state_bytes(), "device": str(dev)}


def _gc_settle() -> None:
    """MXS_GC_FREEZE=1: after the warmup, collect once and move every surviving object to the
    permanent generation (gc.freeze), so the cyclic collector's full passes no longer walk the
    job's long-lived state during the timed steps (A/B knob)."""
    import gc
    import os

    if os.environ.get("MXS_GC_FREEZE", "0") == "1":
        gc.collect()
        gc.freeze()
    # MXS_SWITCH_INTERVAL=<seconds>: the interpreter's thread switch interval (A/B of GIL
    # hand-offs between the step and the spill worker; Python's default is 0.005).
    if os.environ.get("MXS_SWITCH_INTERVAL"):
        __import__("sys").setswitchinterval(float(os.environ["MXS_SWITCH_INTERVAL"]))


def _cgroup_cpu_stat() -> dict:
    try:
        with open("/sys/fs/cgroup/cpu.stat") as f:
            return {k: int(v) for k, v in (ln.split() for ln in f if ln.strip())}
    except (OSError, ValueError):
        return {}


@__import__("contextlib").contextmanager
def _cpu_accounting():
    """Process CPU time and cgroup CPU throttling over the timed region, on stderr: a CPU quota
    exhausted by the process's threads stalls the stepping thread at arbitrary points."""
    import resource
    import sys
    import threading

    import gc

    gcs = {"n": [0, 0, 0], "ms": [0.0, 0.0, 0.0], "t": 0.0}

    def on_gc(phase, info):
        if phase == "start":
            gcs["t"] = time.perf_counter()
        else:
            g = info["generation"]
            gcs["n"][g] += 1
            gcs["ms"][g] += (time.perf_counter() - gcs["t"]) * 1e3

    gc.callbacks.append(on_gc)
    r0, c0, t0 = resource.getrusage(resource.RUSAGE_SELF), _cgroup_cpu_stat(), time.perf_counter()
    try:
        yield
    finally:
        gc.callbacks.remove(on_gc)
        print(f"gc in timed region: collections per generation {gcs['n']}, ms "
              f"{[round(x, 2) for x in gcs['ms']]}, tracked objects {len(gc.get_objects())}",
              file=sys.stderr)
        r1, c1, dt = resource.getrusage(resource.RUSAGE_SELF), _cgroup_cpu_stat(), \
            time.perf_counter() - t0
        cpu = (r1.ru_utime - r0.ru_utime) + (r1.ru_stime - r0.ru_stime)
        d = {k: c1[k] - c0.get(k, 0) for k in c1}
        print(f"timed region {dt * 1e3:.1f} ms: process cpu {cpu * 1e3:.1f} ms "
              f"({cpu / max(dt, 1e-9):.2f} cpus), py threads {threading.active_count()}, "
              f"cgroup {d}", file=sys.stderr)


@__import__("contextlib").contextmanager
def _timed_profile():
    """MXS_BENCH_PROFILE=<file>: cProfile of the timed region only (host hot spots without the
    warmup's one-time allocations), top entries by own time written to <file>."""
    out = __import__("os").environ.get("MXS_BENCH_PROFILE")
    if not out:
        with _cpu_accounting():
            yield
        return
    import cProfile
    import io
    import pstats

    prof = cProfile.Profile()
    prof.enable()
    try:
        yield
    finally:
        prof.disable()
        s = io.StringIO()
        st = pstats.Stats(prof, stream=s)
        st.sort_stats("tottime").print_stats(30)
        st.print_callers("empty|absorb|export")
        st.sort_stats("cumulative").print_stats(40)
        with open(out, "w") as f:
            f.write(s.getvalue())


def config4_spill(steps: int, warmup: int, batch: int = 1 << 22, active: int = 1_000_000,
                  drift: int = 100_000, table_keys: int = 2_000_000, device: str = "cuda") -> dict:
    """Config 4's sliding 1 min / 10 s window + 30 s lateness over a key space that outgrows the
    HBM table: each step draws its events from `active` consecutive key ids whose range moves by
    `drift` per step, so the keys live during a window's lifetime (90 s = 45 steps) number
    active + 45 * drift = 5.5M against a table sized for `table_keys` = 2M (>= 2x over). Hashed
    keyed state with the host-DRAM tier: every 4 steps, sub-tables above 80 % load evict the keys
    whose newest data is more than one pane old (window_compact -> pinned slab on the copy stream,
    absorbed by the C++ tier at the next boundary); firings export the tier's rows of the window
    and combine them with the device's rows ON THE DEVICE (tier_merge + fused epilogue).
    Reports events/s and the tier's size."""
    dev = torch.device(device)
    span = 2_000
    mbps = E.var(E.VAR_RESULT) * 8.0 / 60 / 1024 / 1024
    op = KeyedWindowOperator(size=60_000, slide=10_000, lateness=30_000, agg=K.AGG_SUM_I64,
                             device=dev, max_keys=table_keys, batch_capacity=batch,
                             ooo_bound=5_000, map_prog=E.compile_expr(mbps),
                             filter_prog=E.compile_expr(E.var(E.VAR_MAPPED) < 1e-4),
                             dense_keys=False, spill=True, spill_keep_panes=1,
                             spill_check_steps=4)
    kt = torch.empty(batch, dtype=torch.int64, device=dev)
    tt = torch.empty_like(kt)
    vt = torch.empty_like(kt)
    step_i = [0]

    def step():
        i = step_i[0]
        K.gen_events(kt, tt, vt, seed=41, stream_id=0, idx0=i * batch, nkeys=active,
                     ts_base=i * span, ts_span=span, disorder=2_000, val_lo=0, val_span=20_000,
                     key_base=i * drift)
        fired = op.process(kt, tt, vt)
        step_i[0] += 1
        return sum(len(r.keys) for r in fired)

    for _ in range(warmup):
        step()
    _sync(dev)
    with _timed_profile():
        t0 = time.perf_counter()
        alerts = 0
        for _ in range(steps):
            alerts += step()
        alerts += sum(len(r.keys) for r in op.flush())
        _sync(dev)
        dt = time.perf_counter() - t0
    ex = op.metrics.extra
    return {"config": "4-spill", "metric": "events/sec (sliding 1min/10s + lateness, key space "
            "outgrowing HBM, host-DRAM tier)", "value": batch * steps / dt, "unit": "events/s",
            "ms_per_step": dt / steps * 1e3, "alerts": alerts, "events_per_step": batch,
            "table_keys": table_keys, "live_keys_per_window": active + 45 * drift,
            "spilled_keys": ex.get("spilled_keys", 0), "spilled_rows": ex.get("spilled_rows", 0),
            "dropped_keys": ex.get("dropped_keys", 0), "async_evictions": ex.get("async_evictions", 0),
            "tier_merge": __import__("os").environ.get("MXS_TIER_MERGE", "device"),
            "pinned_slab_allocs": {k: getattr(getattr(op, a, None), "allocs", 0) for k, a in
                                   (("fire", "_pool"), ("tier", "_tier_pool"),
                                    ("evict", "_evict_pool"))},
            "host_tier_rows": op.host_tier.nrows,
            "host_tier_bytes": op.host_tier.nbytes, "hbm_state_bytes": op.state_bytes(),
            "device": str(dev)}


def config5(steps: int, warmup: int, batch: int = 1 << 24, active: int = 4_000_000,
            drift: int = 400_000, table_keys: int = 4_000_000, device: str = "cuda",
            revisit: float = 0.0, promote: bool = True, pipeline: bool | None = None,
            ckpt: bool = False) -> dict:
    """Session windows (gap 5 s, 30 s allowed lateness) over a drifting active key set: each step
    draws events from `active` consecutive key ids whose window advances by `drift` ids, so keys
    go idle and their sessions close. The HBM slot table holds `table_keys` keys; idle keys whose
    fired sessions are still inside the allowed lateness are spilled to the host-DRAM store.
    Alert: sessions whose volume exceeds 1.5x the expected mean (fused map/filter epilogue).
    revisit > 0: that fraction of events (every round(1/revisit)-th) goes to keys that went idle
    ~10 drift windows ago -- spilled keys whose records take the host-DRAM store path.
    pipeline: the operator's pipelined step (a batch's fire/spill host work overlaps the next
    batch's fold); its alerts come out one step later and their latency counts from the arrival
    of the batch that fired them; the timed loop ends with the drain (op.flush()). Default: on
    without revisits; with revisits the promotions join the spill worker every step and the
    unpipelined step is faster (1.86 G against 1.02 G: profiles/r6_cfg5r_unpipelined.json,
    profiles/r6_cfg5r.json)."""
    dev = torch.device(device)
    if pipeline is None:
        pipeline = revisit == 0
    span, gap = 2_000, 5_000
    per_key_step = batch / active
    # A key is active for active/drift steps; its session spans that time.
    exp_sum = per_key_step * (active / drift) * 5_000
    op = KeyedSessionOperator(gap=gap, lateness=30_000, agg=K.AGG_SUM_I64, device=dev,
                              max_keys=table_keys, batch_capacity=batch, ooo_bound=1_000,
                              sub_table_log2=int(__import__("os").environ.get("MXS_SESS_SUB_LOG2", 0))
                              or None,
                              idle_spill_ms=gap + 2 * span, spill_rows=1 << 22,
                              filter_prog=E.compile_expr(E.var(E.VAR_RESULT) > 1.5 * exp_sum),
                              pipeline=pipeline and dev.type == "cuda")
    op.promote_spilled = promote
    kt = torch.empty(batch, dtype=torch.int64, device=dev)
    tt = torch.empty_like(kt)
    vt = torch.empty_like(kt)
    step_i = [0]
    lat = []
    rev = [None, None]  # revisit keys / scratch
    t_prev = [None]  # pipelined: arrival of the batch whose fire the step returns

    def step():
        t_in = time.perf_counter()
        t_fired, t_prev[0] = (t_prev[0] if op.pipeline else t_in), t_in
        i = step_i[0]
        K.gen_events(kt, tt, vt, seed=5, stream_id=0, idx0=i * batch, nkeys=active,
                     ts_base=i * span, ts_span=span, disorder=1_000, val_lo=0, val_span=10_000,
                     key_base=i * drift)
        if revisit > 0 and i >= 12:
            # every stride-th event goes to a key of the drift window 10 steps back: its own
            # uniform draw over that window (gen_events), written over the strided events
            # (torch's int64 remainder_ on the strided view cost ~6 ms of host time per step)
            stride = max(2, round(1.0 / revisit))
            old = kt[::stride]
            if rev[0] is None or rev[0].numel() != old.numel():
                rev[0] = torch.empty(old.numel(), dtype=torch.int64, device=dev)
                rev[1] = torch.empty_like(rev[0])
            K.gen_events(rev[0], rev[1], rev[1], seed=55, stream_id=1, idx0=i * old.numel(),
                         nkeys=drift, ts_base=0, ts_span=1, disorder=0, val_lo=0, val_span=1,
                         key_base=(i - 10) * drift)
            old.copy_(rev[0])
        rows = op.process(kt, tt, vt)
        step_i[0] += 1
        if len(rows) and t_fired is not None:
            lat.append((time.perf_counter() - t_fired) * 1e3)
        return len(rows)

    for _ in range(warmup):
        step()
    _sync(dev)
    _gc_settle()
    lat.clear()
    op.phase_s.clear()
    m0 = dict(op.metrics.__dict__)
    alerts = 0
    with _timed_profile():
        t0 = time.perf_counter()
        for _ in range(steps):
            alerts += step()
        alerts += len(op.flush())  # pipelined: the last batch's fire and spill
        _sync(dev)
        dt = time.perf_counter() - t0
    mt = op.metrics
    ck = None
    if ckpt:  # after the timed loop: one synchronous checkpoint of both tiers (untimed above)
        import tempfile
        from pathlib import Path

        from ..runtime.checkpoint import write_operator_file

        ck = {"snapshot_ms": [], "write_ms": []}
        with tempfile.TemporaryDirectory() as d:
            for _ in range(2):
                _sync(dev)
                c0 = time.perf_counter()
                snap = op.snapshot_state()
                c1 = time.perf_counter()
                write_operator_file(Path(d), "session", 0, snap, op.max_parallelism)
                c2 = time.perf_counter()
                ck["snapshot_ms"].append(round((c1 - c0) * 1e3, 2))
                ck["write_ms"].append(round((c2 - c1) * 1e3, 2))
            # split of the snapshot: the two tiers' rows, then the key groups on the host
            from ..ops import kernels as KK

            _sync(dev)
            c0 = time.perf_counter()
            rows = op.snapshot()
            c1 = time.perf_counter()
            KK.keygroups(torch.from_numpy(np.ascontiguousarray(rows["key"], dtype=np.int64)),
                         max_parallelism=op.max_parallelism)
            c2 = time.perf_counter()
            ck["rows_ms"] = round((c1 - c0) * 1e3, 2)
            ck["keygroups_ms"] = round((c2 - c1) * 1e3, 2)
            ck["rows"] = int(len(snap.kg))
            ck["bytes"] = int(sum(v.nbytes for v in snap.columns.values()))
    return {"config": 5, "pipeline": op.pipeline, "checkpoint": ck, "metric": "events/sec (session-window alert + host-DRAM spill)",
            "value": batch * steps / dt, "unit": "events/s", "ms_per_step": dt / steps * 1e3,
            "p50_alert_latency_ms": statistics.median(lat) if lat else None,
            "p99_alert_latency_ms": (sorted(lat)[min(len(lat) - 1, int(0.99 * len(lat)))]
                                     if lat else None),
            "firings_measured": len(lat), "alerts": alerts,
            "tbase_redos": op.metrics.extra.get("tbase_redos", 0),
            "late_dropped": mt.num_late_records_dropped - m0["num_late_records_dropped"],
            "spilled_keys": mt.spilled_keys - m0["spilled_keys"],
            "records_to_host": mt.records_to_host - m0["records_to_host"],
            "records_promoted": mt.records_promoted - m0["records_promoted"],
            "promoted_keys": mt.promoted_keys - m0["promoted_keys"],
            "overflow_keys": mt.overflow_keys - m0["overflow_keys"],
            "host_store_bytes": op.host_bytes(), "resident_keys": op.resident_keys() if op.gpu else 0,
            "hbm_state_bytes": op.state_bytes() - op.host_bytes(), "events_per_step": batch,
            "active_keys": active, "table_keys": table_keys, "device": str(dev),
            "host_phase_ms_per_step": {k: round(v * 1e3 / steps, 2)
                                       for k, v in sorted(op.phase_s.items())},
            "spill_slab_allocs": op.metrics.extra.get("spill_slab_allocs", 0),
            "promote_bad_keys": op.metrics.extra.get("promote_bad_keys", 0),
            "spill_hot_rows": op.metrics.extra.get("spill_hot_rows", 0),
            "spill_jobs_with_hot_map": op.metrics.extra.get("spill_jobs_with_hot_map", 0),
            "spill_jobs": op.metrics.extra.get("spill_jobs", 0),
            "store_index": op.store.index_stats() if hasattr(op.store, "index_stats") else None}


def config6(steps: int, warmup: int, batch: int = 1 << 24, keys: int = 1_000_000,
            dim: int = 32, device: str = "cuda", mfma: bool = True, zipf: float = 0.0) -> dict:
    """Vector-metric window: 1-min tumbling event-time AVERAGE of a D-float metric vector per
    host (per-core CPU usage; ComputeCpuAvg.java:27-59 with the scalar generalised to a vector),
    1M keys, alert when any core's window average exceeds a threshold. The per-(key, pane)
    vector sums run on the MFMA segmented-sum kernel (mfma=False: the VALU variant)."""
    from ..ops import vector as V
    from ..runtime.vector_window_operator import VectorWindowOperator

    dev = torch.device("cuda", 0) if device != "cpu" and torch.cuda.is_available() \
        else torch.device("cpu")
    step_ms, disorder = 5_000, 2_000
    # Alert when some core's 1-min average usage is 4.4 sigma above the mean (U[0, 100) usage,
    # ~events_per_window samples per key): ~0.1 % of the (key, window) pairs.
    per_window = batch * (60_000 / step_ms) / keys
    thr = 50.0 + 4.4 * (100.0 / math.sqrt(12.0)) / math.sqrt(max(per_window, 1.0))
    op = VectorWindowOperator(dim=dim, size=60_000, device=dev, max_keys=keys,
                              batch_capacity=batch, ooo_bound=disorder, avg=True,
                              threshold=thr, mfma=mfma)
    k = torch.empty(batch, dtype=torch.int64, device=dev)
    ts = torch.empty_like(k)
    vals = torch.empty_like(k)
    vec = torch.empty(batch, dim, dtype=torch.float32, device=dev)
    t0_event = 1_566_957_600_000
    state = {"i": 0}
    lat: list[float] = []

    def step():
        i = state["i"]
        t_in = time.perf_counter()
        K.gen_events(k, ts, vals, seed=11, stream_id=0, idx0=i * batch, nkeys=keys,
                     ts_base=t0_event + i * step_ms, ts_span=step_ms, disorder=disorder,
                     val_lo=0, val_span=1, zipf=zipf)
        V.gen_vectors(vec, seed=11, stream_id=0, idx0=i * batch, lo=0.0, span=100.0)
        fired = op.process(k, ts, vec)
        n = sum(len(r.keys) for r in fired)
        if fired:
            lat.append((time.perf_counter() - t_in) * 1e3)
        state["i"] = i + 1
        return n

    for _ in range(warmup):
        step()
    _sync(dev)
    lat.clear()
    t0 = time.perf_counter()
    alerts = 0
    for _ in range(steps):
        alerts += step()
    _sync(dev)
    dt = time.perf_counter() - t0
    return {"config": 6, "metric": "events/sec (vector-metric tumbling window avg, MFMA reduce)",
            "value": batch * steps / dt, "unit": "events/s", "ms_per_step": dt / steps * 1e3,
            "metric_values_per_sec": batch * steps * dim / dt,
            "p50_alert_latency_ms": statistics.median(lat) if lat else None,
            "p99_alert_latency_ms": (sorted(lat)[min(len(lat) - 1, int(0.99 * len(lat)))]
                                     if lat else None),
            "firings_measured": len(lat),
            "alerts": alerts,
            "keys": keys, "dim": dim, "events_per_step": batch, "mode": "mfma" if mfma else "valu",
            "key_distribution": f"zipf({zipf:g})" if zipf > 0 else "uniform",
            "state_bytes": op.state_bytes(), "device": str(dev)}


def config8(steps: int, warmup: int, batch: int = 1 << 22, keys: int = 100_000,
            device: str = "cuda", quantiles=None, distinct: bool = False) -> dict:
    """Process-window median at scale (ComputeCpuMiddle.java:34-48 shape): per host, the median
    CPU usage of every 1-min tumbling event-time window over `keys` hosts; every element is kept
    (ListState analogue, runtime/list_window_operator.py) and each firing sorts the window's
    values by host (one radix sort over the host-id bits) and selects each host's median
    (segment_median_select: LDS bitonic sort / radix select per segment).
    quantiles (e.g. [0.5, 0.95, 0.99]): the same window with WindowQuantiles' function instead
    of the median -- Q nearest-rank quantiles per host from one firing.
    distinct: the same window with WindowDistinctCount's function -- per host, the number of
    different values (the generator draws them from 10,000 possibilities) from one firing."""
    from ..runtime.list_window_operator import KeyedListWindowOperator

    dev = torch.device(device)
    step_ms, disorder = 5_000, 1_000
    if quantiles and distinct:
        raise ValueError("config 8: --quantiles and --distinct exclude each other")
    if distinct:
        op = KeyedListWindowOperator(size=60_000, device=dev, func="distinct")
    elif quantiles:
        from ..api.aggregations import WindowQuantiles

        ppm = WindowQuantiles(1, quantiles).ppm
        op = KeyedListWindowOperator(size=60_000, device=dev, func=("quantiles", ppm))
    else:
        op = KeyedListWindowOperator(size=60_000, device=dev)
    kt = torch.empty(batch, dtype=torch.int64, device=dev)
    tt = torch.empty_like(kt)
    vt = torch.empty_like(kt)
    t0_event = 1_566_957_600_000
    state = {"i": 0}
    lat: list[float] = []

    def step():
        i = state["i"]
        t_in = time.perf_counter()
        K.gen_events(kt, tt, vt, seed=8, stream_id=0, idx0=i * batch, nkeys=keys,
                     ts_base=t0_event + i * step_ms, ts_span=step_ms, disorder=disorder,
                     val_lo=0, val_span=10_000, val_f64=True)
        fired = op.process(kt, tt, vt)
        wm = t0_event + (i + 1) * step_ms - disorder - 1
        fired += op.advance_watermark(wm)
        n = sum(len(r[2]) for r in fired)
        if fired:
            lat.append((time.perf_counter() - t_in) * 1e3)
        state["i"] = i + 1
        return n

    for _ in range(warmup):
        step()
    _sync(dev)
    lat.clear()
    t0 = time.perf_counter()
    rows = 0
    for _ in range(steps):
        rows += step()
    _sync(dev)
    dt = time.perf_counter() - t0
    res = {"config": 8, "metric": "events/sec (process-window median per key, ListState)",
           "value": batch * steps / dt, "unit": "events/s", "ms_per_step": dt / steps * 1e3,
           "p50_fire_step_ms": statistics.median(lat) if lat else None, "medians": rows,
           "keys": keys, "events_per_step": batch, "window_values": batch * 12,
           "device": str(dev)}
    if quantiles:
        res["metric"] = f"events/sec (process-window {len(ppm)} quantiles per key, ListState)"
        res["quantiles_ppm"] = list(ppm)
    if distinct:
        res["metric"] = "events/sec (process-window distinct count per key, ListState)"
    return res


def config13(steps: int, warmup: int, batch: int | None = None, keys: int = 100_000,
             size: int = 1_000, slide: int | None = None, zipf: float = 0.0,
             device: str = "cuda") -> dict:
    """Keyed window join at scale: two device-generated streams (two stream ids of gen_events)
    of `batch` events per side and step feed KeyedJoinWindowOperator directly; every firing
    matches the sides' key segments, scans the pair counts and expands every pair into three
    int64 columns on the device (24 B per pair, nothing copied to the host).

    Defaults: 100,000 keys, 2**21 events per side and 1 s step, tumbling 1 s windows -- a firing
    holds about 21 events per key and side, so about 100,000 x 21 x 21 = 4.4e7 pairs. With
    `zipf` > 0 a few keys take most of the events (exponent 1.2: key 0 is the hottest), and a
    key's pair count grows with the square of its share: the default batch is then 2**15 per side
    and step, which gives a firing of the same order (about 3.6e7 pairs, most of them of the
    hottest keys).
    Also timed in the same call: a device fill of one firing's output bytes."""
    from ..runtime.join_window_operator import KeyedJoinWindowOperator

    dev = torch.device(device)
    if batch is None:
        batch = (1 << 15) if zipf > 0 else (1 << 21)
    step_ms, disorder = 1_000, 200
    op = KeyedJoinWindowOperator(size=size, slide=slide, device=dev)
    cols = [[torch.empty(batch, dtype=torch.int64, device=dev) for _ in range(3)] for _ in (0, 1)]
    t0_event = 1_566_957_600_000
    state = {"i": 0}
    lat: list[float] = []
    firings = {"n": 0, "pairs": 0}

    def step():
        i = state["i"]
        t_in = time.perf_counter()
        for sd, (kt, tt, vt) in enumerate(cols):
            K.gen_events(kt, tt, vt, seed=13, stream_id=sd, idx0=i * batch, nkeys=keys,
                         ts_base=t0_event + i * step_ms, ts_span=step_ms, disorder=disorder,
                         val_lo=0, val_span=10_000, val_f64=True, zipf=zipf)
            op.process(sd, kt, tt, vt)
        fired = op.advance_watermark(t0_event + (i + 1) * step_ms - disorder - 1)
        n = sum(int(r[2].numel()) for r in fired)
        if fired:
            _sync(dev)  # the expand of this step, not the next step's first readback, ends it
            lat.append((time.perf_counter() - t_in) * 1e3)
            firings["n"] += len({r[0] for r in fired})
            firings["pairs"] += n
        state["i"] = i + 1
        return n

    for _ in range(warmup):
        step()
    _sync(dev)
    lat.clear()
    firings.update(n=0, pairs=0)
    t0 = time.perf_counter()
    pairs = 0
    for _ in range(steps):
        pairs += step()
    _sync(dev)
    dt = time.perf_counter() - t0
    per_firing = firings["pairs"] // max(1, firings["n"])
    res = {"config": 13, "metric": "events/sec (keyed window join, both sides)",
           "value": 2 * batch * steps / dt, "unit": "events/s", "pairs_per_s": pairs / dt,
           "ms_per_step": dt / steps * 1e3,
           "p50_fire_step_ms": statistics.median(lat) if lat else None,
           "pairs": pairs, "firings": firings["n"], "pairs_per_firing": per_firing,
           "expand_bytes": 24 * pairs, "late_dropped": op.metrics.num_late_records_dropped,
           "keys": keys, "events_per_side_and_step": batch, "size_ms": size,
           "slide_ms": slide or size, "zipf": zipf, "device": str(dev)}
    if per_firing:
        # The same number of bytes written by a plain device fill (the streaming-store yardstick).
        buf = torch.empty(3 * per_firing, dtype=torch.int64, device=dev)
        buf.fill_(1)
        _sync(dev)
        t1 = time.perf_counter()
        for _ in range(5):
            buf.fill_(2)
        _sync(dev)
        fill_ms = (time.perf_counter() - t1) / 5 * 1e3
        res["fill_ms_per_firing_bytes"] = fill_ms
        res["fill_GBps"] = 24 * per_firing / fill_ms / 1e6
    return res


def config14(steps: int, warmup: int, batch: int | None = None, keys: int = 100_000,
             lo: int = -500, hi: int = 500, zipf: float = 0.0, device: str = "cuda") -> dict:
    """Keyed interval join at scale: two device-generated streams (two stream ids of gen_events)
    of `batch` events per side and 1 s step feed KeyedIntervalJoinOperator directly; every batch
    is sorted, probes the other side's buffer, scans the range lengths, expands every pair into
    four int64 columns on the device (32 B per pair, nothing copied to the host) and is merged
    into its own side's buffer; the watermark follows the steps and cleans the buffers.

    Defaults: 100,000 keys, 2**21 events per side and step -- about 21 events per key, side and
    second -- and bounds (-500, 500) ms: an element meets the other side's elements of one
    second, so a step yields about 2**21 x 21 = 4.4e7 pairs, config 13's firing. With `zipf` > 0
    the default batch is 2**15 per side and step, as in config 13.
    Also timed in the same call: a device fill of one step's output bytes."""
    from ..runtime.interval_join_operator import KeyedIntervalJoinOperator

    dev = torch.device(device)
    if batch is None:
        batch = (1 << 15) if zipf > 0 else (1 << 21)
    step_ms, disorder = 1_000, 200
    op = KeyedIntervalJoinOperator(lo=lo, hi=hi, device=dev)
    cols = [[torch.empty(batch, dtype=torch.int64, device=dev) for _ in range(3)] for _ in (0, 1)]
    t0_event = 1_566_957_600_000
    state = {"i": 0}
    lat: list[float] = []

    def step():
        i = state["i"]
        t_in = time.perf_counter()
        n = 0
        for sd, (kt, tt, vt) in enumerate(cols):
            K.gen_events(kt, tt, vt, seed=14, stream_id=sd, idx0=i * batch, nkeys=keys,
                         ts_base=t0_event + i * step_ms, ts_span=step_ms, disorder=disorder,
                         val_lo=0, val_span=10_000, val_f64=True, zipf=zipf)
            n += sum(int(ch[0].numel()) for ch in op.process(sd, kt, tt, vt))
        op.advance_watermark(t0_event + (i + 1) * step_ms - disorder - 1)
        _sync(dev)
        lat.append((time.perf_counter() - t_in) * 1e3)
        state["i"] = i + 1
        return n

    for _ in range(warmup):
        step()
    _sync(dev)
    lat.clear()
    t0 = time.perf_counter()
    pairs = 0
    for _ in range(steps):
        pairs += step()
    _sync(dev)
    dt = time.perf_counter() - t0
    per_step = pairs // max(1, steps)
    res = {"config": 14, "metric": "events/sec (keyed interval join, both sides)",
           "value": 2 * batch * steps / dt, "unit": "events/s", "pairs_per_s": pairs / dt,
           "ms_per_step": dt / steps * 1e3, "p50_step_ms": statistics.median(lat) if lat else None,
           "pairs": pairs, "pairs_per_step": per_step, "expand_bytes": 32 * pairs,
           "buffered_rows": list(op.n), "late_dropped": op.metrics.num_late_records_dropped,
           "keys": keys, "events_per_side_and_step": batch, "lo_ms": lo, "hi_ms": hi,
           "zipf": zipf, "device": str(dev)}
    if per_step:
        # The same number of bytes written by a plain device fill (the streaming-store yardstick).
        buf = torch.empty(4 * per_step, dtype=torch.int64, device=dev)
        buf.fill_(1)
        _sync(dev)
        t1 = time.perf_counter()
        for _ in range(5):
            buf.fill_(2)
        _sync(dev)
        fill_ms = (time.perf_counter() - t1) / 5 * 1e3
        res["fill_ms_per_step_bytes"] = fill_ms
        res["fill_GBps"] = 32 * per_step / fill_ms / 1e6
    return res


def _spread(xs: list) -> dict:
    """Median, extremes and the 10th / 90th percentile of repeated step times (ms)."""
    a = np.sort(np.asarray(xs, dtype=np.float64))
    return {"median": float(np.median(a)), "min": float(a[0]), "max": float(a[-1]),
            "p10": float(a[int(0.1 * (a.size - 1))]), "p90": float(a[int(round(0.9 * (a.size - 1)))])}


def config15(steps: int, warmup: int, batch: int | None = None, keys: int = 1_000_000,
             when: str | None = ">", zipf: float = 0.0, rules: int = 1 << 12,
             device: str = "cuda") -> dict:
    """Keyed latest-value lookup at scale (``samples.connect(rules).key_by(..).process(
    LookupLatest(..))``): `batch` device-generated samples per step (gen_events, values uniform
    in [0, 10000)) probe the per-key thresholds of KeyedLookupOperator, fed directly; a rule
    stream of `rules` updates per step moves thresholds while the job runs. Every key has a
    threshold before the first step and thresholds are uniform in [9800, 10000), so about 1 % of
    the samples alert and leave the device as four int64 columns. ``when=None`` keeps every
    sample (default 0.0): the gather-only path.

    Timed per step, each behind a device synchronise, alternating in the same call: the native
    step (upsert + probe) and a yardstick that is not the code under test, the torch
    composition ``table[keys]``, compare, ``nonzero``, four index gathers. The sample generation
    is outside both windows."""
    from ..runtime.lookup_operator import KeyedLookupOperator

    dev = torch.device(device)
    batch = batch or (1 << 21)
    default_bits = None if when is not None else 0
    op = KeyedLookupOperator(when, default_bits, dev)
    step_ms = 1_000
    t0_event = 1_566_957_600_000
    # every key's first threshold
    ids = torch.arange(keys, dtype=torch.int64, device=dev)
    first = torch.empty(keys, dtype=torch.int64, device=dev)
    scratch = torch.empty(keys, dtype=torch.int64, device=dev)
    K.gen_events(scratch, torch.empty_like(scratch), first, seed=15, stream_id=2, idx0=0,
                 nkeys=keys, ts_base=t0_event, ts_span=1, disorder=0, val_lo=9_800, val_span=200,
                 val_f64=True)
    op.upsert(ids, first)
    del ids, first, scratch
    sk, st, sv = (torch.empty(batch, dtype=torch.int64, device=dev) for _ in range(3))
    rk, rt, rv = (torch.empty(rules, dtype=torch.int64, device=dev) for _ in range(3))
    state = {"i": 0}
    native_ms: list[float] = []
    torch_ms: list[float] = []
    cmp = {None: None, ">": torch.gt, ">=": torch.ge, "<": torch.lt, "<=": torch.le,
           "==": torch.eq, "!=": torch.ne}[when]

    def yardstick():
        rows = op.table[sk]                       # a key at or beyond cap has no rule: none here
        t = rows[:, 0].view(torch.float64)
        mask = rows[:, 1] != 0
        if cmp is not None:
            mask &= cmp(sv.view(torch.float64), t)
        idx = mask.nonzero().squeeze(1)
        return sk[idx], sv[idx], rows[:, 0][idx], st[idx]

    def step():
        i = state["i"]
        K.gen_events(sk, st, sv, seed=15, stream_id=0, idx0=i * batch, nkeys=keys,
                     ts_base=t0_event + i * step_ms, ts_span=step_ms, disorder=0, val_lo=0,
                     val_span=10_000, val_f64=True, zipf=zipf)
        K.gen_events(rk, rt, rv, seed=15, stream_id=1, idx0=i * rules, nkeys=keys,
                     ts_base=t0_event + i * step_ms, ts_span=step_ms, disorder=0, val_lo=9_800,
                     val_span=200, val_f64=True)
        _sync(dev)
        t_in = time.perf_counter()
        op.process(1, rk, rt, rv)
        out = op.process(0, sk, st, sv)
        _sync(dev)
        native_ms.append((time.perf_counter() - t_in) * 1e3)
        kept = int(out[0][0].numel()) if out else 0
        t_in = time.perf_counter()
        ref = yardstick()
        _sync(dev)
        torch_ms.append((time.perf_counter() - t_in) * 1e3)
        if int(ref[0].numel()) != kept or (out and not all(
                torch.equal(a, b) for a, b in zip(out[0], ref))):
            raise RuntimeError("config 15: the native probe and the torch composition differ")
        state["i"] = i + 1
        return kept

    for _ in range(warmup):
        step()
    native_ms.clear()
    torch_ms.clear()
    kept = 0
    for _ in range(steps):
        kept += step()
    nat, ref = _spread(native_ms), _spread(torch_ms)
    return {"config": 15, "metric": "events/sec (keyed latest-value lookup, samples probed)",
            "value": batch / nat["median"] * 1e3, "unit": "events/s",
            "ms_per_step": nat["median"], "native_ms": nat, "torch_ms": ref,
            "torch_events_per_s": batch / ref["median"] * 1e3,
            "native_over_torch_time": nat["median"] / ref["median"],
            "kept_rows": kept, "kept_per_step": kept // max(1, steps),
            "kept_share": kept / max(1, steps * batch), "when": when, "keys": keys,
            "samples_per_step": batch, "rules_per_step": rules, "zipf": zipf,
            "table_rows": op.cap, "steps": steps, "device": str(dev)}


def config20(steps: int, warmup: int, batch: int | None = None, keys: int = 1_000_000,
             rules: int = 8, dense: bool = False, device: str = "cuda") -> dict:
    """Broadcast rule set at scale (``samples.key_by(0).connect(rules.broadcast(..)).process(
    RuleSetAlert(..))``): config 15's samples (`batch` device-generated samples per step, values
    uniform in [0, 10000)) are tested against `rules` rules of RuleSetOperator, fed directly. Rule
    r is ``> 9900 + 10 r``: about 5 % rows per sample at 8 rules; two rules move every step, as a
    rule stream would move them while the job runs. With `dense` rule r is ``> -1 - r``: every
    sample breaks every rule, the expansion-bound case. The rows leave the device operator as
    five int64 columns.

    Timed per step, each behind a device synchronise, alternating in the same call: the native
    step (rule update + probe) and a yardstick that is not the code under test, the torch
    composition: an ``n x R`` compare, ``nonzero`` (row-major: sample order, then rule id), five
    index gathers. The sample generation is outside both windows."""
    from ..runtime.ruleset_operator import RuleSetOperator

    if not 1 <= rules <= K.RULESET_MAX:
        raise ValueError(f"config 20: 1 .. {K.RULESET_MAX} rules")
    dev = torch.device(device)
    batch = batch or (1 << 21)
    op = RuleSetOperator(dev)
    step_ms = 1_000
    t0_event = 1_566_957_600_000
    gt = K.LOOKUP_WHENS[">"]

    def threshold(r: int, i: int) -> float:
        moved = float((i + r) % 5)           # a rule that moves takes one of five values
        return -1.0 - r - moved if dense else 9_900.0 + 10 * r + moved

    def bits_of(xs) -> np.ndarray:
        return np.asarray(xs, dtype=np.float64).view(np.int64)

    current = [threshold(r, 0) for r in range(rules)]
    op.update(np.arange(rules), np.full(rules, gt), bits_of(current))
    ids = torch.arange(rules, dtype=torch.int64, device=dev)
    sk, st, sv = (torch.empty(batch, dtype=torch.int64, device=dev) for _ in range(3))
    state = {"i": 0}
    native_ms: list[float] = []
    torch_ms: list[float] = []

    def yardstick():
        thr_bits = torch.from_numpy(bits_of(current)).to(dev)
        mask = sv.view(torch.float64)[:, None] > thr_bits.view(torch.float64)[None, :]
        idx = mask.nonzero()
        s, r = idx[:, 0], idx[:, 1]
        return sk[s], sv[s], ids[r], thr_bits[r], st[s]

    def step():
        i = state["i"]
        K.gen_events(sk, st, sv, seed=20, stream_id=0, idx0=i * batch, nkeys=keys,
                     ts_base=t0_event + i * step_ms, ts_span=step_ms, disorder=0, val_lo=0,
                     val_span=10_000, val_f64=True)
        moving = sorted({i % rules, (i + 1) % rules})
        for r in moving:
            current[r] = threshold(r, i + 1)
        _sync(dev)
        t_in = time.perf_counter()
        op.process(1, np.asarray(moving), np.full(len(moving), gt),
                   bits_of([current[r] for r in moving]))
        out = op.process(0, sk, st, sv)
        _sync(dev)
        native_ms.append((time.perf_counter() - t_in) * 1e3)
        rows = sum(int(o[0].numel()) for o in out)
        t_in = time.perf_counter()
        ref = yardstick()
        _sync(dev)
        torch_ms.append((time.perf_counter() - t_in) * 1e3)
        got = [torch.cat([o[c] for o in out]) for c in range(5)] if out else None
        if int(ref[0].numel()) != rows or (out and not all(
                torch.equal(a, b) for a, b in zip(got, ref))):
            raise RuntimeError("config 20: the native probe and the torch composition differ")
        state["i"] = i + 1
        return rows

    for _ in range(warmup):
        step()
    native_ms.clear()
    torch_ms.clear()
    rows = 0
    for _ in range(steps):
        rows += step()
    nat, ref = _spread(native_ms), _spread(torch_ms)
    return {"config": 20, "metric": "events/sec (broadcast rule set, samples probed)",
            "value": batch / nat["median"] * 1e3, "unit": "events/s",
            "ms_per_step": nat["median"], "native_ms": nat, "torch_ms": ref,
            "torch_events_per_s": batch / ref["median"] * 1e3,
            "native_over_torch_time": nat["median"] / ref["median"],
            "rows": rows, "rows_per_step": rows // max(1, steps),
            "rows_per_sample": rows / max(1, steps * batch), "rules": rules, "dense": dense,
            "samples_per_step": batch, "steps": steps, "device": str(dev)}


def config16(steps: int, warmup: int, batch: int | None = None, keys: int = 1_000_000,
             timeout_ms: int = 3_000, zipf: float = 0.0, device: str = "cuda") -> dict:
    """Keyed event-time timers at scale (``samples.key_by(0).process(CountWithTimeout(..))``):
    `batch` device-generated samples per 1 s step (gen_events, uniform or zipf keys) feed
    KeyedTimeoutOperator directly, and every step ends with a watermark at the step's end, which
    fires the keys that have been silent for `timeout_ms`. The rows leave the device as four int64
    columns (key id, count, last, deadline) ordered by (deadline, key id).

    Timed per step, each behind a device synchronise, alternating in the same call: the native
    step (update + firing) and a yardstick that is not the code under test, the torch
    composition ``scatter_reduce(amax)`` of the arrival index (the key's last row), ``bincount``
    (the counts), a compare and ``nonzero`` (the firing), gathers and a stable sort by deadline
    (the output). Both must give the same rows every step. The sample generation is outside both
    windows."""
    from ..runtime.timeout_operator import KeyedTimeoutOperator

    dev = torch.device(device)
    batch = batch or (1 << 21)
    op = KeyedTimeoutOperator(timeout_ms, device=dev, dense_limit=max(keys, 1 << 26),
                              capacity=keys)
    step_ms = 1_000
    t0_event = 1_566_957_600_000
    none = K.TIMEOUT_NONE
    sk, st, sv = (torch.empty(batch, dtype=torch.int64, device=dev) for _ in range(3))
    arrival = torch.arange(batch, dtype=torch.int64, device=dev)
    y_count = torch.zeros(keys, dtype=torch.int64, device=dev)
    y_last = torch.zeros(keys, dtype=torch.int64, device=dev)
    y_dead = torch.full((keys,), none, dtype=torch.int64, device=dev)
    state = {"i": 0}
    native_ms: list[float] = []
    torch_ms: list[float] = []

    def yardstick(wm: int):
        nonlocal y_last, y_dead
        last_row = torch.full((keys,), -1, dtype=torch.int64, device=dev)
        last_row.scatter_reduce_(0, sk, arrival, reduce="amax")
        seen = last_row >= 0
        y_count.add_(torch.bincount(sk, minlength=keys))
        y_last = torch.where(seen, st[last_row.clamp_(min=0)], y_last)
        y_dead = torch.where(seen, y_last + timeout_ms, y_dead)
        ids = ((y_dead != none) & (y_dead <= wm)).nonzero().squeeze(1)
        dl = y_dead[ids]
        y_dead[ids] = none
        order = torch.sort(dl, stable=True).indices   # ties stay in key order
        ids = ids[order]
        return ids, y_count[ids], y_last[ids], dl[order]

    def step():
        i = state["i"]
        K.gen_events(sk, st, sv, seed=16, stream_id=0, idx0=i * batch, nkeys=keys,
                     ts_base=t0_event + i * step_ms, ts_span=step_ms, disorder=0, val_lo=0,
                     val_span=100, zipf=zipf)
        wm = t0_event + (i + 1) * step_ms
        _sync(dev)
        t_in = time.perf_counter()
        op.process(sk, st)
        out = op.advance_watermark(wm)
        _sync(dev)
        native_ms.append((time.perf_counter() - t_in) * 1e3)
        fired = int(out[0][0].numel()) if out else 0
        t_in = time.perf_counter()
        ref = yardstick(wm)
        _sync(dev)
        torch_ms.append((time.perf_counter() - t_in) * 1e3)
        if int(ref[0].numel()) != fired or (out and not all(
                torch.equal(a, b) for a, b in zip(out[0], ref))):
            raise RuntimeError("config 16: the native firing and the torch composition differ")
        state["i"] = i + 1
        return fired

    for _ in range(warmup):
        step()
    native_ms.clear()
    torch_ms.clear()
    fired = 0
    for _ in range(steps):
        fired += step()
    nat, ref = _spread(native_ms), _spread(torch_ms)
    return {"config": 16, "metric": "events/sec (keyed timers: count, last seen, timeout firing)",
            "value": batch / nat["median"] * 1e3, "unit": "events/s",
            "ms_per_step": nat["median"], "native_ms": nat, "torch_ms": ref,
            "torch_events_per_s": batch / ref["median"] * 1e3,
            "native_over_torch_time": nat["median"] / ref["median"],
            "fired_rows": fired, "fired_per_step": fired // max(1, steps),
            "fired_share": fired / max(1, steps * keys), "timeout_ms": timeout_ms, "keys": keys,
            "samples_per_step": batch, "zipf": zipf, "table_rows": op.cap,
            "tiles": int(op.tile_min.numel()),
            "tileskip": os.environ.get("MXS_TIMEOUT_TILESKIP", "1") != "0",
            "steps": steps, "warmup": warmup, "device": str(dev)}


def config17(steps: int, warmup: int, batch: int | None = None, keys: int = 1_000_000,
             for_ms: int = 3_000, zipf: float = 0.0, device: str = "cuda") -> dict:
    """Sustained-condition alerts at scale (``samples.key_by(0).process(SustainedAlert(2, ">",
    90, for_))``): `batch` device-generated samples per 1 s step (gen_events, uniform or zipf
    keys) feed KeyedSustainOperator directly. A key breaches for 10 consecutive steps out of
    every 1000, at a phase of its own, so about 1 % of the keys are in a breaching run at any
    time and runs start and end at every step; their values lie in 91..99, all others in 0..89.
    The transitions leave the device as five int64 columns (key id, code, since, value, ts) in
    arrival order.

    Timed per step, each behind a device synchronise, alternating in the same call: the native
    step and a yardstick that is not the code under test, the torch composition of the same
    result -- a stable sort by key, ``cummax`` of the stretch starts and (stretch id, timestamp)
    for the run starts and their largest timestamp so far, gathers of the keys' carried state,
    compares, ``nonzero`` and a sort of the kept rows by arrival. Both must give the same rows
    every step, and the same table at the end. The sample generation is outside both windows."""
    from ..runtime.sustain_operator import KeyedSustainOperator

    dev = torch.device(device)
    batch = batch or (1 << 21)
    thr = 90
    op = KeyedSustainOperator(">", thr, for_ms, device=dev, dense_limit=max(keys, 1 << 26),
                              capacity=keys)
    step_ms = 1_000
    t0_event = 1_566_957_600_000
    none = K.SUSTAIN_NONE
    shift = 1 << 11  # > the timestamps' span within a step
    sk, st, sv = (torch.empty(batch, dtype=torch.int64, device=dev) for _ in range(3))
    pos = torch.arange(batch, dtype=torch.int64, device=dev)
    y_state = K.sustain_table(keys, dev)
    state = {"i": 0}
    native_ms: list[float] = []
    torch_ms: list[float] = []

    def shifted(x, fill):
        out = torch.empty_like(x)
        out[0] = fill
        out[1:] = x[:-1]
        return out

    def yardstick():
        order = torch.sort(sk, stable=True).indices
        k, t, v = sk[order], st[order], sv[order]
        b = v.to(torch.float64) > float(thr)
        head = shifted(k, -1) != k
        tail = torch.ones_like(head)
        tail[:-1] = head[1:]
        cs, cf = y_state[k, 0], y_state[k, 1] != 0   # the key's state before the batch
        # a stretch starts at its key's first row and behind every non-breach
        start = head | ~shifted(b, False)
        sidx = torch.cummax(torch.where(start, pos, 0), 0).values
        carried = head[sidx] & (cs != none)
        since = torch.where(carried, cs, t[sidx])
        sid = torch.cumsum(start, 0) * shift
        tmin = t.min()
        tmax = torch.cummax(sid + (t - tmin), 0).values - sid + tmin
        fin = b & ((carried & cf) | (tmax - since >= for_ms))
        fbefore = torch.where(head, cf, shifted(fin, False))
        sbefore = torch.where(head, cs, shifted(since, 0))
        fire = fin & ~fbefore
        idx = (fire | (~b & fbefore)).nonzero().squeeze(1)
        by_arrival = torch.sort(order[idx]).indices
        idx = idx[by_arrival]
        code = fire[idx]
        rows = (k[idx], code.to(torch.int64), torch.where(code, since[idx], sbefore[idx]), v[idx],
                t[idx])
        kt = k[tail]
        y_state[kt, 0] = torch.where(b[tail], since[tail], none)
        y_state[kt, 1] = fin[tail].to(torch.int64)
        return rows

    def step():
        i = state["i"]
        K.gen_events(sk, st, sv, seed=17, stream_id=0, idx0=i * batch, nkeys=keys,
                     ts_base=t0_event + i * step_ms, ts_span=step_ms, disorder=0, val_lo=0,
                     val_span=100, zipf=zipf)
        breach = (sk * 2_654_435_761 + i) % 1_000 < 10
        sv.copy_(torch.where(breach, 91 + sv % 9, sv % 90))
        _sync(dev)
        t_in = time.perf_counter()
        out = op.process(sk, sv, st, is_float=False)
        _sync(dev)
        native_ms.append((time.perf_counter() - t_in) * 1e3)
        rows = int(out[0][0].numel()) if out else 0
        t_in = time.perf_counter()
        ref = yardstick()
        _sync(dev)
        torch_ms.append((time.perf_counter() - t_in) * 1e3)
        if int(ref[0].numel()) != rows or (out and not all(
                torch.equal(a, b) for a, b in zip(out[0], ref))):
            raise RuntimeError("config 17: the native rows and the torch composition differ")
        state["i"] = i + 1
        return rows, int(ref[1].sum()) if rows else 0

    for _ in range(warmup):
        step()
    native_ms.clear()
    torch_ms.clear()
    rows = fired = 0
    for _ in range(steps):
        r, f = step()
        rows, fired = rows + r, fired + f
    if not torch.equal(op.state[:keys], y_state):
        raise RuntimeError("config 17: the native table and the torch composition differ")
    open_runs = int((y_state[:, 0] != none).sum())
    nat, ref = _spread(native_ms), _spread(torch_ms)
    return {"config": 17, "metric": "events/sec (sustained-condition alerts: per-key scan)",
            "value": batch / nat["median"] * 1e3, "unit": "events/s",
            "ms_per_step": nat["median"], "native_ms": nat, "torch_ms": ref,
            "torch_events_per_s": batch / ref["median"] * 1e3,
            "native_over_torch_time": nat["median"] / ref["median"],
            "rows": rows, "rows_per_step": rows // max(1, steps),
            "fired_per_step": fired // max(1, steps),
            "resolved_per_step": (rows - fired) // max(1, steps),
            "open_runs_share": open_runs / keys, "firing_keys": int(y_state[:, 1].sum()),
            "for_ms": for_ms, "keys": keys, "samples_per_step": batch, "zipf": zipf,
            "table_rows": op.cap, "steps": steps, "warmup": warmup, "device": str(dev)}


def config18(steps: int, warmup: int, batch: int | None = None, keys: int = 1_000_000,
             times: int = 5, within_ms: int = 3_000, zipf: float = 0.0,
             device: str = "cuda") -> dict:
    """Burst alerts at scale (``samples.key_by(0).process(BurstAlert(2, ">", 90, times,
    within))``) on config 17's data: `batch` device-generated samples per 1 s step (gen_events,
    uniform or zipf keys) feed KeyedBurstOperator directly; a key breaches for 10 consecutive
    steps out of every 1000, at a phase of its own. The transitions leave the device as five
    int64 columns (key id, code, since, value, ts) in arrival order.

    Timed per step, each behind a device synchronise, alternating in the same call on the same
    batch: the burst step and config 17's native step (KeyedSustainOperator, ``for_`` =
    `within`), which does strictly less per row -- no ring, no look-back. The ratio is reported,
    not gated. Outside both windows the C++ twin runs every step on host copies: the first three
    steps' rows and the final ring and rows must equal the device's. The sample generation is
    outside the windows too."""
    from ..runtime.burst_operator import KeyedBurstOperator, unpack
    from ..runtime.sustain_operator import KeyedSustainOperator, threshold_bits

    dev = torch.device(device)
    batch = batch or (1 << 21)
    thr = 90
    op = KeyedBurstOperator(">", thr, times, within_ms, device=dev,
                            dense_limit=max(keys, 1 << 26), capacity=keys)
    sustain = KeyedSustainOperator(">", thr, within_ms, device=dev,
                                   dense_limit=max(keys, 1 << 26), capacity=keys)
    twin = K.burst_table(keys, times, "cpu")
    step_ms = 1_000
    t0_event = 1_566_957_600_000
    sk, st, sv = (torch.empty(batch, dtype=torch.int64, device=dev) for _ in range(3))
    state = {"i": 0}
    burst_ms: list[float] = []
    sustain_ms: list[float] = []

    def step():
        i = state["i"]
        K.gen_events(sk, st, sv, seed=17, stream_id=0, idx0=i * batch, nkeys=keys,
                     ts_base=t0_event + i * step_ms, ts_span=step_ms, disorder=0, val_lo=0,
                     val_span=100, zipf=zipf)
        breach = (sk * 2_654_435_761 + i) % 1_000 < 10
        sv.copy_(torch.where(breach, 91 + sv % 9, sv % 90))
        _sync(dev)
        t_in = time.perf_counter()
        out = op.process(sk, sv, st, is_float=False)
        _sync(dev)
        burst_ms.append((time.perf_counter() - t_in) * 1e3)
        t_in = time.perf_counter()
        ref = sustain.process(sk, sv, st, is_float=False)
        _sync(dev)
        sustain_ms.append((time.perf_counter() - t_in) * 1e3)
        want = K.burst_update(twin[0], twin[1], sk.cpu(), sv.cpu(), st.cpu(), kind=K.SUSTAIN_LONG,
                              when=">", threshold_bits=threshold_bits(thr), within=within_ms)
        rows = int(out[0][0].numel()) if out else 0
        if rows != int(want[0].numel()) or (i < 3 and out and not all(
                torch.equal(a.cpu(), b) for a, b in zip(out[0], want))):
            raise RuntimeError("config 18: the native rows and the twin's differ")
        state["i"] = i + 1
        fired = int(out[0][1].sum()) if out else 0
        return rows, fired, int(ref[0][0].numel()) if ref else 0

    for _ in range(warmup):
        step()
    burst_ms.clear()
    sustain_ms.clear()
    rows = fired = sustain_rows = 0
    for _ in range(steps):
        r, f, s = step()
        rows, fired, sustain_rows = rows + r, fired + f, sustain_rows + s
    if not torch.equal(op.row[:keys].cpu(), twin[1]) or not all(
            np.array_equal(a, b) for a, b in zip(unpack(op.ring[:keys], op.row[:keys]),
                                                 unpack(*twin))):
        raise RuntimeError("config 18: the native state and the twin's differ")
    held = (twin[1][:, 1] >> K.BURST_HELD_SHIFT) & 0x7f
    nat, ref = _spread(burst_ms), _spread(sustain_ms)
    return {"config": 18, "metric": "events/sec (burst alerts: per-key look-back and scan)",
            "value": batch / nat["median"] * 1e3, "unit": "events/s",
            "ms_per_step": nat["median"], "native_ms": nat, "sustain_ms": ref,
            "sustain_events_per_s": batch / ref["median"] * 1e3,
            "burst_over_sustain_time": nat["median"] / ref["median"],
            "rows": rows, "rows_per_step": rows // max(1, steps),
            "fired_per_step": fired // max(1, steps),
            "resolved_per_step": (rows - fired) // max(1, steps),
            "sustain_rows_per_step": sustain_rows // max(1, steps),
            "keys_with_breaches": int((held > 0).sum()), "keys_with_full_ring":
            int((held == times).sum()), "firing_keys": int((twin[1][:, 1] & 1).sum()),
            "times": times, "within_ms": within_ms, "keys": keys, "samples_per_step": batch,
            "zipf": zipf, "table_rows": op.cap, "steps": steps, "warmup": warmup,
            "device": str(dev)}


def config19(steps: int, warmup: int, batch: int | None = None, keys: int = 1_000_000,
             for_ms: int = 3_000, disorder_ms: int = 3_000, zipf: float = 0.0,
             device: str = "cuda") -> dict:
    """Event-time order in front of a rule at scale (``samples.key_by(0).process(
    EventTimeOrdered(SustainedAlert(2, ">", 90, for_)))``) on config 17's data, every timestamp
    displaced backwards uniformly within `disorder_ms` (0: the stream is in order). Each 1 s step
    sends the watermark of the step's end minus the disorder, so no row is late and about
    `disorder_ms` / 1 s steps of rows are buffered at any time.

    Timed per step, each behind a device synchronise, alternating in the same call on the same
    batch: the ordered step -- EventOrderBuffer.push, release at the watermark and
    KeyedSustainOperator over the released rows -- and config 17's plain native step, a second
    KeyedSustainOperator over the batch in arrival order. The ratio is reported, not gated.
    Outside both windows the C++ twins (buffer and rule) run every step on host copies: the
    first three steps' rows and the final buffer contents must equal the device's, and every
    step's row count. The sample generation is outside the windows too."""
    from ..runtime.reorder_operator import EventOrderBuffer
    from ..runtime.sustain_operator import KeyedSustainOperator

    dev = torch.device(device)
    batch = batch or (1 << 21)
    thr = 90
    if disorder_ms < 0:
        raise ValueError("config 19: --disorder-ms must be >= 0")
    make = lambda d: KeyedSustainOperator(">", thr, for_ms, device=d,  # noqa: E731
                                          dense_limit=max(keys, 1 << 26), capacity=keys)
    buf, rule, plain = EventOrderBuffer(dev, capacity=4 * batch), make(dev), make(dev)
    tbuf, trule = EventOrderBuffer("cpu", capacity=4 * batch), make("cpu")
    step_ms = 1_000
    t0_event = 1_566_957_600_000
    sk, st, sv = (torch.empty(batch, dtype=torch.int64, device=dev) for _ in range(3))
    state = {"i": 0}
    ordered_ms: list[float] = []
    plain_ms: list[float] = []
    chunks: list[int] = []
    buffered: list[int] = []
    contrib: list[int] = []

    def step():
        i = state["i"]
        K.gen_events(sk, st, sv, seed=17, stream_id=0, idx0=i * batch, nkeys=keys,
                     ts_base=t0_event + i * step_ms, ts_span=step_ms, disorder=disorder_ms,
                     val_lo=0, val_span=100, zipf=zipf)
        breach = (sk * 2_654_435_761 + i) % 1_000 < 10
        sv.copy_(torch.where(breach, 91 + sv % 9, sv % 90))
        wm = t0_event + (i + 1) * step_ms - 1 - disorder_ms
        _sync(dev)
        t_in = time.perf_counter()
        buf.push(sk, st, sv)
        cols = buf.release(wm)
        out = rule.process(cols[0], cols[2], cols[1], is_float=False) if cols is not None else []
        _sync(dev)
        ordered_ms.append((time.perf_counter() - t_in) * 1e3)
        chunks.append(len(buf.chunks))
        buffered.append(buf.rows_buffered)
        contrib.append(buf.last_contrib)
        t_in = time.perf_counter()
        ref = plain.process(sk, sv, st, is_float=False)
        _sync(dev)
        plain_ms.append((time.perf_counter() - t_in) * 1e3)
        tbuf.push(sk.cpu(), st.cpu(), sv.cpu())
        tcols = tbuf.release(wm)
        want = trule.process(tcols[0], tcols[2], tcols[1], is_float=False) \
            if tcols is not None else []
        rows = int(out[0][0].numel()) if out else 0
        if rows != (int(want[0][0].numel()) if want else 0) or (i < 3 and out and not all(
                torch.equal(a.cpu(), b) for a, b in zip(out[0], want[0]))):
            raise RuntimeError("config 19: the native rows and the twins' differ")
        state["i"] = i + 1
        return rows, int(cols[0].numel()) if cols is not None else 0, \
            int(ref[0][0].numel()) if ref else 0

    for _ in range(warmup):
        step()
    for x in (ordered_ms, plain_ms, chunks, buffered, contrib):
        x.clear()
    rows = released = plain_rows = 0
    for _ in range(steps):
        r, n, p = step()
        rows, released, plain_rows = rows + r, released + n, plain_rows + p
    if buf.metrics != tbuf.metrics or not all(
            np.array_equal(a, b) for a, b in zip(buf.rows(), tbuf.rows())):
        raise RuntimeError("config 19: the native buffer and the twin's differ")
    nat, ref = _spread(ordered_ms), _spread(plain_ms)
    return {"config": 19, "metric": "events/sec (event-time order in front of sustained alerts)",
            "value": batch / nat["median"] * 1e3, "unit": "events/s",
            "ms_per_step": nat["median"], "ordered_ms": nat, "plain_ms": ref,
            "plain_events_per_s": batch / ref["median"] * 1e3,
            "ordered_over_plain_time": nat["median"] / ref["median"],
            "rows": rows, "rows_per_step": rows // max(1, steps),
            "plain_rows_per_step": plain_rows // max(1, steps),
            "released_per_step": released // max(1, steps),
            "live_chunks": int(np.median(chunks)) if chunks else 0,
            "buffered_rows": int(np.median(buffered)) if buffered else 0,
            "contributing_chunks": int(np.median(contrib)) if contrib else 0,
            "slice_path_steps": sum(c == 1 for c in contrib),
            "consolidations": buf.consolidations, "arena_rows": buf.cap,
            "late_dropped": buf.metrics.num_late_records_dropped,
            "disorder_ms": disorder_ms, "for_ms": for_ms, "keys": keys,
            "samples_per_step": batch, "zipf": zipf, "steps": steps, "warmup": warmup,
            "device": str(dev)}


def config21(steps: int, warmup: int, batch: int | None = None, keys: int = 1_000_000,
             states: int = 3, zipf: float = 0.0, device: str = "cuda") -> dict:
    """Keyed state machines at scale (``samples.key_by(0).process(StateMachineAlert(2, bounds,
    table))``) on config 17's data: `batch` device-generated samples per 1 s step (gen_events,
    uniform or zipf keys) feed KeyedStateMachineOperator directly; a key breaches for 10
    consecutive steps out of every 1000, at a phase of its own, with values in 91..99, all
    others in 0..89. `states` = 3 is a severity with hysteresis over the bounds (90, 95): ok /
    warning / critical, critical held until the value falls below 90, every change reported;
    any other `states` (2 .. 16) is a saturating counter of breaches in a row over the bound
    90, reported when it saturates and when a saturated key falls back -- 16 is the
    composition-bound case, every function 16 nibbles wide. The rows leave the device as five
    int64 columns (key id, from << 4 | to, since, value, ts) in arrival order.

    Timed per step, each behind a device synchronise, alternating in the same call on the same
    batch: the state-machine step and config 17's native step (KeyedSustainOperator, ``for_`` =
    3 s). Both sort by key, scan, read the count back and sort their rows by arrival; the
    difference is the scan and one more radix digit of the rows' tags. The ratio is reported,
    not gated. Outside both windows the C++ twin runs every step on host copies: every step's
    row count, the first three steps' rows and the final table must equal the device's. The
    sample generation is outside the windows too."""
    from ..runtime.fsm_operator import KeyedStateMachineOperator
    from ..runtime.sustain_operator import KeyedSustainOperator

    dev = torch.device(device)
    batch = batch or (1 << 21)
    if states == 3:
        bounds, table, report = [90, 95], [[0, 1, 2], [0, 1, 2], [0, 2, 2]], "change"
    elif 2 <= states <= 16:
        top = states - 1
        bounds, table = [90], [[0, min(s + 1, top)] for s in range(states)]
        report = [(top - 1, top), (top, 0)]
    else:
        raise ValueError("config 21: --states lies in [2, 16]")
    op = KeyedStateMachineOperator(bounds, table, 0, report, device=dev,
                                   dense_limit=max(keys, 1 << 26), capacity=keys)
    sustain = KeyedSustainOperator(">", 90, 3_000, device=dev, dense_limit=max(keys, 1 << 26),
                                   capacity=keys)
    twin = K.fsm_table(keys, "cpu")
    rule = dict(cuts=op.cuts, cols=op.cols, report=op.masks, states=op.states,
                classes=op.classes, initial=op.initial)
    step_ms = 1_000
    t0_event = 1_566_957_600_000
    sk, st, sv = (torch.empty(batch, dtype=torch.int64, device=dev) for _ in range(3))
    state = {"i": 0}
    fsm_ms: list[float] = []
    sustain_ms: list[float] = []

    def step():
        i = state["i"]
        K.gen_events(sk, st, sv, seed=17, stream_id=0, idx0=i * batch, nkeys=keys,
                     ts_base=t0_event + i * step_ms, ts_span=step_ms, disorder=0, val_lo=0,
                     val_span=100, zipf=zipf)
        breach = (sk * 2_654_435_761 + i) % 1_000 < 10
        sv.copy_(torch.where(breach, 91 + sv % 9, sv % 90))
        _sync(dev)
        t_in = time.perf_counter()
        out = op.process(sk, sv, st, is_float=False)
        _sync(dev)
        fsm_ms.append((time.perf_counter() - t_in) * 1e3)
        t_in = time.perf_counter()
        ref = sustain.process(sk, sv, st, is_float=False)
        _sync(dev)
        sustain_ms.append((time.perf_counter() - t_in) * 1e3)
        want = K.fsm_update(twin, sk.cpu(), sv.cpu(), st.cpu(), kind=K.SUSTAIN_LONG, **rule)
        rows = int(out[0][0].numel()) if out else 0
        if rows != int(want[0].numel()) or (i < 3 and out and not all(
                torch.equal(a.cpu(), b) for a, b in zip(out[0], want))):
            raise RuntimeError("config 21: the native rows and the twin's differ")
        state["i"] = i + 1
        return rows, int(ref[0][0].numel()) if ref else 0

    for _ in range(warmup):
        step()
    fsm_ms.clear()
    sustain_ms.clear()
    rows = sustain_rows = 0
    for _ in range(steps):
        r, s = step()
        rows, sustain_rows = rows + r, sustain_rows + s
    if not torch.equal(op.state[:keys].cpu(), twin):
        raise RuntimeError("config 21: the native table and the twin's differ")
    seen = twin[:, 0] != K.FSM_NONE
    nat, ref = _spread(fsm_ms), _spread(sustain_ms)
    return {"config": 21, "metric": "events/sec (keyed state machines: packed-function scan)",
            "value": batch / nat["median"] * 1e3, "unit": "events/s",
            "ms_per_step": nat["median"], "native_ms": nat, "sustain_ms": ref,
            "sustain_events_per_s": batch / ref["median"] * 1e3,
            "fsm_over_sustain_time": nat["median"] / ref["median"],
            "rows": rows, "rows_per_step": rows // max(1, steps),
            "sustain_rows_per_step": sustain_rows // max(1, steps),
            "keys_seen": int(seen.sum()),
            "keys_per_state": torch.bincount(twin[seen, 1], minlength=states).tolist(),
            "states": states, "classes": op.classes, "keys": keys, "samples_per_step": batch,
            "zipf": zipf, "table_rows": op.cap, "steps": steps, "warmup": warmup,
            "device": str(dev)}


def _rate_torch_step(table, keys, vals, ts, ts_base: int, span: int, per_ms: int, threshold):
    """config 22's yardstick: the counter-rate step written with library ops on long counters --
    stable sort by key, a segmented ``cummax`` of the timestamps (the segment number in the high
    bits, so ``ts - ts_base`` must lie in [0, span)), gathers, the arithmetic, the rows put back
    in arrival order and ``nonzero``. `table` is int64[keys, 2] = (last_ts, last value), last_ts
    I64_MIN for a key never seen; it is updated. On a tie ``cummax`` keeps the later element, the
    rule the earlier one: equal only where, as in config 22, a key's value is a function of its
    timestamp. Returns the five columns."""
    n = keys.numel()
    sk, perm = torch.sort(keys, stable=True)
    t, v = ts[perm], vals[perm]
    head = torch.ones(n, dtype=torch.bool, device=keys.device)
    head[1:] = sk[1:] != sk[:-1]
    seg = torch.cumsum(head, 0) - 1
    cm, at = torch.cummax(seg * span + (t - ts_base), 0)
    carry = table[sk]
    # exclusive: the element in front, unless this one begins its key's run
    run_t = torch.roll(cm, 1) - seg * span + ts_base
    run_v = v[torch.roll(at, 1)]
    in_run = ~head & (run_t > carry[:, 0])
    bt = torch.where(in_run, run_t, carry[:, 0])
    bv = torch.where(in_run, run_v, carry[:, 1])
    based = (t > bt) & (bt != K.I64_MIN)
    inc = torch.where(v >= bv, v - bv, v)
    dt = torch.where(based, t - bt, torch.ones_like(t))
    rate = inc.to(torch.float64) * float(per_ms) / dt.to(torch.float64)
    keep = based if threshold is None else based & (rate < threshold)
    # the state: the run's arg-max against the carry, stored by the row that ends the run
    tail = torch.ones(n, dtype=torch.bool, device=keys.device)
    tail[:-1] = head[1:]
    end_t = cm - seg * span + ts_base
    newer = end_t > carry[:, 0]
    rows = torch.stack([torch.where(newer, end_t, carry[:, 0]),
                        torch.where(newer, v[at], carry[:, 1])], 1)
    table[sk[tail]] = rows[tail]
    # arrival order: scatter by the sort's permutation, then compact
    mask = torch.zeros(n, dtype=torch.bool, device=keys.device)
    mask[perm] = keep
    cols = torch.empty((3, n), dtype=torch.int64, device=keys.device)
    cols[0, perm] = rate.view(torch.int64)
    cols[1, perm] = inc
    cols[2, perm] = dt
    idx = torch.nonzero(mask).squeeze(1)
    return keys[idx], cols[0, idx], cols[1, idx], cols[2, idx], ts[idx]


def config22(steps: int, warmup: int, batch: int | None = None, keys: int = 1_000_000,
             threshold: float | None = None, zipf: float = 0.0, device: str = "cuda") -> dict:
    """Counter rates at scale (``samples.key_by(0).process(CounterRate(2))``) on config 17's keys
    and timestamps: `batch` device-generated samples per 1 s step (gen_events, uniform or zipf
    keys) feed KeyedRateOperator directly. The value column is made on the device: key k's
    counter grows with the timestamp at a slope of its own, 1000 .. 9999 per ms, and restarts
    once every 1000 steps at a phase of its own, so about 0.1 % of the keys report a reset per
    step. Without `threshold` every based sample is a row, the expansion-bound case; with one
    the rule is ``rate < threshold`` (1 090 000 per second keeps the slowest 1 % of the keys).
    The rows leave the device as five int64 columns (key id, rate bits, inc, dt, ts) in arrival
    order.

    Timed per step, each behind a device synchronise, alternating in the same call on the same
    batch: the counter-rate step, config 17's native step (KeyedSustainOperator over a gauge
    column of the same batch, ``for_`` = 3 s) and the torch composition of the same step
    (_rate_torch_step). The ratios are reported, not gated. Outside the windows the C++ twin runs
    every step on host copies: every step's row count and ignored samples, the first three
    steps' rows and the final table must equal the device's, and the composition's row count
    must equal them too. The sample generation is outside the windows."""
    from ..runtime.rate_operator import KeyedRateOperator
    from ..runtime.sustain_operator import KeyedSustainOperator

    dev = torch.device(device)
    batch = batch or (1 << 21)
    when = None if threshold is None else "<"
    op = KeyedRateOperator(1000, when, threshold, device=dev, dense_limit=max(keys, 1 << 26),
                           capacity=keys)
    sustain = KeyedSustainOperator(">", 90, 3_000, device=dev, dense_limit=max(keys, 1 << 26),
                                   capacity=keys)
    twin = K.rate_table(keys, "cpu")
    lib = K.rate_table(keys, dev)
    rule = dict(kind=K.SUSTAIN_LONG, per_ms=1000, when=when, threshold_bits=op.tbits,
                max_gap=None)
    step_ms = 1_000
    t0_event = 1_566_957_600_000
    sk, st, sv, gauge = (torch.empty(batch, dtype=torch.int64, device=dev) for _ in range(4))
    state = {"i": 0}
    rate_ms: list[float] = []
    sustain_ms: list[float] = []
    torch_ms: list[float] = []
    ignored = {"native": 0, "twin": 0}

    def step():
        i = state["i"]
        K.gen_events(sk, st, gauge, seed=17, stream_id=0, idx0=i * batch, nkeys=keys,
                     ts_base=t0_event + i * step_ms, ts_span=step_ms, disorder=0, val_lo=0,
                     val_span=100, zipf=zipf)
        h = (sk + 1) * 2_654_435_761
        slope = 1_000 + h % 9_000
        since = i - (i - (h >> 7) % 1_000) % 1_000      # the key's last restart, a step number
        sv.copy_(slope * (st - (t0_event + since * step_ms)))
        _sync(dev)
        t_in = time.perf_counter()
        out = op.process(sk, sv, st, is_float=False)
        _sync(dev)
        rate_ms.append((time.perf_counter() - t_in) * 1e3)
        t_in = time.perf_counter()
        ref = sustain.process(sk, gauge, st, is_float=False)
        _sync(dev)
        sustain_ms.append((time.perf_counter() - t_in) * 1e3)
        t_in = time.perf_counter()
        comp = _rate_torch_step(lib, sk, sv, st, t0_event + i * step_ms, step_ms, 1000, threshold)
        _sync(dev)
        torch_ms.append((time.perf_counter() - t_in) * 1e3)
        want, ooo = K.rate_update(twin, sk.cpu(), sv.cpu(), st.cpu(), **rule)
        ignored["twin"] += ooo
        rows = int(out[0][0].numel()) if out else 0
        if rows != int(want[0].numel()) or (i < 3 and out and not all(
                torch.equal(a.cpu(), b) for a, b in zip(out[0], want))):
            raise RuntimeError("config 22: the native rows and the twin's differ")
        if int(comp[0].numel()) != rows or (i < 3 and out and not all(
                torch.equal(a, b) for a, b in zip(out[0], comp))):
            raise RuntimeError("config 22: the torch composition's rows and the native ones differ")
        state["i"] = i + 1
        return rows, int(ref[0][0].numel()) if ref else 0

    for _ in range(warmup):
        step()
    rate_ms.clear()
    sustain_ms.clear()
    torch_ms.clear()
    rows = sustain_rows = 0
    for _ in range(steps):
        r, s = step()
        rows, sustain_rows = rows + r, sustain_rows + s
    if not torch.equal(op.state[:keys].cpu(), twin) or op.out_of_order != ignored["twin"]:
        raise RuntimeError("config 22: the native table and the twin's differ")
    if not torch.equal(lib.cpu(), twin):
        raise RuntimeError("config 22: the torch composition's table and the twin's differ")
    nat, ref, comp = _spread(rate_ms), _spread(sustain_ms), _spread(torch_ms)
    return {"config": 22, "metric": "events/sec (counter rates: arg-max scan, dense rows)",
            "value": batch / nat["median"] * 1e3, "unit": "events/s",
            "ms_per_step": nat["median"], "native_ms": nat, "sustain_ms": ref, "torch_ms": comp,
            "sustain_events_per_s": batch / ref["median"] * 1e3,
            "rate_over_sustain_time": nat["median"] / ref["median"],
            "torch_over_rate_time": comp["median"] / nat["median"],
            "rows": rows, "rows_per_step": rows // max(1, steps),
            "row_share": rows / max(1, steps * batch),
            "sustain_rows_per_step": sustain_rows // max(1, steps),
            "out_of_order": op.out_of_order,
            "keys_seen": int((twin[:, 0] != K.RATE_NONE).sum()),
            "threshold": threshold, "keys": keys, "samples_per_step": batch, "zipf": zipf,
            "table_rows": op.cap, "steps": steps, "warmup": warmup, "device": str(dev)}


def bandwidth_text(lines: int, channels: int = 1_000, seed: int = 7) -> np.ndarray:
    """Synthetic chapter3 input (chapter3/README.md:286 format, ``BandwidthMonitorWithEventTime``)
    as fixed-width lines ``yyyy-MM-ddTHH:mm:ss chNNN.example.com VVVVVVVVV`` over one hour of
    event time, built with numpy (a Python f-string per line would dominate a 10^8-line file).
    Healthy channels move 150-300 MB per line; 1 % of the channels are starved (a few KB per
    line) and alert in every 5-min window -- a small alert stream, as in a monitoring system.
    The byte count is zero-padded (Long.parseLong accepts leading zeros)."""
    import datetime as _dt

    rng = np.random.default_rng(seed)
    t0s = 1_566_957_600  # 2019-08-28T10:00:00+08:00
    secs = (np.arange(lines, dtype=np.int64) * 3600) // max(lines, 1)
    tz = _dt.timezone(_dt.timedelta(hours=8))
    stamps = np.frombuffer("".join(_dt.datetime.fromtimestamp(t0s + i, tz).strftime("%Y-%m-%dT%H:%M:%S")
                                   for i in range(3600)).encode(), np.uint8).reshape(3600, 19)
    width = max(3, len(str(channels - 1)))
    names = np.frombuffer("".join(f"ch{c:0{width}d}.example.com" for c in range(channels)).encode(),
                          np.uint8).reshape(channels, width + 14)
    ch = rng.integers(0, channels, lines)
    vals = rng.integers(150_000_000, 300_000_000, lines)
    starved = ch % 100 == 0
    vals[starved] = rng.integers(1, 1000, int(starved.sum()))
    w = 19 + 1 + names.shape[1] + 1 + 9 + 1
    out = np.empty((lines, w), np.uint8)
    out[:, :19] = stamps[secs]
    out[:, 19] = 32
    out[:, 20:20 + names.shape[1]] = names[ch]
    o = 20 + names.shape[1]
    out[:, o] = 32
    v = vals.copy()
    for k in range(8, -1, -1):
        out[:, o + 1 + k] = 48 + (v % 10)
        v //= 10
    out[:, w - 1] = 10
    return out.reshape(-1)


def cpu_metric_text(lines: int, hosts: int = 10_000, seed: int = 11) -> np.ndarray:
    """Synthetic chapter1/2 input ``ts ip cpuN usage`` (Main.java:21-24, ComputeCpuMax.java:20-23)
    as fixed-width lines built with numpy: epoch seconds, an IPv4-like host name out of `hosts`,
    cpu0..cpu63, usage with one decimal (``dd.d``)."""
    rng = np.random.default_rng(seed)
    hn = np.frombuffer("".join(f"10.{i // 65536 % 256:03d}.{i // 256 % 256:03d}.{i % 256:03d}"
                               for i in range(hosts)).encode(), np.uint8).reshape(hosts, 14)
    cn = np.frombuffer("".join(f"cpu{c:02d}" for c in range(64)).encode(), np.uint8).reshape(64, 5)
    h = rng.integers(0, hosts, lines)
    c = rng.integers(0, 64, lines)
    u = rng.integers(0, 1000, lines)  # usage * 10
    w = 10 + 1 + 14 + 1 + 5 + 1 + 4 + 1
    out = np.empty((lines, w), np.uint8)
    t = 1_563_452_000 + np.arange(lines, dtype=np.int64) // max(1, lines // 3600)
    for k in range(9, -1, -1):
        out[:, k] = 48 + (t % 10)
        t //= 10
    out[:, 10] = 32
    out[:, 11:25] = hn[h]
    out[:, 25] = 32
    out[:, 26:31] = cn[c]
    out[:, 31] = 32
    out[:, 32] = 48 + u // 100
    out[:, 33] = 48 + (u // 10) % 10
    out[:, 34] = 46
    out[:, 35] = 48 + u % 10
    out[:, w - 1] = 10
    return out.reshape(-1)


class _ByteCounter:
    """print() target of the API benches: takes the native formatter's bytes (every output row
    is formatted -- Tuple/Double.toString, subtask prefix -- and counted, not written)."""

    def __init__(self):
        self.lines = 0
        self.bytes = 0

    def __call__(self, s: str) -> None:
        self.lines += 1
        self.bytes += len(s) + 1

    def raw(self, data: bytes, nlines: int | None = None) -> None:
        self.lines += data.count(b"\n") if nlines is None else nlines
        self.bytes += len(data)


def config9(lines: int = 16_000_000, hosts: int = 10_000, device: str = "cuda",
            batch_lines: int = 1 << 20, text_ingest: str = "auto") -> dict:
    """The reference's ComputeCpuMax job (ComputeCpuMax.java:15-27: keyBy(0).max(2), one output
    record per input record) through the DataStream API over a text file: readTextFile ->
    map(parse) -> keyBy(host) -> max(usage) -> print. On a GPU: device ingest (dictionary ids),
    the rolling max on the device, the per-record emit as ONE device column batch per micro-batch
    (keep-first template fields gathered by key id), formatted by the native threaded formatter.
    Lines per second end to end (wall clock of env.execute, every output line formatted)."""
    import os
    import tempfile

    from ..api.environment import StreamExecutionEnvironment
    from . import chapters as C

    text = cpu_metric_text(lines, hosts)
    fd, path = tempfile.mkstemp(suffix=".txt")
    with os.fdopen(fd, "wb") as f:
        f.write(text.tobytes())
    line_w = text.size // max(lines, 1)
    fd, head = tempfile.mkstemp(suffix=".txt")
    with os.fdopen(fd, "wb") as f:
        f.write(text[:50_000 * line_w].tobytes())
    del text

    def run(file, batch):
        sink = _ByteCounter()
        env = StreamExecutionEnvironment(4).set_output(sink)
        env.config.native = "auto"
        env.config.device = device
        env.config.batch_size = batch
        env.config.text_ingest = text_ingest
        C.build_compute_cpu_max(env, env.read_text_file(file))
        t = time.perf_counter()
        env.execute("ComputeCpuMax")
        return time.perf_counter() - t, sink

    try:
        run(head, batch_lines)  # warm-up job (module loads, code objects, pinned slots)
        dt, sink = run(path, batch_lines)
    finally:
        os.unlink(path)
        os.unlink(head)
    return {"config": 9, "metric": "lines/sec through the DataStream API (file replay)",
            "value": lines / dt, "unit": "lines/s", "seconds": dt, "output_lines": sink.lines,
            "output_bytes": sink.bytes, "lines": lines, "bytes_per_line": line_w, "hosts": hosts,
            "batch_lines": batch_lines, "job": "ComputeCpuMax (keyBy(0).max(2), rolling emit)",
            "ingest": ("device" if text_ingest == "device" or str(device).startswith("cuda")
                       else "host"), "device": device}


def config7(lines: int = 16_000_000, channels: int = 1_000, device: str = "cuda",
            batch_lines: int = 1 << 20, profile: bool = False) -> dict:
    """The reference's BandwidthMonitorWithEventTime job (BandwidthMonitorWithEventTime.java:25-57)
    through the DataStream API over a text file replay: env.readTextFile -> assigner -> map(parse)
    -> keyBy -> 5 min / 5 s sliding event-time window reduce -> Mbps map -> filter -> sink.
    On a GPU the planner runs it on the device ingest: the C++ reader fills pinned ring slots,
    the batch is parsed on the device with channel names interned in the HBM dictionary, the
    native window operator reads the device columns, the Mbps map + filter run in the fire
    kernel. Lines per second end to end (wall clock of env.execute, the file in the page cache)."""
    import os
    import tempfile

    from ..api.environment import StreamExecutionEnvironment
    from . import chapters as C

    text = bandwidth_text(lines, channels)
    fd, path = tempfile.mkstemp(suffix=".txt")
    with os.fdopen(fd, "wb") as f:
        f.write(text.tobytes())
        # written back before the timed job (in the page cache, clean): dirty-page writeback of
        # the fresh file otherwise competes with the timed read (345-548 M lines/s run to run)
        f.flush()
        os.fsync(f.fileno())
    head_lines = 50_000
    line_w = text.size // max(lines, 1)
    fd, head = tempfile.mkstemp(suffix=".txt")
    with os.fdopen(fd, "wb") as f:
        f.write(text[:head_lines * line_w].tobytes())
    del text

    def run(file, batch):
        alerts = [0]
        env = StreamExecutionEnvironment(4).set_output(lambda s: alerts.__setitem__(0, alerts[0] + 1))
        env.config.native = "auto"
        env.config.device = device
        env.config.batch_size = batch
        C.build_bandwidth_event_time(env, env.read_text_file(file))
        t = time.perf_counter()
        res = env.execute("BandwidthMonitorWithEventTime")
        return time.perf_counter() - t, alerts[0], res

    try:
        # Warm-up job (untimed): module loads, kernel code objects, and the pinned slot pool of
        # this batch size -- a long-running service allocates its page-locked ingest slots once,
        # not per job (4 slots x batch x 48 B: ~13 ms of pinning per 200 MB).
        run(head, batch_lines)
        if profile:
            import cProfile
            import pstats

            pr = cProfile.Profile()
            pr.enable()
        dt, alerts, res = run(path, batch_lines)
        if profile:
            pr.disable()
            pstats.Stats(pr).sort_stats("cumulative").print_stats(40)
    finally:
        os.unlink(path)
        os.unlink(head)
    return {"config": 7, "metric": "lines/sec through the DataStream API (file replay)",
            "value": lines / dt, "unit": "lines/s", "seconds": dt, "alerts": alerts,
            "lines": lines, "bytes_per_line": line_w, "channels": channels,
            "batch_lines": batch_lines,
            "job": "BandwidthMonitorWithEventTime (5 min / 5 s sliding, 1 min bound)",
            "ingest": "device" if str(device).startswith("cuda") else "host", "device": device}


def config10(steps: int, warmup: int, batch: int = 1 << 24, keys: int = 1_000_000,
             device: str = "cuda", top_n: int | None = None, n: int = 10) -> dict:
    """Top-N hosts by bytes per minute at the headline shape: 1M dense keys, 1-min tumbling
    event-time int64 sum, device-generated events, then the N keys with the largest sums of
    every firing. top_n = N: the operator cuts each firing to its candidates on the device
    (KeyedWindowOperator top_n) and the host ranks those; None: the firing leaves in full (one
    28-byte row per key) and numpy takes the top N on the host -- what the same query costs
    without the cut. Both print the same winners (`top_checksum`)."""
    dev = torch.device("cuda", 0) if device != "cpu" and torch.cuda.is_available() \
        else torch.device("cpu")
    step_ms, disorder = 5_000, 2_000
    op = KeyedWindowOperator(size=60_000, agg=K.AGG_SUM_I64, device=dev, max_keys=keys,
                             batch_capacity=batch, ooo_bound=disorder, dense_keys=True,
                             pipeline="stream", **({} if top_n is None else {"top_n": top_n}))
    want = n if top_n is None else top_n
    k = torch.empty(batch, dtype=torch.int64, device=dev)
    ts = torch.empty_like(k)
    vals = torch.empty_like(k)
    t0_event = 1_566_957_600_000
    state = {"i": 0, "check": 0, "windows": 0}
    lat: list[float] = []

    def rank(fr) -> None:
        """The window's top rows: sum descending, key ascending (api/aggregations.WindowTopN)."""
        raw = fr.raw.view(np.int64) if fr.raw.dtype == np.uint64 else fr.raw
        keys_ = fr.keys.view(np.int64) if fr.keys.dtype == np.uint64 else fr.keys
        if raw.size > want:
            thr = np.partition(raw, raw.size - want)[raw.size - want]
            sel = np.nonzero(raw >= thr)[0]
        else:
            sel = np.arange(raw.size)
        order = sel[np.lexsort((keys_[sel], -raw[sel]))][:want]
        state["check"] = (state["check"] * 31 + int(keys_[order].sum()) * 7 + int(raw[order].sum())) % (1 << 61)
        state["windows"] += 1

    def step(drain: bool = False):
        i = state["i"]
        t_in = time.perf_counter()
        if drain:
            fired = op.flush()
        else:
            K.gen_events(k, ts, vals, seed=1234, stream_id=0, idx0=i * batch, nkeys=keys,
                         ts_base=t0_event + i * step_ms, ts_span=step_ms, disorder=disorder,
                         val_lo=0, val_span=20_000)
            fired = op.process(k, ts, vals)
            state["i"] = i + 1
        for fr in fired:
            rank(fr)
        if fired:
            lat.append((time.perf_counter() - t_in) * 1e3)

    for _ in range(warmup):
        step()
    _sync(dev)
    lat.clear()
    out0, fires0 = op.metrics.num_records_out, state["windows"]
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    step(drain=True)
    _sync(dev)
    dt = time.perf_counter() - t0
    fires = state["windows"] - fires0
    rows = op.metrics.num_records_out - out0
    return {"config": 10, "metric": "events/sec (top-N keys of a 1-min tumbling sum, "
                                    + ("device cut)" if top_n is not None else "host cut)"),
            "value": batch * steps / dt, "unit": "events/s", "ms_per_step": dt / steps * 1e3,
            "p50_fire_step_ms": statistics.median(lat) if lat else None,
            "firings_measured": fires, "top_n": want,
            "cut": "device" if top_n is not None else "host",
            "d2h_rows_per_firing": rows / fires if fires else None,
            "d2h_bytes_per_firing": rows * 28 / fires if fires else None,
            "fired_rows_per_firing": (op.metrics.extra.get("topn_rows_in", 0) / op.metrics.num_fires
                                      if top_n is not None and op.metrics.num_fires else
                                      (rows / fires if fires else None)),
            "top_checksum": state["check"], "keys": keys, "events_per_step": batch,
            "device": str(dev)}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, required=True, choices=[1, 2, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22])
    ap.add_argument("--top-n", type=int, nargs="?", const=10, default=None,
                    help="config 10: cut every firing to its top N on the device (default N = "
                         "10); without it the firing leaves in full and numpy takes the top 10")
    ap.add_argument("--dim", type=int, default=32, help="config 6: metric vector width")
    ap.add_argument("--valu", action="store_true", help="config 6: VALU instead of MFMA reduce")
    ap.add_argument("--zipf", type=float, default=0.0,
                    help="config 6 / 13: power-law key skew (13: 1.2 is the hot-key case)")
    ap.add_argument("--host-fold", action="store_true",
                    help="config 5: fold records of spilled keys in host DRAM (no promotion to HBM)")
    ap.add_argument("--spill", action="store_true",
                    help="configs 2/4: key space outgrowing the HBM table (host-DRAM tier)")
    ap.add_argument("--ckpt", action="store_true",
                    help="config 5: time one synchronous checkpoint after the timed loop")
    ap.add_argument("--no-pipeline", action="store_true",
                    help="config 5: the unpipelined session step")
    ap.add_argument("--revisit", type=float, default=0.0,
                    help="config 5: fraction of events for spilled (long idle) keys")
    ap.add_argument("--lo", type=int, default=-500, help="config 14: lower bound in ms")
    ap.add_argument("--hi", type=int, default=500, help="config 14: upper bound in ms")
    ap.add_argument("--when", choices=["gt", "none", "<"], default="gt",
                    help="config 15: sample > threshold (about 1 %% kept) or keep every sample; "
                         "config 22: '<' adds the rule rate < --threshold (otherwise every based "
                         "sample is a row)")
    ap.add_argument("--threshold", type=float, default=1_090_000.0,
                    help="config 22 with --when '<': the rate per second below which a sample "
                         "leaves (the default keeps the slowest 1 %% of the keys)")
    ap.add_argument("--timeout-ms", type=int, default=3_000,
                    help="config 16: a key fires after this much silence (event time)")
    ap.add_argument("--for-ms", type=int, default=3_000,
                    help="config 17: a key is reported once its condition has held this long")
    ap.add_argument("--times", type=int, default=5,
                    help="config 18: a key is reported at this many breaches")
    ap.add_argument("--within-ms", type=int, default=3_000,
                    help="config 18: within this span (event time)")
    ap.add_argument("--disorder-ms", type=int, default=3_000,
                    help="config 19: timestamps are displaced backwards uniformly within this "
                         "span, and the watermark runs this far behind (0: an in-order stream)")
    ap.add_argument("--rules", type=int, default=8,
                    help="config 20: rules in force (1 .. 64); rule r is > 9900 + 10 r")
    ap.add_argument("--states", type=int, default=3,
                    help="config 21: 3 is the severity with hysteresis; any other count in "
                         "[2, 16] a saturating counter of breaches in a row (16: the widest "
                         "packed function)")
    ap.add_argument("--dense", action="store_true",
                    help="config 20: every sample breaks every rule (the expansion-bound case)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=None,
                    help="events per step; config 13: per side and step (default 2**21, and "
                         "2**15 with --zipf, where a hot key's pairs grow with the square of "
                         "its events)")
    ap.add_argument("--lines", type=int, default=None, help="config 7: lines in the file")
    ap.add_argument("--profile", action="store_true", help="config 7: cProfile the job")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--gpu-parse", action="store_true", help="config 1 on the GPU parse path")
    ap.add_argument("--hashed-keys", action="store_true",
                    help="configs 2/4: hashed keyed state instead of dictionary-id slots")
    ap.add_argument("--sort-path", action="store_true",
                    help="config 2: the radix-sort rolling path instead of the sort-free one")
    ap.add_argument("--keys", type=int, default=None, help="config 2: key space (default 10k); config 13: 100k")
    ap.add_argument("--size", type=int, default=None,
                    help="config 11: count-window size (default 100); config 12: the tumbling "
                         "countWindow(size) instead of the rolling aggregate; config 13: window "
                         "size in ms (default 1000)")
    ap.add_argument("--by", choices=["max", "min"], default=None,
                    help="config 12: the arg-select scan of maxBy / minBy instead of the plain max")
    ap.add_argument("--slide", type=int, default=None,
                    help="config 11: count-window slide (omitted: the tumbling countWindow(size)); "
                         "config 13: window slide in ms (omitted: tumbling)")
    ap.add_argument("--latency-fire", type=int, default=0,
                    help="config 4: fire right away when at most this many windows are due "
                         "(latency-bounded mode; 0 = pipelined firing)")
    ap.add_argument("--quantiles", default=None,
                    help="config 8: comma-separated quantiles in [0, 1] (e.g. 0.5,0.95,0.99) "
                         "instead of the median")
    ap.add_argument("--distinct", action="store_true",
                    help="config 8: the exact per-key distinct count instead of the median")
    ap.add_argument("--threads", type=int, default=4,
                    help="config 1 CPU path: parse threads (the reference job runs at P = 4)")
    a = ap.parse_args(argv)
    if a.config == 1:
        r = config1(a.steps, a.warmup, a.batch or (1 << 20),
                    device="cpu" if a.device == "cuda" and not a.gpu_parse else a.device,
                    threads=a.threads)
    elif a.config == 2 and a.spill:
        r = config2_spill(a.steps, a.warmup, a.batch or (1 << 22), device=a.device,
                          revisit=a.revisit or 0.01)
    elif a.config == 2:
        r = config2(a.steps, a.warmup, a.batch or (1 << 24), device=a.device,
                    keys=a.keys or 10_000, dense_keys=not a.hashed_keys,
                    sort_free=not a.sort_path)
    elif a.config == 4 and a.spill:
        r = config4_spill(a.steps, a.warmup, a.batch or (1 << 22), device=a.device)
    elif a.config == 4:
        r = config4(a.steps, a.warmup, a.batch or (1 << 24), device=a.device,
                    dense_keys=not a.hashed_keys, latency_fire=a.latency_fire)
    elif a.config == 7:
        r = config7(lines=a.lines or 16_000_000, device=a.device,
                    batch_lines=a.batch or (1 << 20), profile=a.profile)
    elif a.config == 9:
        r = config9(lines=a.lines or 16_000_000, device=a.device,
                    batch_lines=a.batch or (1 << 20))
    elif a.config == 8:
        r = config8(a.steps, a.warmup, a.batch or (1 << 22), device=a.device,
                    quantiles=[float(x) for x in a.quantiles.split(",")] if a.quantiles else None,
                    distinct=a.distinct)
    elif a.config == 10:
        r = config10(a.steps, a.warmup, a.batch or (1 << 24), keys=a.keys or 1_000_000,
                     device=a.device, top_n=a.top_n)
    elif a.config == 11:
        r = config11(a.steps, a.warmup, a.batch or (1 << 24), keys=a.keys or 10_000,
                     size=a.size or 100, slide=a.slide, device=a.device)
    elif a.config == 12:
        r = config12(a.steps, a.warmup, a.batch or (1 << 24), keys=a.keys or 10_000,
                     size=a.size or 0, by=a.by, device=a.device)
    elif a.config == 13:
        r = config13(a.steps, a.warmup, a.batch, keys=a.keys or 100_000, size=a.size or 1_000,
                     slide=a.slide, zipf=a.zipf, device=a.device)
    elif a.config == 14:
        r = config14(a.steps, a.warmup, a.batch, keys=a.keys or 100_000, lo=a.lo, hi=a.hi,
                     zipf=a.zipf, device=a.device)
    elif a.config == 15:
        r = config15(a.steps, a.warmup, a.batch, keys=a.keys or 1_000_000,
                     when=">" if a.when == "gt" else None, zipf=a.zipf, device=a.device)
    elif a.config == 16:
        r = config16(a.steps, a.warmup, a.batch, keys=a.keys or 1_000_000,
                     timeout_ms=a.timeout_ms, zipf=a.zipf, device=a.device)
    elif a.config == 17:
        r = config17(a.steps, a.warmup, a.batch, keys=a.keys or 1_000_000, for_ms=a.for_ms,
                     zipf=a.zipf, device=a.device)
    elif a.config == 18:
        r = config18(a.steps, a.warmup, a.batch, keys=a.keys or 1_000_000, times=a.times,
                     within_ms=a.within_ms, zipf=a.zipf, device=a.device)
    elif a.config == 19:
        r = config19(a.steps, a.warmup, a.batch, keys=a.keys or 1_000_000, for_ms=a.for_ms,
                     disorder_ms=a.disorder_ms, zipf=a.zipf, device=a.device)
    elif a.config == 20:
        r = config20(a.steps, a.warmup, a.batch, keys=a.keys or 1_000_000, rules=a.rules,
                     dense=a.dense, device=a.device)
    elif a.config == 21:
        r = config21(a.steps, a.warmup, a.batch, keys=a.keys or 1_000_000, states=a.states,
                     zipf=a.zipf, device=a.device)
    elif a.config == 22:
        r = config22(a.steps, a.warmup, a.batch, keys=a.keys or 1_000_000,
                     threshold=a.threshold if a.when == "<" else None, zipf=a.zipf,
                     device=a.device)
    elif a.config == 6:
        r = config6(a.steps, a.warmup, a.batch or (1 << 24), dim=a.dim, device=a.device,
                    mfma=not a.valu, zipf=a.zipf)
    else:
        r = config5(a.steps, a.warmup, a.batch or (1 << 24), device=a.device, revisit=a.revisit,
                    promote=not a.host_fold, pipeline=False if a.no_pipeline else None,
                    ckpt=a.ckpt)
    print(json.dumps(r), flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
