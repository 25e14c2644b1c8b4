"""``keyBy(k).maxBy(p)`` / ``minBy(p)``, rolling and over ``countWindow(n)``, through the
DataStream API: the native operators (NativeRollingByOp / NativeCountWindowByOp on the
arg-select engine) against the exact host operators (``native="off"``)."""
import random
from collections import Counter

import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

from mxstream.api import windowing as W
from mxstream.api.environment import StreamExecutionEnvironment
from mxstream.api.time import Time
from mxstream.api.tuples import Tuple3, Tuple4
from mxstream.models import chapters as C
from mxstream.runtime.executor import ManualClock
from mxstream.runtime.operators import LONG_MIN, OpContext, Rec

HOSTS = ["a", "b", "c", "10.8.22.1"]
PROCS = ["p0", "p1", "p2", "p3", "p4"]


def _job(events, by, native, count=None, batch_size=7, comm=None, device=None, pos=2):
    out = []
    env = StreamExecutionEnvironment(4, clock=ManualClock(0)).set_output(out.append)
    env.config.native = native
    if device is not None:
        env.config.device = device
    env._comm = comm
    s = (env.from_collection(events, batch_size=batch_size)
         .map(lambda e: Tuple3(e[0], e[1], e[2])).key_by(0))
    if count is not None:
        s = s.count_window(count)
    getattr(s, by)(pos).print()
    env.execute("by")
    return out


def _per_key(lines):
    """host -> its printed lines in order (a key's records all print from one subtask)."""
    d = {}
    for ln in lines:
        body = ln.split("> ", 1)[1] if "> " in ln else ln
        d.setdefault(body[1:].split(",", 1)[0], []).append(body)
    return d


def _events(floats):
    val = st.integers(0, 3)
    if floats:
        val = val.map(lambda v: v / 4)
    return st.lists(st.tuples(st.sampled_from(HOSTS), st.sampled_from(PROCS), val),
                    min_size=1, max_size=60)


# ---- 1. native equals host --------------------------------------------------------------------
@settings(max_examples=40, deadline=None, suppress_health_check=list(HealthCheck))
@given(data=st.data(), floats=st.booleans(), by=st.sampled_from(["max_by", "min_by"]))
def test_native_rolling_by_equals_host(data, floats, by):
    ev = data.draw(_events(floats))
    a = _job(ev, by, "off")
    b = _job(ev, by, "auto")
    assert Counter(a) == Counter(b) and len(a) == len(ev)
    assert _per_key(a) == _per_key(b)  # rolling: in order per key


@settings(max_examples=40, deadline=None, suppress_health_check=list(HealthCheck))
@given(data=st.data(), floats=st.booleans(), by=st.sampled_from(["max_by", "min_by"]),
       n=st.integers(1, 5))
def test_native_count_window_by_equals_host(data, floats, by, n):
    ev = data.draw(_events(floats))
    a = _job(ev, by, "off", count=n)
    b = _job(ev, by, "auto", count=n)
    assert Counter(a) == Counter(b)
    assert _per_key(a) == _per_key(b)


def test_winner_record_is_emitted_whole():
    """maxBy carries the winner's other fields; ties keep the earlier record."""
    ev = [("h", "init", 5), ("h", "idle", 3), ("h", "java", 97), ("h", "tie", 97),
          ("h", "gcc", 98), ("g", "sh", 1)]
    for native in ("off", "auto"):
        got = _per_key(_job(ev, "max_by", native, batch_size=2))
        assert got["h"] == ["(h,init,5)", "(h,init,5)", "(h,java,97)", "(h,java,97)",
                            "(h,gcc,98)"]
        got = _per_key(_job(ev, "min_by", native, batch_size=2))
        assert got["h"] == ["(h,init,5)", "(h,idle,3)", "(h,idle,3)", "(h,idle,3)", "(h,idle,3)"]
        got = _per_key(_job(ev, "max_by", native, count=2, batch_size=3))
        assert got["h"] == ["(h,init,5)", "(h,java,97)"]


def test_supported_data_runs_on_the_engine(monkeypatch):
    """Tuples of string / int keys and int / float values never reach the host operator."""
    from mxstream.runtime import native_ops as N
    from mxstream.runtime.rolling_operator import KeyedRollingOperator

    def no_fallback(self):
        raise AssertionError("fell back to the host operator")

    built = []
    init = KeyedRollingOperator.__init__

    def spy(self, **kw):
        init(self, **kw)
        built.append((self.arg_select, self.count_window))

    monkeypatch.setattr(N.NativeRollingByOp, "_to_fallback", no_fallback)
    monkeypatch.setattr(N.NativeCountWindowByOp, "_to_fallback", no_fallback)
    monkeypatch.setattr(KeyedRollingOperator, "__init__", spy)
    rng = random.Random(2)
    for floats in (False, True):
        ev = [(rng.choice(HOSTS), rng.choice(PROCS), rng.randint(0, 3) / (4 if floats else 1))
              for _ in range(50)]
        ev = [(h, p, float(v) if floats else int(v)) for h, p, v in ev]
        assert Counter(_job(ev, "max_by", "auto")) == Counter(_job(ev, "max_by", "off"))
        assert Counter(_job(ev, "min_by", "auto", count=3)) == \
            Counter(_job(ev, "min_by", "off", count=3))
    assert built and all(a for a, _ in built) and {c for _, c in built} == {0, 3}


def test_int_keys_and_wider_records():
    rng = random.Random(5)
    ev = [(rng.randint(0, 5), f"p{rng.randint(0, 3)}", rng.randint(0, 3), i) for i in range(80)]
    res = {}
    for native in ("off", "auto"):
        for count in (None, 3):
            out = []
            env = StreamExecutionEnvironment(4, clock=ManualClock(0)).set_output(out.append)
            env.config.native = native
            s = (env.from_collection(ev, batch_size=9)
                 .map(lambda e: Tuple4(e[0], e[1], e[2], e[3])).key_by(0))
            if count:
                s = s.count_window(count)
            s.min_by(2).print()
            env.execute("wide")
            res[native, count] = out
    for count in (None, 3):
        assert Counter(res["auto", count]) == Counter(res["off", count])
        assert _per_key(res["auto", count]) == _per_key(res["off", count])
        assert len(res["off", count]) > 0


# ---- 2. planner shape ---------------------------------------------------------------------------
def _planned_ops(stream):
    from mxstream.api import planner
    from mxstream.runtime.executor import Executor

    stream.print()
    env = stream.env
    sinks = planner.plan(env, list(env._sinks))
    return [n.factory() for n in Executor._topo(sinks) if n.kind == "op"]


def _keyed(key=0):
    env = StreamExecutionEnvironment(4)
    return env.from_collection([("a", "p", 1)]).map(lambda e: Tuple3(e[0], e[1], e[2])).key_by(key)


def test_rolling_by_lowers_to_the_native_operator():
    from mxstream.runtime.native_ops import NativeRollingByOp

    for by, kind in (("max_by", "maxBy"), ("min_by", "minBy")):
        sel = [o for o in _planned_ops(getattr(_keyed(), by)(2))
               if isinstance(o, NativeRollingByOp)]
        assert len(sel) == 1 and (sel[0].kind, sel[0].key_pos, sel[0].val_pos) == (kind, 0, 2)


def test_count_window_by_lowers_to_the_native_operator():
    from mxstream.runtime.native_ops import NativeCountWindowByOp

    for by, kind in (("max_by", "maxBy"), ("min_by", "minBy")):
        sel = [o for o in _planned_ops(getattr(_keyed().count_window(4), by)(2))
               if isinstance(o, NativeCountWindowByOp)]
        assert len(sel) == 1 and (sel[0].kind, sel[0].count, sel[0].slide) == (kind, 4, 0)


def test_unsupported_by_shapes_stay_on_the_host():
    from mxstream.runtime.native_ops import NativeRollingOp
    from mxstream.runtime.operators import RollingReduceOp, WindowOp

    shapes = [
        _keyed().count_window(4, 2).max_by(2),                       # sliding count window
        _keyed().time_window(Time.seconds(5)).max_by(2),             # time window
        _keyed().window(W.EventTimeSessionWindows.with_gap(Time.seconds(5))).min_by(2),
        _keyed(lambda t: t.f0).count_window(4).max_by(2),            # key selector
    ]
    for s in shapes:
        ops = _planned_ops(s)
        assert not any(isinstance(o, NativeRollingOp) for o in ops)
        assert any(type(o) is WindowOp for o in ops)
    ops = _planned_ops(_keyed(lambda t: t.f0).max_by(2))             # key selector, rolling
    assert not any(isinstance(o, NativeRollingOp) for o in ops)
    assert any(type(o) is RollingReduceOp for o in ops)


def test_unlowered_by_shapes_still_equal_the_host():
    rng = random.Random(9)
    ev = [(rng.choice(HOSTS), rng.choice(PROCS), rng.randint(0, 3)) for _ in range(70)]

    def run(native, shape):
        out = []
        env = StreamExecutionEnvironment(4, clock=ManualClock(0)).set_output(out.append)
        env.config.native = native
        s = env.from_collection(ev, batch_size=7).map(lambda e: Tuple3(e[0], e[1], e[2]))
        if shape == "slide":
            s.key_by(0).count_window(4, 2).max_by(2).print()
        elif shape == "selector":
            s.key_by(lambda t: t.f0).min_by(2).print()
        else:
            s.key_by(0).window(W.TumblingProcessingTimeWindows.of(Time.seconds(5))) \
                .max_by(2).print()
        env.execute("unlowered")
        return out

    for shape in ("slide", "selector", "time"):
        a, b = run("off", shape), run("auto", shape)
        assert Counter(a) == Counter(b)
        if shape != "time":
            assert len(a) > 0


# ---- 3. checkpoints -----------------------------------------------------------------------------
def _ctx():
    return OpContext("by", 4, 128, lambda: 0, "ProcessingTime")


@pytest.mark.parametrize("count", [None, 3])
@pytest.mark.parametrize("by", ["max_by", "min_by"])
def test_snapshot_restore_mid_stream_continues_identically(by, count):
    from mxstream.runtime.native_ops import NativeCountWindowByOp, NativeRollingByOp

    rng = random.Random(11)
    recs = [Rec(Tuple3(rng.choice(HOSTS), rng.choice(PROCS), rng.randint(0, 3)), LONG_MIN, 0)
            for _ in range(90)]
    s = getattr(_keyed().count_window(count) if count else _keyed(), by)(2)
    cls = NativeCountWindowByOp if count else NativeRollingByOp

    def fresh():
        op = [o for o in _planned_ops(s) if isinstance(o, cls)][0]
        op.open(_ctx())
        return op

    def feed(op, part):
        out = []
        for i in range(0, len(part), 8):
            out += op.process(part[i:i + 8])
        return [(r.value, r.ts, r.subtask) for r in out]

    whole = fresh()
    ref = feed(whole, recs)
    first = fresh()
    head = feed(first, recs[:45])
    snap = first.snapshot()
    assert snap["engine"]["meta"]["arg_select"] is True and snap["templates"]
    second = fresh()
    second.restore(snap)
    assert head + feed(second, recs[45:]) == ref and len(ref) > 10
    # the restored operator holds native state: unsupported data raises, as after any batch
    with pytest.raises(TypeError):
        second.process([Rec(Tuple3("a", "p", "text"), LONG_MIN, 0)])


# ---- 4. NaN and mixed types ---------------------------------------------------------------------
@pytest.mark.parametrize("count", [None, 2])
def test_nan_and_mixed_first_batches_fall_back(count):
    nan = float("nan")
    cases = [
        [("a", "p0", 1.0), ("a", "p1", nan), ("a", "p2", 2.0), ("b", "p3", 0.5), ("a", "p4", 3.0)],
        [("a", "p0", 1), ("a", "p1", 2.5), ("b", "p2", 2), ("a", "p3", 0), ("b", "p4", 7)],
        [("a", "p0", "x"), ("a", "p1", "y"), ("b", "p2", "z"), ("a", "p3", "w")],
    ]
    for ev in cases:
        a = _job(ev, "max_by", "off", count=count, batch_size=16)
        b = _job(ev, "max_by", "auto", count=count, batch_size=16)
        assert Counter(a) == Counter(b) and len(a) > 0


def test_nan_after_native_state_raises():
    from mxstream.runtime.executor import JobExecutionException

    ev = [("a", "p0", 1.0), ("a", "p1", 2.0), ("a", "p2", float("nan"))]
    assert len(_job(ev, "max_by", "off", batch_size=2)) == 3
    with pytest.raises((JobExecutionException, TypeError)):
        _job(ev, "max_by", "auto", batch_size=2)


# ---- 5. two ranks -------------------------------------------------------------------------------
def _rank_events():
    """A host's events stay on one source partition at G = 2 (the source deals rank::world), so
    its arrival order, and with it every rolling winner, is the single-rank one."""
    rng = random.Random(21)
    return [(HOSTS[(i % 2) * 2 + rng.randint(0, 1)], rng.choice(PROCS), rng.randint(0, 3))
            for i in range(120)]


def test_two_loopback_ranks_equal_one():
    from mxstream.parallel.comm import run_loopback

    ev = _rank_events()
    for by, count in (("max_by", None), ("min_by", 3)):
        ref = _job(ev, by, "auto", count=count, batch_size=10)
        res = run_loopback(2, lambda comm: _job(ev, by, "auto", count=count, batch_size=10,
                                                comm=comm))
        got = [ln for out in res for ln in out]
        assert Counter(got) == Counter(ref) and _per_key(got) == _per_key(ref)


def _gloo_worker(rank, world, port, q):
    import os

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    try:
        ev = _rank_events()
        q.put((rank, [_job(ev, "max_by", "auto", batch_size=10),
                      _job(ev, "min_by", "auto", count=3, batch_size=10)], None))
    except Exception:  # noqa: BLE001
        import traceback

        q.put((rank, [], traceback.format_exc()))
    import torch.distributed as dist

    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


def test_two_gloo_processes_equal_one():
    import os
    import socket

    import torch.multiprocessing as mp

    for k in ("RANK", "WORLD_SIZE"):
        os.environ.pop(k, None)
    ev = _rank_events()
    ref = [_job(ev, "max_by", "auto", batch_size=10),
           _job(ev, "min_by", "auto", count=3, batch_size=10)]
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
    errs = [e for *_, e in res if e]
    assert not errs, errs
    for j in range(2):
        got = [ln for _, outs, _ in res for ln in outs[j]]
        assert Counter(got) == Counter(ref[j]) and _per_key(got) == _per_key(ref[j])


# ---- 6. GPU: the ComputeCpuMax-shaped file job with maxBy(2) -------------------------------------
def _cpu_lines(n):
    """"ts host cpuN usage" lines; host 10.8.0.1 climbs all the way, so its winner changes in
    every later micro-batch; the others tie and repeat (one decimal)."""
    rng = random.Random(3)
    out = []
    for i in range(n):
        h = rng.randint(0, 12)
        usage = (i * 100.0 / n) if h == 1 else rng.randint(0, 40) / 2
        out.append(f"{1563452000 + i} 10.8.0.{h} cpu{rng.randint(0, 7)} {usage:.1f}")
    return out


def _file_job(tmp_path, lines, native, device, by="max_by", replay=False):
    """readTextFile -> map(parse) -> keyBy(host) -> maxBy(usage) -> print. replay: the file's
    lines as a text collection in micro-batches of 256 lines (the file reader's ring hands a GPU
    ingest chunks of a megabyte or more: a few thousand lines are ONE batch there)."""
    path = tmp_path / "cpu.txt"
    path.write_text("\n".join(lines) + "\n")
    out = []
    env = StreamExecutionEnvironment(4, clock=ManualClock(0)).set_output(out.append)
    env.config.native = native
    env.config.device = device
    env.config.batch_size = 256
    if replay:
        env.config.text_ingest = "device"
        text = env.from_collection(path.read_text().splitlines(), batch_size=256)
    else:
        text = env.read_text_file(str(path))
    getattr(text.map(C.ParseCpu()).key_by(0), by)(2).print()
    env.execute("ComputeCpuMaxBy")
    return out


@pytest.mark.parametrize("replay", [False, True])
def test_file_job_cpu_equals_host(tmp_path, replay):
    lines = _cpu_lines(3000)
    host = _file_job(tmp_path, lines, "off", "cpu")
    got = _file_job(tmp_path, lines, "auto", "cpu", replay=replay)
    assert Counter(got) == Counter(host) and _per_key(got) == _per_key(host)
    assert len(set(_per_key(host)["10.8.0.1"])) > 50  # the winner keeps changing


@pytest.mark.gpu
@pytest.mark.parametrize("replay", [False, True])
@pytest.mark.parametrize("by", ["max_by", "min_by"])
def test_file_job_gpu_device_path_equals_host(tmp_path, gpu_device, monkeypatch, by, replay):
    from mxstream.runtime import native_ops as N

    device_batches = []
    orig = N.NativeRollingByOp._run_device

    def spy(self, batches):
        device_batches.append(len(batches))
        return orig(self, batches)

    monkeypatch.setattr(N.NativeRollingByOp, "_run_device", spy)
    lines = _cpu_lines(3000)
    host = _file_job(tmp_path, lines, "off", "cpu", by)
    got = _file_job(tmp_path, lines, "auto", "cuda", by, replay)
    # device ingest and the device emit path; replayed: many micro-batches, so the stored
    # winner rows of one batch are read, and replaced, by the next
    assert len(device_batches) > (5 if replay else 0)
    assert Counter(got) == Counter(host) and _per_key(got) == _per_key(host)
    assert len(set(_per_key(host)["10.8.0.1"])) > (50 if by == "max_by" else 0)


@pytest.mark.gpu
def test_native_by_matches_host_on_gpu(gpu_device, monkeypatch):
    from mxstream.runtime.rolling_operator import KeyedRollingOperator

    engines = []
    init = KeyedRollingOperator.__init__

    def spy(self, **kw):
        init(self, **kw)
        engines.append((self.device.type, self.arg_select))

    monkeypatch.setattr(KeyedRollingOperator, "__init__", spy)
    rng = np.random.default_rng(7)
    for trial in range(4):
        ev = [(HOSTS[int(rng.integers(0, 4))], PROCS[int(rng.integers(0, 5))],
               int(rng.integers(0, 4))) for _ in range(int(rng.integers(5, 150)))]
        for by in ("max_by", "min_by"):
            for count in (None, 1 + trial):
                a = _job(ev, by, "off", count=count)
                b = _job(ev, by, "auto", count=count, device="cuda")
                assert Counter(a) == Counter(b) and _per_key(a) == _per_key(b)
    assert len(engines) == 16 and set(engines) == {("cuda", True)}
