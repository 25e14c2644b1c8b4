"""``keyBy(k).countWindow(size, slide)`` through the DataStream API: the native sliding count
window (NativeCountWindowOp in its sliding mode) against the exact host WindowOperator."""
from collections import Counter

import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

from mxstream.api import windowing as W
from mxstream.api.environment import StreamExecutionEnvironment
from mxstream.api.tuples import Tuple2
from mxstream.runtime.executor import ManualClock

KEYS = ["a", "b", "c", "10.8.22.1"]


def _avg():
    from mxstream.api.functions import AggregateFunction

    class Avg(AggregateFunction):
        def create_accumulator(self):
            return Tuple2(0, 0)

        def add(self, v, acc):
            return Tuple2(acc.f0 + 1, acc.f1 + v.f1)

        def get_result(self, acc):  # (the guard is what lets the planner trace it)
            return acc.f1 / acc.f0 if acc.f0 else 0.0

        def merge(self, a, b):
            return Tuple2(a.f0 + b.f0, a.f1 + b.f1)

    return Avg()


def _apply(ws, agg):
    if agg == "reduce":
        return ws.reduce(lambda a, b: Tuple2(a.f0, a.f1 + b.f1))
    if agg == "avg":
        return ws.aggregate(_avg())
    return getattr(ws, agg)(1)


def _run_slide(events, size, slide, native, agg):
    out = []
    env = StreamExecutionEnvironment(4, clock=ManualClock(0)).set_output(out.append)
    env.config.native = native
    ws = (env.from_collection(events).map(lambda e: Tuple2(e[0], e[1])).key_by(0)
          .count_window(size, slide))
    _apply(ws, agg).print()
    env.execute("sliding count")
    return out


def _planned_ops(stream):
    from mxstream.api import planner
    from mxstream.runtime.executor import Executor

    stream.print()
    env = stream.env
    sinks = planner.plan(env, list(env._sinks))
    return [n.factory() for n in Executor._topo(sinks) if n.kind == "op"]


@settings(max_examples=50, deadline=None, suppress_health_check=[HealthCheck.too_slow])
@given(events=st.lists(st.tuples(st.sampled_from(KEYS), st.integers(0, 1000)),
                       min_size=1, max_size=60),
       size=st.integers(1, 6), slide=st.integers(1, 6),
       agg=st.sampled_from(["reduce", "sum", "min", "max", "avg"]))
def test_native_sliding_count_window_equals_host(events, size, slide, agg):
    a = _run_slide(events, size, slide, "off", agg)
    b = _run_slide(events, size, slide, "auto", agg)
    assert Counter(a) == Counter(b)


@pytest.mark.parametrize("floats", [False, True])
@pytest.mark.parametrize("name", ["SumAggregate", "CountAggregate", "AvgAggregate",
                                  "MinAggregate", "MaxAggregate"])
def test_builtin_aggregates_over_sliding_count_windows(name, floats):
    """avg divides by, and count reports, the window's real element count min(m, size)."""
    from mxstream.api import aggregations as A

    rng = np.random.default_rng(3)
    ev = [(KEYS[int(rng.integers(0, 4))],
           float(rng.integers(-800, 800)) / 8 if floats else int(rng.integers(-100, 100)))
          for _ in range(70)]
    res = {}
    for native in ("off", "auto"):
        out = []
        env = StreamExecutionEnvironment(4, clock=ManualClock(0)).set_output(out.append)
        env.config.native = native
        (env.from_collection(ev).map(lambda e: Tuple2(e[0], e[1])).key_by(0)
         .count_window(5, 2).aggregate(getattr(A, name)(1)).print())
        env.execute("builtin")
        res[native] = Counter(out)
    assert res["auto"] == res["off"] and len(res["off"]) > 0


def test_issue_examples_through_the_api():
    ev = [("a", v) for v in range(1, 12)]
    for native in ("off", "auto"):
        assert sorted(int(ln.split(",")[-1].rstrip(")")) for ln in
                      _run_slide(ev, 4, 2, native, "sum")) == [3, 10, 18, 26, 34]
        assert sorted(int(ln.split(",")[-1].rstrip(")")) for ln in
                      _run_slide(ev, 3, 5, native, "sum")) == [12, 27]


def test_native_sliding_count_window_is_selected():
    from mxstream.runtime.native_ops import NativeCountWindowOp

    env = StreamExecutionEnvironment(4)
    ops = _planned_ops(env.from_collection([("a", 1)]).key_by(0).count_window(4, 2)
                       .reduce(lambda a, b: Tuple2(a.f0, a.f1 + b.f1)))
    sel = [o for o in ops if isinstance(o, NativeCountWindowOp)]
    assert len(sel) == 1 and (sel[0].count, sel[0].slide) == (4, 2)
    env = StreamExecutionEnvironment(4)
    ops = _planned_ops(env.from_collection([("a", 1)]).map(lambda e: Tuple2(e[0], e[1]))
                       .key_by(0).count_window(4, 2).aggregate(_avg()))
    sel = [o for o in ops if isinstance(o, NativeCountWindowOp)]
    assert len(sel) == 1 and (sel[0].kind, sel[0].slide) == ("avg", 2)


def test_unsupported_sliding_count_windows_stay_on_the_host():
    from mxstream.runtime.native_ops import NativeCountWindowOp
    from mxstream.runtime.operators import WindowOp

    def red(ws):
        return ws.reduce(lambda a, b: Tuple2(a.f0, a.f1 + b.f1))

    def keyed():
        return StreamExecutionEnvironment(4).from_collection([("a", 1)]).key_by(0)

    shapes = [
        red(keyed().count_window(130, 1)),  # 130 panes per window
        red(keyed().window(W.GlobalWindows.create()).evictor(W.CountEvictor.of(4, True))
            .trigger(W.CountTrigger.of(2))),  # evicts after the function
        red(keyed().window(W.GlobalWindows.create()).evictor(W.CountEvictor.of(4))
            .trigger(W.PurgingTrigger.of(W.CountTrigger.of(2)))),  # purging trigger
    ]
    for s in shapes:
        ops = _planned_ops(s)
        assert not any(isinstance(o, NativeCountWindowOp) for o in ops)
        assert any(type(o) is WindowOp for o in ops)
    ops = _planned_ops(red(keyed().count_window(192, 3)))  # 64 panes: the largest lowered
    assert any(isinstance(o, NativeCountWindowOp) for o in ops)


@pytest.mark.gpu
def test_native_sliding_count_windows_match_host_on_gpu(monkeypatch, gpu_device):
    monkeypatch.setenv("MXS_DEVICE", "cuda")
    rng = np.random.default_rng(7)
    for trial in range(8):
        ev = [(KEYS[int(rng.integers(0, 4))], int(rng.integers(0, 1000)))
              for _ in range(int(rng.integers(5, 80)))]
        size, slide = int(rng.integers(1, 7)), int(rng.integers(1, 7))
        for agg in ("reduce", "max", "sum", "avg"):
            assert Counter(_run_slide(ev, size, slide, "auto", agg)) == \
                Counter(_run_slide(ev, size, slide, "off", agg))
