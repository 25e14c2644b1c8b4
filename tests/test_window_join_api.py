"""``a.join(b).where().equal_to().window().apply(fn)`` and ``co_group`` (api/joins.py): the host
plan is Flink's (tag, union, keyed window, co-group function); the planner lowers a projection
join over tumbling / sliding event-time windows onto NativeJoinOp. Firings compare as multisets."""
from __future__ import annotations

import re
from collections import Counter

import pytest

from mxstream.api.tuples import Tuple2, Tuple3

PROJECT = lambda l, r: Tuple3(l.f0, l.f1, r.f1)  # noqa: E731


def _env(native="auto", tmp_path=None, fault=None, comm=None):
    from mxstream.api.environment import (FsStateBackend, RestartStrategies,
                                          StreamExecutionEnvironment)
    from mxstream.api.time import TimeCharacteristic
    from mxstream.runtime.executor import ManualClock

    out = []
    env = StreamExecutionEnvironment(4, clock=ManualClock(0)).set_output(out.append)
    env.config.native = native
    env.config.fault_injection = fault
    env._comm = comm
    env.set_stream_time_characteristic(TimeCharacteristic.EventTime)
    if tmp_path is not None:
        env.enable_checkpointing(500)
        env.set_state_backend(FsStateBackend(str(tmp_path)))
        env.set_restart_strategy(RestartStrategies.fixed_delay_restart(2, 0))
    return env, out


def _side(env, events, bound=100, timed=False):
    """(key, value, timestamp[, arrival time]) events -> a stream of Tuple2(key, value) with
    event time. `timed`: every event arrives at its arrival time (its timestamp + 10 ms unless
    given), so watermarks advance between micro-batches."""
    from mxstream.api.time import Time
    from mxstream.api.watermarks import BoundedOutOfOrdernessTimestampExtractor

    src = (env.from_timed_collection([(e[3] if len(e) > 3 else e[2] + 10, e) for e in events])
           if timed
           else env.from_collection(events))
    return (src.assign_timestamps_and_watermarks(
        BoundedOutOfOrdernessTimestampExtractor(Time.milliseconds(bound), extractor=lambda e: e[2]))
        .map(lambda e: Tuple2(e[0], e[1])))


def _tumbling(ms):
    from mxstream.api.time import Time
    from mxstream.api.windowing import TumblingEventTimeWindows

    return TumblingEventTimeWindows.of(Time.milliseconds(ms))


def _sliding(size, slide):
    from mxstream.api.time import Time
    from mxstream.api.windowing import SlidingEventTimeWindows

    return SlidingEventTimeWindows.of(Time.milliseconds(size), Time.milliseconds(slide))


def _rows(lines):
    return [ln[ln.index("("):] for ln in lines]


@pytest.fixture
def route(monkeypatch):
    """Spies: the join engines built (the native route) and the fallbacks taken."""
    from mxstream.runtime.join_window_operator import KeyedJoinWindowOperator
    from mxstream.runtime.native_ops import NativeJoinOp

    seen = {"built": 0, "fallback": 0, "lowered": 0}
    init, to_fb, op_init = (KeyedJoinWindowOperator.__init__, NativeJoinOp._to_fallback,
                            NativeJoinOp.__init__)

    def spy_init(self, *a, **kw):
        seen["built"] += 1
        init(self, *a, **kw)

    def spy_fb(self):
        seen["fallback"] += 1
        to_fb(self)

    def spy_op(self, *a, **kw):
        seen["lowered"] += 1
        op_init(self, *a, **kw)

    monkeypatch.setattr(KeyedJoinWindowOperator, "__init__", spy_init)
    monkeypatch.setattr(NativeJoinOp, "_to_fallback", spy_fb)
    monkeypatch.setattr(NativeJoinOp, "__init__", spy_op)
    return seen


# ---- 1. golden ---------------------------------------------------------------------------------
GOLD_L = [("h1", 90.0, 1000), ("h1", 95.0, 2000), ("h2", 10.0, 1500)]
GOLD_R = [("h1", 5, 1200), ("h1", 7, 2500), ("h3", 1, 1000)]


def _golden(native, fn=PROJECT, co_group=False):
    env, out = _env(native)
    a, b = _side(env, GOLD_L, 0), _side(env, GOLD_R, 0)
    two = a.co_group(b) if co_group else a.join(b)
    two.where(0).equal_to(0).window(_tumbling(3000)).apply(fn).print()
    env.execute("golden")
    return out


def test_golden_join(route):
    host = _golden("off")
    assert _rows(host) == ["(h1,90.0,5)", "(h1,90.0,7)", "(h1,95.0,5)", "(h1,95.0,7)"]
    assert route == {"built": 0, "fallback": 0, "lowered": 0}
    native = _golden("auto")
    assert route == {"built": 1, "fallback": 0, "lowered": 1}
    assert Counter(native) == Counter(host)  # the right column prints as a long
    # the other ways to write the same function
    from mxstream.api.functions import FlatJoinFunction, JoinFunction

    class J(JoinFunction):
        def join(self, l, r):
            return Tuple3(l.f0, l.f1, r.f1)

    class FJ(FlatJoinFunction):
        def join(self, l, r, out):
            out.collect(Tuple3(l.f0, l.f1, r.f1))
            out.collect(Tuple3(l.f0, l.f1, r.f1))

    assert _golden("off", J()) == host and Counter(_golden("auto", J())) == Counter(host)
    assert route["built"] == 2
    assert _golden("auto", FJ()) == [ln for ln in host for _ in (0, 1)]
    assert route == {"built": 2, "fallback": 0, "lowered": 2}  # a flat join: host operators


# ---- 9. co_group -------------------------------------------------------------------------------
def test_co_group_outer_join_shape(route):
    def left_outer(lefts, rights, out):
        for l in lefts:
            if not rights:
                out.collect(Tuple3(l.f0, l.f1, -1))
            for r in rights:
                out.collect(Tuple3(l.f0, l.f1, r.f1))

    for native in ("off", "auto"):
        got = _rows(_golden(native, left_outer, co_group=True))
        assert Counter(got) == Counter(["(h1,90.0,5)", "(h1,90.0,7)", "(h1,95.0,5)",
                                        "(h1,95.0,7)", "(h2,10.0,-1)"])
        assert [g for g in got if "h1" in g] == ["(h1,90.0,5)", "(h1,90.0,7)", "(h1,95.0,5)",
                                                 "(h1,95.0,7)"]
    assert route == {"built": 0, "fallback": 0, "lowered": 0}

    from mxstream.api.functions import CoGroupFunction

    class Sizes(CoGroupFunction):
        def co_group(self, lefts, rights, out):
            out.collect(Tuple2(len(lefts), len(rights)))

    assert Counter(_rows(_golden("auto", Sizes(), co_group=True))) == \
        Counter(["(2,2)", "(1,0)", "(0,1)"])


# ---- 7. API job: native equals host -------------------------------------------------------------
def _value(i, kind, salt):
    return float(i % 13) * 1.5 + salt if kind == "float" else (i * 7 + int(salt * 4)) % 23


def _events(kinds=("float", "float")):
    left = [(f"host{i % 7}", _value(i, kinds[0], 0.25), i * 40) for i in range(400)]
    right = [(f"host{j % 7 + 2}", _value(j, kinds[1], 1), j * 53 + 7) for j in range(300)]
    return left, right


def _job(kinds=("float", "float"), native="auto", fn=PROJECT, where=0, equal_to=0, stage=None,
         events=None, timed=False, **env_kw):
    env, out = _env(native, **env_kw)
    left, right = events or _events(kinds)
    timed = timed or env_kw.get("tmp_path") is not None
    a, b = _side(env, left, timed=timed), _side(env, right, timed=timed)
    w = a.join(b).where(where).equal_to(equal_to).window(_sliding(3000, 1000))
    if stage is not None:
        w = stage(w)
    w.apply(fn).print()
    res = env.execute("join-job")
    return out, res


def _brute_count(left, right, size=3000, slide=1000):
    """Rows of the sliding-window join from the event lists alone (in-order streams: no element
    is late): pairs of one key, counted once per window that contains both."""
    n = 0
    for lk, _lv, lt in left:
        for rk, _rv, rt in right:
            if lk != rk:
                continue
            lo = max(lt, rt) - size + 1           # window starts s with s <= min, s + size > max
            hi = min(lt, rt)
            n += max(0, hi // slide - (lo + slide - 1) // slide + 1)
    return n


@pytest.mark.parametrize("kinds", [("float", "float"), ("float", "int"), ("int", "int")])
def test_api_job_native_equals_host(route, kinds):
    host, _ = _job(kinds, native="off")
    assert route == {"built": 0, "fallback": 0, "lowered": 0}
    got, res = _job(kinds)
    assert route == {"built": 1, "fallback": 0, "lowered": 1}
    assert Counter(got) == Counter(host)
    assert len(got) == _brute_count(*_events(kinds)) > 1000
    assert not any(re.search(r"host[0178]\b", ln) for ln in got)
    num = {"float": r"-?\d+\.\d+", "int": r"-?\d+"}
    pat = rf"(\d+> )?\(host[2-6],{num[kinds[0]]},{num[kinds[1]]}\)"
    assert all(re.fullmatch(pat, ln) for ln in got), got[:3]
    assert res.metrics["Window(Apply).numLateRecordsDropped"] == 0


def test_late_elements_are_dropped_on_both_sides(route):
    left, right = _events()
    left[200] = ("host3", 1.0, 10, 8010)    # 8 s behind the watermark when they arrive
    right[150] = ("host3", 2.0, 20, 7967)
    host, hres = _job(native="off", events=(left, right), timed=True)
    got, res = _job(events=(left, right), timed=True)
    assert route["built"] == 1 and Counter(got) == Counter(host)
    key = "Window(Apply).numLateRecordsDropped"
    assert res.metrics[key] == hres.metrics[key] == 2


# ---- 8. fallbacks keep the host route ------------------------------------------------------------
def _selector(v):
    return v[0]


FALLBACKS = {
    # name: (job arguments, lowered by the planner?, falls back at run time?)
    "arithmetic": (dict(fn=lambda l, r: Tuple3(l.f0, l.f1 + r.f1, r.f1)), 0, 0),
    "two_left_fields": (dict(fn=lambda l, r: Tuple3(l.f1, l.f1, l.f0)), 0, 0),
    "not_a_tuple": (dict(fn=lambda l, r: l.f1), 0, 0),
    "key_selector": (dict(where=_selector), 0, 0),
    "allowed_lateness": (dict(stage=lambda w: w.allowed_lateness(500)), 0, 0),
    "trigger": (dict(stage=lambda w: w.trigger(__import__(
        "mxstream.api.windowing", fromlist=["x"]).EventTimeTrigger.create())), 0, 0),
    "int_beyond_2_53": (dict(big=2 ** 53 + 1), 1, 1),
    "mixed_key_types": (dict(int_keys_right=True), 1, 1),
}


@pytest.mark.parametrize("case", sorted(FALLBACKS))
def test_fallbacks_keep_the_host_route_and_equal_it(route, case):
    kw, lowered, fell = FALLBACKS[case]
    kw = dict(kw)
    left, right = _events(("float", "int"))
    if kw.pop("big", None):
        right[0] = (right[0][0], 2 ** 53 + 1, right[0][2])
    if kw.pop("int_keys_right", None):
        right = [(j % 9, v, t) for j, (_k, v, t) in enumerate(right)]
    host, _ = _job(native="off", events=(left, right), **kw)
    assert route == {"built": 0, "fallback": 0, "lowered": 0}
    got, _ = _job(events=(left, right), **kw)
    assert route == {"built": 0, "fallback": fell, "lowered": lowered}
    assert got == host  # the host operators themselves: Flink's order too
    if case == "int_beyond_2_53":
        assert any(str(2 ** 53 + 1) in ln for ln in got)
    if case != "mixed_key_types":
        assert len(got) > 1000


# ---- 10. restart from a checkpoint -----------------------------------------------------------------
def test_api_job_restarts_from_checkpoint(tmp_path, route):
    clean, _ = _job(("float", "int"), tmp_path=tmp_path / "clean")
    got, res = _job(("float", "int"), tmp_path=tmp_path / "ft", fault="Window:200")
    assert res.metrics["numRestarts"] == 1
    assert res.metrics["restoredCheckpointId"] >= 1
    assert set(got) == set(clean) and len(clean) > 1000
    assert route["built"] >= 2 and route["fallback"] == 0


# ---- 11. world 2 ---------------------------------------------------------------------------------
def test_api_job_invariant_to_world(route):
    from mxstream.parallel.comm import run_loopback

    ref, _ = _job(("float", "int"))
    assert route["built"] == 1
    res = run_loopback(2, lambda comm: _job(("float", "int"), comm=comm))
    got = [line for out, _ in res for line in out]
    assert Counter(got) == Counter(ref)
    assert route["built"] == 1 and route["lowered"] == 1  # host operators on both ranks


# ---- 12. validation ------------------------------------------------------------------------------
def test_stage_order_and_positions():
    env, _ = _env()
    a, b = _side(env, GOLD_L), _side(env, GOLD_R)
    with pytest.raises(ValueError):
        a.join(b).equal_to(0)
    with pytest.raises(ValueError):
        a.join(b).window(_tumbling(1000))
    with pytest.raises(ValueError):
        a.join(b).where(0).window(_tumbling(1000))
    with pytest.raises(ValueError):
        a.co_group(b).equalTo(0)
    with pytest.raises(ValueError):
        a.join(b).where(-1)
    with pytest.raises(ValueError):
        a.join(b).where(0).equal_to(-2)
    for bad in (None, 1.5, True):
        with pytest.raises(TypeError):
            a.join(b).where(bad)
    with pytest.raises(TypeError):
        a.join(b).where(0).equalTo(0).window("1 minute")
    with pytest.raises(TypeError):
        a.join([1, 2, 3])
    with pytest.raises(ValueError):
        a.join(b).where(0).equal_to(0).window(_tumbling(1000)).allowedLateness(-1).apply(PROJECT)
    assert hasattr(a.join(b).where(0), "equalTo") and hasattr(a, "coGroup")


def test_join_projection_trace():
    from mxstream.api.planner import trace_join_projection as tr

    assert tr(PROJECT, (0, 0), 2, 2) == (("k", "l", "r"), 1, 1)
    assert tr(lambda l, r: Tuple3(r.f2, r.f0, l.f0), (1, 0), 3, 3) == (("r", "k", "l"), 0, 2)
    assert tr(lambda l, r: (l[0], r[1], l[1], r[1], r[0]), (0, 0), 2, 2) == \
        (("k", "r", "l", "r", "k"), 1, 1)
    assert tr(PROJECT, (0, 0), 1, 2) is None                                  # arity
    assert tr(lambda l, r: Tuple2(l.f0, l.f1), (0, 0), 2, 2) is None          # no right value
    assert tr(lambda l, r: Tuple3(l.f1, l.f2, r.f1), (0, 0), 3, 2) is None    # two left fields
    assert tr(lambda l, r: Tuple2(l.f0, l.f1 * r.f1), (0, 0), 2, 2) is None   # arithmetic
    assert tr(lambda l, r: Tuple2(l.f0, 1.0), (0, 0), 2, 2) is None           # a constant
    assert tr(lambda l, r: Tuple2(l.f0, r.f1) if l.f1 > 0 else None, (0, 0), 2, 2) is None


def test_tag_operator_keeps_column_batches_columnar():
    import numpy as np

    from mxstream.ops.text import FK_DOUBLE, FK_LONG
    from mxstream.runtime.columnar import ColumnBatch, TagSideOp, expand_columns
    from mxstream.runtime.operators import WM, Rec

    cb = ColumnBatch(2, [np.array([4, 5]), np.array([1.5, 2.5])], (FK_LONG, FK_DOUBLE), None,
                     np.array([10, 20]), np.array([0, 1], dtype=np.int32))
    op = TagSideOp(1, columnar=True)
    assert op.accepts_columns and not TagSideOp(0).accepts_columns
    out = op.process([cb, WM(5), Rec(Tuple2(6, 3.5), 30, 2)])
    assert isinstance(out[0], ColumnBatch) and out[0].side == 1 and cb.side is None
    assert out[0].cols is cb.cols and out[1] == WM(5)
    assert out[2] == Rec((1, Tuple2(6, 3.5)), 30, 2)
    # expanded after all (the fallback): the same tagged records
    assert expand_columns(out[:1]) == [Rec((1, Tuple2(4, 1.5)), 10, 0), Rec((1, Tuple2(5, 2.5)), 20, 1)]


def test_native_operator_takes_tagged_column_batches(route):
    """Column batches of both sides (one with its own dictionary) and records in one pass."""
    import numpy as np

    from mxstream.api.planner import trace_join_projection as tr
    from mxstream.ops.native import load
    from mxstream.ops.text import FK_DOUBLE, FK_LONG, FK_STR
    from mxstream.runtime.columnar import ColumnBatch
    from mxstream.runtime.native_ops import NativeJoinOp
    from mxstream.runtime.operators import WM, OpContext, Rec

    layout, lv, rv = tr(PROJECT, (0, 0), 2, 2)
    op = NativeJoinOp(key_pos=(0, 0), val_pos=(lv, rv), layout=layout, ok_arities=({2}, {2}),
                      assigner=_tumbling(1000), device="cpu", fallback_factory=None)
    op.open(OpContext("join", 4, 128, lambda: 0, "EventTime"))
    d1, d2 = load().StringDict(), load().StringDict()
    ids1 = np.array([d1.intern(s) for s in ("a", "b", "a")])
    d2.intern("zz")
    ids2 = np.array([d2.intern(s) for s in ("b", "a")])
    lcb = ColumnBatch(3, [ids1, np.array([1.0, 2.0, 3.0])], (FK_STR, FK_DOUBLE), d1,
                      np.array([100, 200, 300]), np.zeros(3, np.int32), side=0)
    rcb = ColumnBatch(2, [ids2, np.array([7, 8])], (FK_STR, FK_LONG), d2,
                      np.array([150, 250]), np.zeros(2, np.int32), side=1)
    out = op.process([lcb, rcb, Rec((1, Tuple2("a", 9)), 400, 0), WM(2000)])
    assert route["built"] == 1 and isinstance(out[0], ColumnBatch) and out[-1] == WM(2000)
    rows = Counter(str(r.value) for r in out[0].to_recs())
    assert rows == Counter(["(a,1.0,8)", "(a,1.0,9)", "(a,3.0,8)", "(a,3.0,9)", "(b,2.0,7)"])
    assert set(out[0].ts.tolist()) == {999} and out[0].kinds == (FK_STR, FK_DOUBLE, FK_LONG)
    # the operator's own dictionary: nothing was interned into the parsers' ones
    assert d1.strings() == ["a", "b"] and d2.strings() == ["zz", "b", "a"]
    assert out[0].strings is op.dict and op.dict is not d1
    assert sorted(op.dict.strings()) == ["a", "b", "zz"]
    with pytest.raises(TypeError):  # native state exists: no way back to the host operator
        op.process([Rec((0, Tuple2(5, 1.0)), 2500, 0), WM(3000)])


def test_fallback_in_the_middle_of_a_pass_takes_the_rest_of_it(route):
    """A flush that switches to the host operator hands it the watermark seen so far, the
    records it held and everything that follows in the pass; nothing stays pending."""
    from mxstream.api.planner import trace_join_projection as tr
    from mxstream.runtime.native_ops import NativeJoinOp
    from mxstream.runtime.operators import WM, OpContext, Operator, Rec

    seen = []

    class Host(Operator):
        num_late_records_dropped = 0

        def process(self, items):
            seen.extend(items)
            return [it for it in items if isinstance(it, WM)]

    layout, lv, rv = tr(PROJECT, (0, 0), 2, 2)
    op = NativeJoinOp(key_pos=(0, 0), val_pos=(lv, rv), layout=layout, ok_arities=({2}, {2}),
                      assigner=_tumbling(1000), device="cpu", fallback_factory=Host)
    op.open(OpContext("join", 4, 128, lambda: 0, "EventTime"))
    bad = Rec((0, Tuple2("a", "not a number")), 200, 0)
    good = Rec((1, Tuple2("a", 1)), 400, 0)
    out = op.process([WM(100), bad, WM(300), good, WM(500)])
    assert out == [WM(100), WM(300), WM(500)]
    assert seen == [WM(100), bad, WM(300), good, WM(500)]
    assert route == {"built": 0, "fallback": 1, "lowered": 1} and not op.pending and op.op is None
    assert op.process([good]) == [] and seen[-1] is good and not op.pending


@pytest.mark.gpu
def test_gpu_native_operator_reads_device_batches_in_place(gpu_device, route):
    """Device column batches (integer keys) of both sides go to the arenas as they are once the
    engine exists; the first pass (no engine yet) and records go through the host columns."""
    import numpy as np
    import torch

    from mxstream.api.planner import trace_join_projection as tr
    from mxstream.ops.text import FK_DOUBLE, FK_LONG
    from mxstream.runtime.columnar import ColumnBatch, DeviceColumnBatch, TagSideOp
    from mxstream.runtime.native_ops import NativeJoinOp
    from mxstream.runtime.operators import WM, OpContext, Rec

    layout, lv, rv = tr(PROJECT, (0, 0), 2, 2)
    op = NativeJoinOp(key_pos=(0, 0), val_pos=(lv, rv), layout=layout, ok_arities=({2}, {2}),
                      assigner=_tumbling(1000), device=str(gpu_device), fallback_factory=None)
    op.open(OpContext("join", 4, 128, lambda: 0, "EventTime"))
    tags = [TagSideOp(0, True), TagSideOp(1, True)]

    def batch(side, keys, vals, ts, kind):
        dt = torch.float64 if kind == FK_DOUBLE else torch.int64
        cb = DeviceColumnBatch(len(keys), [torch.tensor(keys, device=gpu_device),
                                           torch.tensor(vals, dtype=dt, device=gpu_device)],
                               (FK_LONG, kind), None, torch.tensor(ts, device=gpu_device))
        return tags[side].process([cb])[0]

    out = op.process([batch(0, [1, 2], [1.5, 2.5], [100, 200], FK_DOUBLE),
                      batch(1, [2, 2], [7, 8], [150, 250], FK_LONG), WM(999)])
    assert route["built"] == 1
    rows = Counter(str(r.value) for cb in out if isinstance(cb, ColumnBatch) for r in cb.to_recs())
    assert rows == Counter(["(2,2.5,7)", "(2,2.5,8)"])
    calls = []
    host = DeviceColumnBatch.host
    DeviceColumnBatch.host = lambda self: (calls.append(1), host(self))[1]
    try:
        out = op.process([batch(0, [1, 2, 1], [1.0, 2.0, 3.0], [1100, 1200, 1300], FK_DOUBLE),
                          batch(1, [1, 3], [4, 5], [1150, 1250], FK_LONG),
                          Rec((1, Tuple2(1, 6)), 1400, 0), WM(1999)])
    finally:
        DeviceColumnBatch.host = host
    assert not calls and route["built"] == 1
    (cb,) = [o for o in out if isinstance(o, ColumnBatch)]
    assert Counter(str(r.value) for r in cb.to_recs()) == \
        Counter(["(1,1.0,4)", "(1,1.0,6)", "(1,3.0,4)", "(1,3.0,6)"])
    assert set(np.asarray(cb.ts).tolist()) == {1999} and cb.kinds == (FK_LONG, FK_DOUBLE, FK_LONG)
    with pytest.raises(TypeError):  # an integer beyond 2**53 after native state exists
        op.process([batch(1, [1], [2 ** 53 + 1], [2100], FK_LONG), WM(2999)])

    # string keys of a device dictionary: translated to the operator's ids on the device
    from mxstream.ops.ingest import DeviceDict
    from mxstream.ops.text import FK_STR

    sop = NativeJoinOp(key_pos=(0, 0), val_pos=(lv, rv), layout=layout, ok_arities=({2}, {2}),
                       assigner=_tumbling(1000), device=str(gpu_device), fallback_factory=None)
    sop.open(OpContext("join", 4, 128, lambda: 0, "EventTime"))
    sop.process([Rec((0, Tuple2("a", 1.0)), 100, 0), Rec((1, Tuple2("a", 2)), 200, 0), WM(999)])
    dd = DeviceDict(str(gpu_device))
    ids = dd.intern_many(["b", "a", "c"]).tolist()

    def sbatch(side, names, vals, ts, kind):
        dt = torch.float64 if kind == FK_DOUBLE else torch.int64
        keys = torch.tensor([ids["bac".index(x)] for x in names], dtype=torch.int32,
                            device=gpu_device)
        cb = DeviceColumnBatch(len(names), [keys, torch.tensor(vals, dtype=dt, device=gpu_device)],
                               (FK_STR, kind), dd, torch.tensor(ts, device=gpu_device))
        return tags[side].process([cb])[0]

    out = sop.process([sbatch(0, "abc", [1.0, 2.0, 3.0], [1100, 1200, 1300], FK_DOUBLE),
                       sbatch(1, "ba", [4, 5], [1150, 1250], FK_LONG), WM(1999)])
    (cb,) = [o for o in out if isinstance(o, ColumnBatch)]
    assert Counter(str(r.value) for r in cb.to_recs()) == Counter(["(a,1.0,5)", "(b,2.0,4)"])
    assert len(dd) == 3 and sorted(sop.dict.strings()) == ["a", "b", "c"]
