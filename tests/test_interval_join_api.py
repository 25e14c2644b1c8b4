"""``a.key_by(k).interval_join(b.key_by(k)).between(lo, hi).process(fn)`` (api/joins.py): the host
plan is Flink's (tag, union, keyed IntervalJoinOp); the planner lowers a projection join with
positional keys onto NativeIntervalJoinOp. Outputs compare as multisets."""
from __future__ import annotations

import re
from collections import Counter

import pytest

from mxstream.api.functions import ProcessJoinFunction
from mxstream.api.tuples import Tuple2, Tuple3

PROJECT = lambda l, r: Tuple3(l.f0, l.f1, r.f1)  # noqa: E731


class Project(ProcessJoinFunction):
    def process_element(self, left, right, ctx, out):
        out.collect(Tuple3(left.f0, left.f1, right.f1))


def _env(native="auto", tmp_path=None, fault=None, comm=None, event_time=True):
    from mxstream.api.environment import (FsStateBackend, RestartStrategies,
                                          StreamExecutionEnvironment)
    from mxstream.api.time import TimeCharacteristic
    from mxstream.runtime.executor import ManualClock

    out = []
    env = StreamExecutionEnvironment(4, clock=ManualClock(0)).set_output(out.append)
    env.config.native = native
    env.config.fault_injection = fault
    env._comm = comm
    if event_time:
        env.set_stream_time_characteristic(TimeCharacteristic.EventTime)
    if tmp_path is not None:
        env.enable_checkpointing(500)
        env.set_state_backend(FsStateBackend(str(tmp_path)))
        env.set_restart_strategy(RestartStrategies.fixed_delay_restart(2, 0))
    return env, out


def _side(env, events, bound=100, timed=False):
    """(key, value, timestamp[, arrival time]) events -> Tuple2(key, value) with event time."""
    from mxstream.api.time import Time
    from mxstream.api.watermarks import BoundedOutOfOrdernessTimestampExtractor

    src = (env.from_timed_collection([(e[3] if len(e) > 3 else e[2] + 10, e) for e in events])
           if timed else env.from_collection(events))
    return (src.assign_timestamps_and_watermarks(
        BoundedOutOfOrdernessTimestampExtractor(Time.milliseconds(bound), extractor=lambda e: e[2]))
        .map(lambda e: Tuple2(e[0], e[1])))


@pytest.fixture
def route(monkeypatch):
    """Spies: the engines built (the native route), the fallbacks taken, the lowerings."""
    from mxstream.runtime.interval_join_operator import KeyedIntervalJoinOperator
    from mxstream.runtime.native_ops import NativeIntervalJoinOp

    seen = {"built": 0, "fallback": 0, "lowered": 0}
    init, to_fb, op_init = (KeyedIntervalJoinOperator.__init__, NativeIntervalJoinOp._to_fallback,
                            NativeIntervalJoinOp.__init__)

    def spy_init(self, *a, **kw):
        seen["built"] += 1
        init(self, *a, **kw)

    def spy_fb(self):
        seen["fallback"] += 1
        to_fb(self)

    def spy_op(self, *a, **kw):
        seen["lowered"] += 1
        op_init(self, *a, **kw)

    monkeypatch.setattr(KeyedIntervalJoinOperator, "__init__", spy_init)
    monkeypatch.setattr(NativeIntervalJoinOp, "_to_fallback", spy_fb)
    monkeypatch.setattr(NativeIntervalJoinOp, "__init__", spy_op)
    return seen


def _rows(lines):
    return [ln[ln.index("("):] for ln in lines]


# ---- golden ------------------------------------------------------------------------------------
GOLD_L = [("h1", 90.0, 1000), ("h1", 95.0, 2000), ("h2", 10.0, 1500)]
GOLD_R = [("h1", 5, 1200), ("h1", 7, 2500), ("h1", 9, 2501), ("h3", 1, 1000), ("h2", 4, 1499)]


def _golden(native, fn=PROJECT, lo=0, hi=500, stage=None, ka=0, kb=0):
    from mxstream.api.time import Time

    env, out = _env(native)
    a, b = _side(env, GOLD_L, 0), _side(env, GOLD_R, 0)
    j = a.key_by(ka).interval_join(b.key_by(kb)).between(Time.milliseconds(lo), hi)
    if stage is not None:
        j = stage(j)
    j.process(fn).print()
    env.execute("golden")
    return out


def test_golden_interval_join(route):
    host = _golden("off")
    # l(h1, 1000) takes r in [1000, 1500]; l(h1, 2000) takes [2000, 2500]; h2's r is 1 ms early
    assert sorted(_rows(host)) == ["(h1,90.0,5)", "(h1,95.0,7)"]
    assert route == {"built": 0, "fallback": 0, "lowered": 0}
    for fn in (PROJECT, Project()):
        native = _golden("auto", fn)
        assert Counter(native) == Counter(host)
    assert route == {"built": 2, "fallback": 0, "lowered": 2}
    assert sorted(_rows(_golden("auto", lo=-1))) == ["(h1,90.0,5)", "(h1,95.0,7)", "(h2,10.0,4)"]
    assert sorted(_rows(_golden("auto", hi=501))) == ["(h1,90.0,5)", "(h1,95.0,7)", "(h1,95.0,9)"]
    excl = lambda j: j.lower_bound_exclusive().upperBoundExclusive()  # noqa: E731
    for native in ("off", "auto"):
        assert sorted(_rows(_golden(native, lo=-1, hi=501, stage=excl))) == \
            ["(h1,90.0,5)", "(h1,95.0,7)"]


def test_bounds_time_characteristic_and_stage_validation():
    env, _ = _env()
    a, b = _side(env, GOLD_L), _side(env, GOLD_R)
    ka, kb = a.key_by(0), b.key_by(0)
    with pytest.raises(ValueError, match="lowerBound <= upperBound must be fulfilled"):
        ka.interval_join(kb).between(5, 4)
    with pytest.raises(ValueError, match="lowerBound <= upperBound must be fulfilled"):
        ka.intervalJoin(kb).between(3, 4).lower_bound_exclusive().upper_bound_exclusive()
    ka.interval_join(kb).between(3, 4).lowerBoundExclusive()  # (4, 4) is fine
    with pytest.raises(TypeError):
        ka.interval_join(b)  # not keyed
    with pytest.raises(ValueError):
        ka.interval_join(kb).process(PROJECT)
    with pytest.raises(TypeError):
        ka.interval_join(kb).between(0, 1).process(42)
    other, _ = _env()
    with pytest.raises(ValueError, match="one execution environment"):
        ka.interval_join(_side(other, GOLD_R).key_by(0))
    penv, _ = _env(event_time=False)
    pa, pb = _side(penv, GOLD_L).key_by(0), _side(penv, GOLD_R).key_by(0)
    with pytest.raises(RuntimeError,
                       match="Time-bounded stream joins are only supported in event time"):
        pa.interval_join(pb)


# ---- API job: native equals host -----------------------------------------------------------------
def _value(i, kind, salt):
    return float(i % 13) * 1.5 + salt if kind == "float" else (i * 7 + int(salt * 4)) % 23


def _events(kinds=("float", "float"), int_keys=False):
    key = (lambda i: i % 7) if int_keys else (lambda i: f"host{i % 7}")
    left = [(key(i), _value(i, kinds[0], 0.25), i * 40) for i in range(400)]
    right = [(key(j + 2), _value(j, kinds[1], 1), j * 53 + 7) for j in range(300)]
    return left, right


LO, HI = -500, 700


def _job(kinds=("float", "float"), native="auto", fn=PROJECT, ka=0, kb=0, events=None,
         timed=False, int_keys=False, tag=None, **env_kw):
    env, out = _env(native, **env_kw)
    left, right = events or _events(kinds, int_keys)
    timed = timed or env_kw.get("tmp_path") is not None
    a, b = _side(env, left, timed=timed), _side(env, right, timed=timed)
    joined = a.key_by(ka).interval_join(b.key_by(kb)).between(LO, HI).process(fn)
    joined.print()
    if tag is not None:
        joined.get_side_output(tag).print("side")
    res = env.execute("interval-join-job")
    return out, res


def _brute_count(left, right):
    return sum(1 for lk, _lv, lt in left for rk, _rv, rt in right
               if lk == rk and lt + LO <= rt <= lt + HI)


@pytest.mark.parametrize("int_keys", [False, True], ids=["str_keys", "int_keys"])
@pytest.mark.parametrize("kinds", [("float", "float"), ("float", "int"), ("int", "int")])
def test_api_job_native_equals_host(route, kinds, int_keys):
    host, hres = _job(kinds, native="off", int_keys=int_keys)
    assert route == {"built": 0, "fallback": 0, "lowered": 0}
    got, res = _job(kinds, int_keys=int_keys)
    assert route == {"built": 1, "fallback": 0, "lowered": 1}
    assert Counter(got) == Counter(host)
    assert len(got) == _brute_count(*_events(kinds, int_keys)) > 1000  # in order: nothing is late
    num = {"float": r"-?\d+\.\d+", "int": r"-?\d+"}
    key = r"[0-6]" if int_keys else r"host[0-6]"
    pat = rf"[1-4]> \({key},{num[kinds[0]]},{num[kinds[1]]}\)"  # the N> prefixes of 4 subtasks
    assert all(re.fullmatch(pat, ln) for ln in got), got[:3]
    assert len({ln[0] for ln in got}) > 1
    name = "IntervalJoin.numLateRecordsDropped"
    assert res.metrics[name] == hres.metrics[name] == 0


def test_late_elements_are_dropped_on_both_sides(route):
    left, right = _events()
    left[200] = ("host3", 1.0, 10, 8010)    # 8 s behind the watermark when they arrive
    right[150] = ("host3", 2.0, 20, 7967)
    host, hres = _job(native="off", events=(left, right), timed=True)
    got, res = _job(events=(left, right), timed=True)
    assert route["built"] == 1 and Counter(got) == Counter(host) and len(got) > 1000
    key = "IntervalJoin.numLateRecordsDropped"
    assert res.metrics[key] == hres.metrics[key] == 2


def test_timed_job_with_clean_up_equals_host(route):
    """Watermarks advance between the micro-batches: buffers are cleaned while the job runs."""
    host, _ = _job(("float", "int"), native="off", timed=True)
    got, _ = _job(("float", "int"), timed=True)
    assert route["built"] == 1 and Counter(got) == Counter(host)
    assert len(got) == _brute_count(*_events(("float", "int")))


# ---- the host route ------------------------------------------------------------------------------
def _selector(v):
    return v[0]


class UsesCtx(ProcessJoinFunction):
    def process_element(self, left, right, ctx, out):
        out.collect(Tuple3(left.f0, left.f1, ctx.get_timestamp()))


class Twice(ProcessJoinFunction):
    def process_element(self, left, right, ctx, out):
        out.collect(Tuple3(left.f0, left.f1, right.f1))
        out.collect(Tuple3(left.f0, left.f1, right.f1))


HOST_ROUTE = {
    # name: (job arguments, lowered by the planner?, falls back at run time?)
    "key_selector": (dict(ka=_selector), 0, 0),
    "uses_ctx": (dict(fn=UsesCtx()), 0, 0),
    "two_collects": (dict(fn=Twice()), 0, 0),
    "arithmetic": (dict(fn=lambda l, r: Tuple3(l.f0, l.f1 + r.f1, r.f1)), 0, 0),
    "not_a_tuple": (dict(fn=lambda l, r: l.f1), 0, 0),
    "int_beyond_2_53": (dict(big=2 ** 53 + 1), 1, 1),
    "mixed_key_types": (dict(int_keys_right=True), 1, 1),
}


@pytest.mark.parametrize("case", sorted(HOST_ROUTE))
def test_host_route_and_fallbacks_equal_the_host_plan(route, case):
    kw, lowered, fell = HOST_ROUTE[case]
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
    assert got == host  # the host operators themselves
    if case == "int_beyond_2_53":
        assert any(str(2 ** 53 + 1) in ln for ln in got)
    if case != "mixed_key_types":
        assert len(got) > 1000


def test_ctx_timestamps_and_side_output_on_the_host_route(route):
    from mxstream.api.datastream import OutputTag

    tag = OutputTag("far")

    class Stamps(ProcessJoinFunction):
        def process_element(self, left, right, ctx, out):
            lt, rt = ctx.getLeftTimestamp(), ctx.get_right_timestamp()
            assert ctx.get_timestamp() == ctx.getTimestamp() == max(lt, rt)
            out.collect(Tuple3(left.f0, lt, rt))
            if rt - lt == 500:
                ctx.output(tag, Tuple2(left.f0, rt))

    env, out = _env()
    a, b = _side(env, GOLD_L, 0), _side(env, GOLD_R, 0)
    joined = a.key_by(0).interval_join(b.key_by(0)).between(0, 500).process(Stamps())
    joined.print()
    joined.get_side_output(tag).print("side")
    env.execute("stamps")
    assert route == {"built": 0, "fallback": 0, "lowered": 0}
    main = sorted(_rows(ln for ln in out if "side" not in ln))
    assert main == ["(h1,1000,1200)", "(h1,2000,2500)"]
    assert _rows(ln for ln in out if "side" in ln) == ["(h1,2500)"]


def test_output_records_carry_the_larger_timestamp():
    from mxstream.runtime.operators import WM, IntervalJoinOp, OpContext, Rec

    op = IntervalJoinOp(lambda tv: tv[1][0], -2, 5, lambda l, r: (l, r))
    op.open(OpContext("ij", 4, 128, lambda: 0, "EventTime"))
    assert op.process([Rec((0, ("a", 1)), 10, 0), Rec((1, ("a", 2)), 15, 0)])[0].ts == 15
    assert op.process([Rec((0, ("a", 3)), 17, 0)])[0].ts == 17  # r at 15 = 17 - 2
    # the boundary loss: watermark 15 removes l(10) (10 + 5), so r(15) only meets l(17)
    got = op.process([WM(15), Rec((1, ("a", 4)), 15, 0)])
    assert got[0] == WM(15) and [(r.value, r.ts) for r in got[1:]] == [((("a", 3), ("a", 4)), 17)]
    assert op.process([Rec((1, ("a", 5)), 14, 0)]) == [] and op.num_late_records_dropped == 1
    snap = op.snapshot()
    op2 = IntervalJoinOp(lambda tv: tv[1][0], -2, 5, lambda l, r: (l, r))
    op2.open(OpContext("ij", 4, 128, lambda: 0, "EventTime"))
    op2.restore(snap)
    for o in (op, op2):
        got = o.process([Rec((0, ("a", 6)), 16, 0), WM(17), Rec((0, ("a", 7)), 17, 0)])
        assert [(r.value, r.ts) for r in got if isinstance(r, Rec)] == \
            [((("a", 6), ("a", 2)), 16), ((("a", 6), ("a", 4)), 16)]  # r(15)s gone at 17
    with pytest.raises(ValueError):
        IntervalJoinOp(lambda tv: tv[1][0], -2, 6, lambda l, r: (l, r)).restore(snap)
    with pytest.raises(RuntimeError):
        op.process([Rec((0, ("a", 1)), -(1 << 63), 0)])


# ---- the native operator -------------------------------------------------------------------------
def _native_op(fallback=None, device="cpu"):
    from mxstream.api.planner import trace_join_projection as tr
    from mxstream.runtime.native_ops import NativeIntervalJoinOp
    from mxstream.runtime.operators import OpContext

    layout, lv, rv = tr(PROJECT, (0, 0), 2, 2)
    op = NativeIntervalJoinOp(key_pos=(0, 0), val_pos=(lv, rv), layout=layout,
                              ok_arities=({2}, {2}), lo=-100, hi=100, device=device,
                              fallback_factory=fallback)
    op.open(OpContext("ij", 4, 128, lambda: 0, "EventTime"))
    return op


def test_native_operator_runs_of_one_side_in_arrival_order(route):
    from mxstream.runtime.columnar import ColumnBatch
    from mxstream.runtime.operators import WM, Rec

    op = _native_op()
    L = lambda k, v, t: Rec((0, Tuple2(k, v)), t, 0)  # noqa: E731
    R = lambda k, v, t: Rec((1, Tuple2(k, v)), t, 0)  # noqa: E731
    out = op.process([L("a", 1.0, 100), L("b", 2.0, 100), R("a", 7, 150), L("a", 3.0, 160),
                      WM(120), R("a", 8, 250), R("b", 9, 120), L("a", 4.0, 119)])
    assert route["built"] == 1 and out.count(WM(120)) == 1
    before = out[:out.index(WM(120))]
    rows = [sorted((str(r.value), r.ts) for r in cb.to_recs()) for cb in before]
    # run L, run R (sees both lefts), run L (sees the right): one batch per non-empty run
    assert rows == [[("(a,1.0,7)", 150)], [("(a,3.0,7)", 160)]]
    after = [cb for cb in out[out.index(WM(120)) + 1:] if isinstance(cb, ColumnBatch)]
    assert sorted((str(r.value), r.ts) for cb in after for r in cb.to_recs()) == \
        [("(a,3.0,8)", 250), ("(b,2.0,9)", 120)]
    assert op.num_late_records_dropped == 1
    with pytest.raises(TypeError):  # native state exists: no way back to the host operator
        op.process([L("a", "not a number", 300)])


def test_fallback_before_native_state_takes_the_rest_of_the_pass(route):
    from mxstream.runtime.operators import WM, Operator, Rec

    seen = []

    class Host(Operator):
        num_late_records_dropped = 0

        def process(self, items):
            seen.extend(items)
            return [it for it in items if isinstance(it, WM)]

    op = _native_op(Host)
    bad = Rec((0, Tuple2("a", "not a number")), 200, 0)
    good = Rec((1, Tuple2("a", 1)), 400, 0)
    assert op.process([WM(100), bad, WM(300), good, WM(500)]) == [WM(100), WM(300), WM(500)]
    assert seen == [WM(100), bad, WM(300), good, WM(500)]
    assert route == {"built": 0, "fallback": 1, "lowered": 1} and not op.pending and op.op is None


def test_native_snapshot_restore(route):
    from mxstream.runtime.operators import WM, Rec

    op = _native_op()
    op.process([Rec((0, Tuple2("a", 1.0)), 100, 0), Rec((0, Tuple2("b", 2.0)), 130, 0), WM(90)])
    op2 = _native_op()
    op2.restore(op.snapshot())
    for o in (op, op2):
        out = o.process([Rec((1, Tuple2("b", 5)), 200, 0), Rec((1, Tuple2("a", 6)), 80, 0)])
        assert [str(r.value) for cb in out for r in cb.to_recs()] == ["(b,2.0,5)"]
        assert o.num_late_records_dropped == 1


# ---- restart from a checkpoint, several ranks ----------------------------------------------------
def test_api_job_restarts_from_checkpoint(tmp_path, route):
    clean, _ = _job(("float", "int"), tmp_path=tmp_path / "clean")
    got, res = _job(("float", "int"), tmp_path=tmp_path / "ft", fault="IntervalJoin:200")
    assert res.metrics["numRestarts"] == 1
    assert res.metrics["restoredCheckpointId"] >= 1
    assert set(got) == set(clean) and len(clean) > 1000
    assert route["built"] >= 2 and route["fallback"] == 0


def test_api_job_invariant_to_world(route):
    from mxstream.parallel.comm import run_loopback

    ref, _ = _job(("float", "int"))
    assert route["built"] == 1
    res = run_loopback(2, lambda comm: _job(("float", "int"), comm=comm))
    got = [line for out, _ in res for line in out]
    assert Counter(got) == Counter(ref)
    assert route["built"] == 1 and route["lowered"] == 1  # host operators on both ranks


@pytest.mark.gpu
def test_gpu_api_job_equals_host(gpu_device, route):
    host, _ = _job(("float", "int"), native="off")

    def run():
        env, out = _env()
        env.config.device = "cuda"
        left, right = _events(("float", "int"))
        a, b = _side(env, left), _side(env, right)
        a.key_by(0).interval_join(b.key_by(0)).between(LO, HI).process(Project()).print()
        env.execute("gpu-interval-join")
        return out

    got = run()
    assert route == {"built": 1, "fallback": 0, "lowered": 1}
    assert Counter(got) == Counter(host) and len(got) > 1000
