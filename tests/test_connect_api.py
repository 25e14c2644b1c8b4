"""``a.connect(b)`` (api/connect.py): co-map, co-flat-map and co-process on the host operators
(runtime/operators.py CoMapOp / CoFlatMapOp / CoProcessOp), keyed connected streams with shared
state and timers, and ``LookupLatest`` on the native lookup operator against the host path.
Outputs compare as lists: the native path keeps the per-record order."""
from __future__ import annotations

import pytest

from mxstream.api import functions as F
from mxstream.api.state import ValueStateDescriptor
from mxstream.api.tuples import Tuple2, Tuple3


def _env(native="auto", parallelism=4, device="cpu"):
    from mxstream.api.environment import StreamExecutionEnvironment
    from mxstream.api.time import TimeCharacteristic
    from mxstream.runtime.executor import ManualClock

    out = []
    env = StreamExecutionEnvironment(parallelism, clock=ManualClock(0)).set_output(out.append)
    env.config.native = native
    env.config.device = device
    env.set_stream_time_characteristic(TimeCharacteristic.EventTime)
    return env, out


def _stream(env, events, ts_field, bound=0):
    """Events arrive in event-time order across both inputs (arrival = timestamp + 10)."""
    from mxstream.api.time import Time
    from mxstream.api.watermarks import BoundedOutOfOrdernessTimestampExtractor

    return env.from_timed_collection([(e[ts_field] + 10, e) for e in events]) \
        .assign_timestamps_and_watermarks(BoundedOutOfOrdernessTimestampExtractor(
            Time.milliseconds(bound), extractor=lambda e: e[ts_field]))


class Stamp(F.ProcessFunction):
    """(value, timestamp) of every element."""

    def process_element(self, value, ctx, out):
        out.collect((value, ctx.timestamp()))


A = [("a", 1, 100), ("b", 2, 300), ("a", 3, 500)]
B = [("a", 10.0, 200), ("c", 20.0, 400)]


# ---- co-map, co-flat-map, co-process -------------------------------------------------------------
class Sides(F.CoMapFunction):
    def map1(self, v):
        return ("first", v[0], v[1])

    def map2(self, v):
        return ("second", v[0], v[1])


class Flat(F.CoFlatMapFunction):
    def flat_map1(self, v, out):
        for _ in range(v[1]):
            out.collect(("first", v[0]))

    def flat_map2(self, v, out):
        pass  # input 2 emits nothing


class Proc(F.CoProcessFunction):
    def process_element1(self, v, ctx, out):
        out.collect(("p1", v[0], ctx.timestamp()))

    def process_element2(self, v, ctx, out):
        out.collect(("p2", v[0], ctx.timestamp()))


def test_map_flat_map_and_process_dispatch_on_the_side_and_keep_timestamps():
    def run(stage):
        env, _ = _env()
        got = stage(_stream(env, A, 2).connect(_stream(env, B, 2))).process(Stamp()).collect()
        env.execute("co")
        return got

    assert run(lambda c: c.map(Sides())) == [
        (("first", "a", 1), 100), (("second", "a", 10.0), 200), (("first", "b", 2), 300),
        (("second", "c", 20.0), 400), (("first", "a", 3), 500)]
    assert run(lambda c: c.flatMap(Flat())) == [
        (("first", "a"), 100), (("first", "b"), 300), (("first", "b"), 300),
        (("first", "a"), 500), (("first", "a"), 500), (("first", "a"), 500)]
    assert run(lambda c: c.process(Proc())) == [
        (("p1", "a", 100), 100), (("p2", "a", 200), 200), (("p1", "b", 300), 300),
        (("p2", "c", 400), 400), (("p1", "a", 500), 500)]


def test_process_without_timestamps_sees_none():
    env, _ = _env()
    got = env.from_collection([("a", 1)]).connect(env.from_collection([("b", 2)])) \
        .process(Proc()).collect()
    env.execute("co")
    assert got == [("p1", "a", None), ("p2", "b", None)]


def test_stage_validation():
    env, _ = _env()
    a, b = _stream(env, A, 2), _stream(env, B, 2)
    with pytest.raises(TypeError, match="DataStream"):
        a.connect([1, 2])
    other, _ = _env()
    with pytest.raises(ValueError, match="one execution environment"):
        a.connect(_stream(other, B, 2))
    c = a.connect(b)
    assert not c.keyed and c.get_first_input() is a and c.getSecondInput() is b
    with pytest.raises(TypeError):
        c.map(lambda v: v)
    with pytest.raises(TypeError):
        c.flat_map(Sides())
    with pytest.raises(TypeError):
        c.process(Sides())
    with pytest.raises(TypeError):
        c.key_by(None, 0)
    with pytest.raises(ValueError):
        c.key_by(0, -1)
    for bad in ("=>", "gt", 1, ""):
        with pytest.raises(ValueError, match="when must be one of"):
            F.LookupLatest(2, 1, when=bad)
    with pytest.raises(ValueError):
        F.LookupLatest(-1, 1)
    with pytest.raises(TypeError):
        F.LookupLatest(2, 1, default=True)
    assert F.CoProcessFunction.processElement1 and F.CoFlatMapFunction.flatMap2


# ---- keyed connected streams: shared state -----------------------------------------------------
class Remember(F.CoProcessFunction):
    """Input 2 stores its value; input 1 emits (key, own value, stored value or None)."""

    def open(self, parameters=None):
        self.state = self.get_runtime_context().get_state(ValueStateDescriptor("seen"))

    def process_element1(self, v, ctx, out):
        out.collect(Tuple3(v[0], v[1], self.state.value()))

    def process_element2(self, v, ctx, out):
        self.state.update(v[1])


class First(F.KeySelector):
    def get_key(self, v):
        return v[0]


@pytest.mark.parametrize("how", ["positions", "selectors", "expressions", "keyed_inputs"])
def test_state_of_input_2_is_read_by_input_1_of_the_same_key_only(how):
    env, _ = _env()
    a = _stream(env, A, 2).map(lambda e: Tuple3(*e))
    b = _stream(env, B, 2).map(lambda e: Tuple3(*e))
    if how == "keyed_inputs":  # Flink's rule: two keyed streams connect keyed
        c = a.key_by(0).connect(b.key_by(lambda v: v[0]))
    else:
        c = a.connect(b)
        assert not c.keyed
        c = {"positions": lambda: c.key_by(0, 0), "expressions": lambda: c.keyBy("f0", "f0"),
             "selectors": lambda: c.key_by(First(), lambda v: v[0])}[how]()
    assert c.keyed
    got = c.process(Remember()).collect()
    env.execute("keyed")
    # a@100 before any rule; b never has one (c's rule is another key's); a@500 reads a's rule
    assert got == [Tuple3("a", 1, None), Tuple3("b", 2, None), Tuple3("a", 3, 10.0)]


class KeyedEcho(F.KeyedProcessFunction):
    def process_element(self, e, ctx, out):
        out.collect(Tuple3(e[0], e[1], 1))


def test_prefixes_at_parallelism_4_equal_key_by():
    keys = [f"host{i}" for i in range(12)]
    samples = [(k, 5, 100 + i) for i, k in enumerate(keys)]
    rules = [(k, 1, i) for i, k in enumerate(keys)]
    env, out = _env()
    _stream(env, samples, 2).connect(_stream(env, rules, 2)).key_by(0, 0) \
        .process(Remember()).print()
    env.execute("prefixes")
    env2, want = _env()
    _stream(env2, samples, 2).key_by(0).process(KeyedEcho()).print()
    env2.execute("key_by")
    assert out == want and len({ln[0] for ln in out}) > 1


# ---- timers ------------------------------------------------------------------------------------
class Timers(F.CoProcessFunction):
    """Every element registers an event timer `delay` after its timestamp and says so."""

    def __init__(self, delay=150):
        self.delay = delay

    def process_element1(self, v, ctx, out):
        ctx.timer_service().register_event_time_timer(ctx.timestamp() + self.delay)
        out.collect(("in1", v[0], ctx.timer_service().current_watermark()))

    def process_element2(self, v, ctx, out):
        ctx.timerService().registerEventTimeTimer(ctx.timestamp() + self.delay)
        out.collect(("in2", v[0]))

    def on_timer(self, timestamp, ctx, out):
        assert ctx.timestamp() == timestamp and ctx.time_domain == "EVENT_TIME"
        out.collect(("timer", timestamp))


def test_event_timers_fire_at_the_minimum_watermark_stamped_with_the_timer():
    env, _ = _env()
    # input 1 runs ahead (timestamps to 900 by arrival 40), input 2 lags behind
    a = env.from_timed_collection([(10, ("a", 100)), (20, ("a", 500)), (40, ("a", 900))])
    b = env.from_timed_collection([(100, ("a", 200)), (200, ("a", 400)), (300, ("a", 1000))])
    from mxstream.api.time import Time
    from mxstream.api.watermarks import BoundedOutOfOrdernessTimestampExtractor as Ex

    ex = lambda: Ex(Time.milliseconds(0), extractor=lambda e: e[1])  # noqa: E731
    a, b = a.assign_timestamps_and_watermarks(ex()), b.assign_timestamps_and_watermarks(ex())
    got = a.connect(b).key_by(0, 0).process(Timers()).process(Stamp()).collect()
    env.execute("timers")
    marks = [(v[0], v[1]) if v[0] != "timer" else ("timer", v[1], ts) for v, ts in got]
    assert marks == [
        ("in1", "a"), ("in1", "a"), ("in1", "a"),      # no timer yet: input 2 has no watermark
        ("in2", "a"),                                  # min watermark 200: nothing is due
        ("in2", "a"), ("timer", 250, 250), ("timer", 350, 350),   # min watermark 400
        ("in2", "a"), ("timer", 550, 550), ("timer", 650, 650),   # min watermark 900
        ("timer", 1050, 1050), ("timer", 1150, 1150)]  # left at the end of input: they fire
    # the watermark an element of input 1 sees is the merged one
    assert [v[2] for v, _ in got if v[0] == "in1"] == [-(1 << 63)] * 3


class ProcTimer(F.CoProcessFunction):
    def process_element1(self, v, ctx, out):
        ctx.timer_service().register_processing_time_timer(50)

    def process_element2(self, v, ctx, out):
        pass

    def on_timer(self, timestamp, ctx, out):
        out.collect(("proc", timestamp, ctx.time_domain))


def _open(op):
    from mxstream.runtime.operators import OpContext

    op.open(OpContext("co", 4, 128, lambda: 0, "EventTime"))
    return op


def test_processing_timers_fire_in_on_processing_time():
    from mxstream.runtime.operators import CoProcessOp, Rec

    op = _open(CoProcessOp(lambda tv: tv[1][0], ProcTimer()))
    assert op.process([Rec((0, ("a", 1)), 10, 0)]) == []
    assert op.on_processing_time(49) == []
    out = op.on_processing_time(50)
    assert [(r.value, r.ts) for r in out] == [(("proc", 50, "PROCESSING_TIME"), 50)]
    assert out[0].subtask == op.subtask_of("a") and op.on_processing_time(99) == []


def test_non_keyed_timers_and_state_raise():
    env, _ = _env()
    a, b = _stream(env, A, 2), _stream(env, B, 2)
    a.connect(b).process(Timers()).collect()
    with pytest.raises(RuntimeError, match="Setting timers is only supported on a keyed streams"):
        env.execute("no-timers")
    env, _ = _env()
    _stream(env, A, 2).connect(_stream(env, B, 2)).process(Remember()).collect()
    with pytest.raises(RuntimeError, match="Keyed state is only available on a KeyedStream"):
        env.execute("no-state")


def test_late_elements_are_not_dropped():
    from mxstream.runtime.operators import WM, CoProcessOp, Rec

    op = _open(CoProcessOp(lambda tv: tv[1][0], Remember()))
    out = op.process([WM(1000), Rec((1, ("a", 7)), 5, 0), Rec((0, ("a", 1)), 6, 0)])
    assert [it.value for it in out if isinstance(it, Rec)] == [Tuple3("a", 1, 7)]


class Both(F.CoProcessFunction):
    """State, timers and the watermark in one function (the checkpoint test)."""

    def open(self, parameters=None):
        self.state = self.get_runtime_context().get_state(ValueStateDescriptor("last"))

    def process_element1(self, v, ctx, out):
        ctx.timer_service().register_event_time_timer(ctx.timestamp() + 25)
        out.collect((v[0], v[1], self.state.value(), ctx.timer_service().current_watermark()))

    def process_element2(self, v, ctx, out):
        self.state.update(v[1])
        ctx.timer_service().register_event_time_timer(ctx.timestamp() + 40)

    def on_timer(self, timestamp, ctx, out):
        out.collect(("timer", timestamp, self.state.value()))


def test_checkpoint_in_mid_stream_restores_state_timers_and_watermark():
    from mxstream.runtime.operators import WM, CoProcessOp, Rec

    def items(lo, hi):
        out = []
        for t in range(lo, hi, 10):
            out.append(Rec(((t // 10) % 2, (f"k{t % 3}", t)), t, 0))
            if t % 30 == 0:
                out.append(WM(t - 15))
        return out

    def flat(out):
        return [it if isinstance(it, WM) else (it.value, it.ts, it.subtask) for it in out]

    make = lambda: _open(CoProcessOp(lambda tv: tv[1][0], Both()))  # noqa: E731
    ref = make()
    first, second = flat(ref.process(items(0, 200))), flat(ref.process(items(200, 400)))
    tail = flat(ref.process([WM((1 << 63) - 1)]))
    assert any(isinstance(x, tuple) and x[0][0] == "timer" for x in tail)  # timers left: they fire
    op = make()
    assert flat(op.process(items(0, 200))) == first
    snap = op.snapshot()
    assert snap["wm"] == 165 and snap["timers"]["event"] and snap["keyed"]
    op = make()
    op.restore(snap)
    assert flat(op.process(items(200, 400))) == second
    assert flat(op.process([WM((1 << 63) - 1)])) == tail


# ---- the monitoring job: a per-host threshold that changes while the job runs ------------------
SAMPLES = [(f"host{i % 5}", "cpu", float((i * 37) % 100), i * 10) for i in range(300)]
RULES = [(f"host{i % 4}", 50.0 + 2 * i, i * 150 + 5) for i in range(20)]   # host4: never a rule


class HostLookup(F.LookupLatest):
    """A subclass keeps the host path: the planner lowers exactly LookupLatest."""


def _job(fn, native="auto", device="cpu", int_vals=False):
    env, out = _env(native, device=device)
    conv = int if int_vals else float
    s = _stream(env, SAMPLES, 3).map(lambda e: Tuple3(e[0], e[1], conv(e[2])))
    r = _stream(env, RULES, 2).map(lambda e: Tuple2(e[0], conv(e[1])))
    s.connect(r).key_by(0, 0).process(fn).print()
    env.execute("thresholds")
    return out


def _expected(when, default, int_vals=False):
    import operator

    cmp = {None: lambda a, b: True, ">": operator.gt, "<=": operator.le}[when]
    conv = int if int_vals else float
    events = sorted([(e[3], 0, e) for e in SAMPLES] + [(e[2], 1, e) for e in RULES])
    state, rows = {}, []
    for _, side, e in events:
        if side == 1:
            state[e[0]] = conv(e[1])
            continue
        t = state.get(e[0], default)
        if t is not None and cmp(conv(e[2]), t):
            rows.append(f"({e[0]},{conv(e[2])},{t})")
    return rows


@pytest.fixture
def route(monkeypatch):
    from mxstream.runtime.lookup_operator import KeyedLookupOperator
    from mxstream.runtime.native_ops import NativeLookupOp

    seen = {"built": 0, "fallback": 0}
    init, to_fb = KeyedLookupOperator.__init__, NativeLookupOp._to_fallback

    def spy_init(self, *a, **kw):
        seen["built"] += 1
        init(self, *a, **kw)

    def spy_fb(self):
        seen["fallback"] += 1
        to_fb(self)

    monkeypatch.setattr(KeyedLookupOperator, "__init__", spy_init)
    monkeypatch.setattr(NativeLookupOp, "_to_fallback", spy_fb)
    return seen


@pytest.mark.parametrize("int_vals", [False, True], ids=["float", "int"])
@pytest.mark.parametrize("when,default", [(">", None), ("<=", 60.0), (None, 1.0), (None, None)])
def test_threshold_job_native_on_cpu_equals_the_host_path(route, when, default, int_vals):
    if default is not None and int_vals:
        default = int(default)
    want = _expected(when, default, int_vals)
    host = _job(HostLookup(2, 1, when=when, default=default), int_vals=int_vals)
    assert route == {"built": 0, "fallback": 0}
    assert [ln[ln.index("("):] for ln in host] == want and len(want) > 40
    assert _job(F.LookupLatest(2, 1, when=when, default=default), "off", int_vals=int_vals) == host
    assert route == {"built": 0, "fallback": 0}
    native = _job(F.LookupLatest(2, 1, when=when, default=default), int_vals=int_vals)
    assert route == {"built": 1, "fallback": 0}
    assert native == host and len({ln[0] for ln in native}) > 1   # lists: the same order


def test_threshold_job_quick_start_lines():
    got = _job(F.LookupLatest(2, 1, when=">"))
    # host0's threshold is 50.0 from t = 5; host1 gets 52.0 at t = 155; host4 never has one
    assert got[:3] == ["1> (host0,85.0,50.0)", "1> (host0,70.0,50.0)", "1> (host0,55.0,50.0)"]
    assert got[3] == "4> (host1,92.0,52.0)" and not any("host4" in ln for ln in got)


def test_selector_keys_keep_the_host_operator(route):
    env, out = _env()
    s = _stream(env, SAMPLES, 3).map(lambda e: Tuple3(e[0], e[1], e[2]))
    r = _stream(env, RULES, 2).map(lambda e: Tuple2(e[0], e[1]))
    s.connect(r).key_by(First(), 0).process(F.LookupLatest(2, 1, when=">")).print()
    env.execute("selector")
    assert route == {"built": 0, "fallback": 0}
    assert out == _job(HostLookup(2, 1, when=">"))


@pytest.mark.gpu
@pytest.mark.parametrize("when,default", [(">", None), (None, 1.0)])
def test_gpu_threshold_job_equals_the_host_path(gpu_device, route, when, default):
    host = _job(HostLookup(2, 1, when=when, default=default))
    got = _job(F.LookupLatest(2, 1, when=when, default=default), device="cuda")
    assert route == {"built": 1, "fallback": 0}
    assert got == host and len(got) > 40
