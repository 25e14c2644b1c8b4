"""Broadcast state (api/broadcast.py): ``rules.broadcast(descriptor)``,
``samples[.key_by(k)].connect(..).process(fn)`` on the host operator (runtime/operators.py
BroadcastProcessOp): stage validation, one copy of the state per parallel instance, prefixes,
apply_to_keyed_state, timers, the non-keyed form, checkpoints and the one-rank limit."""
from __future__ import annotations

import pytest

from mxstream.api import functions as F
from mxstream.api.state import MapStateDescriptor, ValueStateDescriptor
from mxstream.api.tuples import Tuple2, Tuple3

RULES = MapStateDescriptor("rules")
COUNT = ValueStateDescriptor("count")
P = 4


def _env(parallelism=P):
    from mxstream.api.environment import StreamExecutionEnvironment
    from mxstream.api.time import TimeCharacteristic
    from mxstream.runtime.executor import ManualClock

    out = []
    env = StreamExecutionEnvironment(parallelism, clock=ManualClock(0)).set_output(out.append)
    env.set_stream_time_characteristic(TimeCharacteristic.EventTime)
    return env, out


def _stream(env, events, ts_field):
    """Events arrive in event-time order across both inputs (arrival = timestamp + 10)."""
    from mxstream.api.time import Time
    from mxstream.api.watermarks import BoundedOutOfOrdernessTimestampExtractor

    return env.from_timed_collection([(e[ts_field] + 10, e) for e in events]) \
        .assign_timestamps_and_watermarks(BoundedOutOfOrdernessTimestampExtractor(
            Time.milliseconds(0), extractor=lambda e: e[ts_field]))


def _open(op, parallelism=P, comm=None):
    from mxstream.runtime.operators import OpContext

    op.open(OpContext("bc", parallelism, 128, lambda: 0, "EventTime", comm=comm))
    return op


class Keyed(F.KeyedBroadcastProcessFunction):
    """Broadcast side: counts its calls in the broadcast state and says so. Element side: the
    key, the value and the count it reads."""

    def process_broadcast_element(self, rule, ctx, out):
        st = ctx.get_broadcast_state(RULES)
        st.put("calls", (st.get("calls") or 0) + 1)
        out.collect(("rule", rule[0], st.get("calls")))

    def process_element(self, v, ctx, out):
        st = ctx.get_broadcast_state(RULES)
        out.collect(Tuple3(ctx.get_current_key(), v[1], st.get("calls")))


class Plain(F.BroadcastProcessFunction):
    def process_broadcast_element(self, rule, ctx, out):
        ctx.get_broadcast_state(RULES).put(rule[0], rule[1])

    def process_element(self, v, ctx, out):
        st = ctx.getBroadcastState(RULES)
        assert not hasattr(ctx, "timer_service") and not hasattr(ctx, "get_current_key")
        out.collect((v[0], sorted(st.immutable_entries()), ctx.timestamp(),
                     ctx.current_watermark()))


KEYS = [f"host{i}" for i in range(12)]
SAMPLES = [(k, 5, 100 + 10 * i) for i, k in enumerate(KEYS)]


# ---- stages --------------------------------------------------------------------------------------
def test_stage_validation():
    from mxstream.api.broadcast import BroadcastConnectedStream, BroadcastStream

    env, _ = _env()
    a, b = _stream(env, SAMPLES, 2), _stream(env, [("r", 1, 5)], 2)
    with pytest.raises(ValueError):
        b.broadcast()
    with pytest.raises(TypeError):
        b.broadcast(COUNT)
    bs = b.broadcast(RULES)
    assert isinstance(bs, BroadcastStream) and bs.getBroadcastStateDescriptors() == [RULES]
    plain, keyed = a.connect(bs), a.key_by(0).connect(bs)
    assert isinstance(plain, BroadcastConnectedStream) and not plain.keyed and keyed.keyed
    assert keyed.getFirstInput().t is a.t and keyed.get_second_input() is bs
    with pytest.raises(TypeError, match="A KeyedBroadcastProcessFunction can only be used on a "
                                        "keyed stream."):
        plain.process(Keyed())
    with pytest.raises(TypeError, match="A BroadcastProcessFunction can only be used on a "
                                        "non-keyed stream."):
        keyed.process(Plain())
    with pytest.raises(TypeError):
        keyed.process(lambda v: v)
    other, _ = _env()
    with pytest.raises(ValueError, match="one execution environment"):
        _stream(other, SAMPLES, 2).connect(bs)
    assert F.KeyedBroadcastProcessFunction.processBroadcastElement \
        and F.KeyedBroadcastProcessFunction.onTimer and F.BroadcastProcessFunction.processElement
    assert not issubclass(F.KeyedBroadcastProcessFunction, F.BroadcastProcessFunction)


class Undeclared(F.KeyedBroadcastProcessFunction):
    def process_broadcast_element(self, rule, ctx, out):
        ctx.get_broadcast_state(MapStateDescriptor("typo"))

    def process_element(self, v, ctx, out):
        pass


class WritesOnTheElementSide(F.KeyedBroadcastProcessFunction):
    def __init__(self, how):
        self.how = how

    def process_broadcast_element(self, rule, ctx, out):
        pass

    def process_element(self, v, ctx, out):
        st = ctx.get_broadcast_state(RULES)
        assert st.get("x") is None and not st.contains("x") and st.immutableEntries() == ()
        {"put": lambda: st.put("x", 1), "put_all": lambda: st.put_all({"x": 1}),
         "remove": lambda: st.remove("x"), "clear": st.clear, "entries": st.entries}[self.how]()


def test_undeclared_descriptor_and_read_only_state():
    from mxstream.runtime.operators import BroadcastProcessOp, Rec

    op = _open(BroadcastProcessOp(lambda v: v[0], Undeclared(), (RULES,)))
    with pytest.raises(ValueError, match="The requested state does not exist. Check for typos in "
                                         "your state descriptor, or specify the state descriptor "
                                         r"in the datastream.broadcast\(...\) call if you forgot "
                                         "to register it."):
        op.process([Rec((1, ("r", 1)), 5, 0)])
    for how in ("put", "put_all", "remove", "clear", "entries"):
        op = _open(BroadcastProcessOp(lambda v: v[0], WritesOnTheElementSide(how), (RULES,)))
        with pytest.raises(TypeError, match="read-only"):
            op.process([Rec((0, ("a", 1)), 5, 0)])


def test_broadcast_state_methods():
    from mxstream.api.state import BroadcastState

    st = BroadcastState({})
    st.put("a", 1)
    st.putAll({"b": 2, "c": 3})
    assert st.get("a") == 1 and st.contains("b") and not st.contains("z") and st.get("z") is None
    assert st.entries() == [("a", 1), ("b", 2), ("c", 3)] == list(st.immutable_entries())
    st.remove("a")
    st.remove("a")
    assert st.entries() == [("b", 2), ("c", 3)]
    st.clear()
    assert st.immutable_entries() == ()


# ---- one copy per parallel instance ---------------------------------------------------------------
class KeyedEcho(F.KeyedProcessFunction):
    def process_element(self, e, ctx, out):
        out.collect(Tuple3(e[0], e[1], 1))


def test_broadcast_side_prints_once_per_subtask_and_elements_carry_the_keys_prefix():
    env, out = _env()
    _stream(env, SAMPLES, 2).key_by(0).connect(_stream(env, [("r", 1, 5)], 2).broadcast(RULES)) \
        .process(Keyed()).print()
    env.execute("prefixes")
    # the broadcast element reaches the P instances, each with a copy of its own: 1, not 1..4
    assert out[:P] == [f"{s}> (rule,r,1)" for s in range(1, P + 1)]
    env2, want = _env()
    _stream(env2, SAMPLES, 2).key_by(0).process(KeyedEcho()).print()
    env2.execute("key_by")
    # every key reads 1 (its instance's copy), under the prefix plain key_by gives it
    assert out[P:] == want and len(want) == len(SAMPLES) and len({ln[0] for ln in want}) > 1


class Visit(F.KeyedBroadcastProcessFunction):
    """Elements count per key in keyed state; a broadcast element visits every key's count."""

    def open(self, parameters=None):
        self.count = self.get_runtime_context().get_state(COUNT)

    def process_element(self, v, ctx, out):
        self.count.update((self.count.value() or 0) + 1)

    def process_broadcast_element(self, rule, ctx, out):
        ctx.apply_to_keyed_state(COUNT, lambda key, st: out.collect((key, st.value())))


def test_apply_to_keyed_state_reaches_every_key_once_over_the_subtasks():
    from mxstream.runtime.operators import BroadcastProcessOp, Rec

    op = _open(BroadcastProcessOp(lambda v: v[0], Visit(), (RULES,)))
    recs = [Rec((0, (k, i)), i, 0) for i, k in enumerate(KEYS + KEYS[:5])]
    assert op.process(recs) == []
    out = op.process([Rec((1, ("visit",)), 50, 0)])
    want = {k: 2 if k in KEYS[:5] else 1 for k in KEYS}
    assert sorted(r.value for r in out) == sorted(want.items())      # every key exactly once
    assert all(r.subtask == op.subtask_of(r.value[0]) and r.ts == 50 for r in out)
    assert [r.subtask for r in out] == sorted(r.subtask for r in out)  # subtask 0 first
    assert len({r.subtask for r in out}) > 1


# ---- timers ---------------------------------------------------------------------------------------
class Timers(F.KeyedBroadcastProcessFunction):
    def process_broadcast_element(self, rule, ctx, out):
        ctx.get_broadcast_state(RULES).put("last", rule[0])

    def process_element(self, v, ctx, out):
        ctx.timer_service().register_event_time_timer(ctx.timestamp() + 150)
        out.collect(("in", v[0], ctx.timerService().current_watermark()))

    def on_timer(self, timestamp, ctx, out):
        st = ctx.get_broadcast_state(RULES)
        assert ctx.time_domain == "EVENT_TIME" and ctx.timestamp() == timestamp
        with pytest.raises(TypeError):
            st.put("last", 0)
        out.collect(("timer", ctx.get_current_key(), timestamp, st.get("last")))


class Stamp(F.ProcessFunction):
    def process_element(self, value, ctx, out):
        out.collect((value, ctx.timestamp()))


def test_timers_fire_at_the_merged_watermark_and_see_the_read_only_state():
    from mxstream.api.time import Time
    from mxstream.api.watermarks import BoundedOutOfOrdernessTimestampExtractor as Ex

    env, _ = _env()
    ex = lambda: Ex(Time.milliseconds(0), extractor=lambda e: e[1])  # noqa: E731
    # the samples run ahead (timestamps to 900 by arrival 40), the rules lag behind
    a = env.from_timed_collection([(10, ("a", 100)), (20, ("a", 500)), (40, ("a", 900))]) \
        .assign_timestamps_and_watermarks(ex())
    b = env.from_timed_collection([(100, ("r1", 200)), (200, ("r2", 400)), (300, ("r3", 1000))]) \
        .assign_timestamps_and_watermarks(ex())
    got = a.key_by(0).connect(b.broadcast(RULES)).process(Timers()).process(Stamp()).collect()
    env.execute("timers")
    assert got == [
        (("in", "a", -(1 << 63)), 100), (("in", "a", -(1 << 63)), 500),
        (("in", "a", -(1 << 63)), 900),                 # no rule yet has a watermark: no timer
        (("timer", "a", 250, "r2"), 250),               # rules at 400: the merged watermark
        (("timer", "a", 650, "r3"), 650),               # rules at 1000, samples at 900
        (("timer", "a", 1050, "r3"), 1050)]             # left at the end of input: it fires


def test_late_elements_are_not_dropped():
    from mxstream.runtime.operators import WM, BroadcastProcessOp, Rec

    op = _open(BroadcastProcessOp(lambda v: v[0], Keyed(), (RULES,)))
    out = op.process([WM(1000), Rec((1, ("r", 1)), 5, 0), Rec((0, ("a", 7)), 6, 0)])
    vals = [it.value for it in out if isinstance(it, Rec)]
    assert vals[P:] == [Tuple3("a", 7, 1)] and len(vals) == P + 1


# ---- the non-keyed form ----------------------------------------------------------------------------
def test_non_keyed_form_has_no_timers_and_no_key_and_reads_its_own_subtasks_copy():
    from mxstream.runtime.operators import BroadcastProcessOp, Rec

    env, _ = _env()
    got = _stream(env, [("x", 100), ("y", 300)], 1) \
        .connect(_stream(env, [("r", 1, 200)], 2).broadcast(RULES)).process(Plain()).collect()
    env.execute("plain")
    # y sees the merged watermark: min(samples at 100, rules at 200); its own comes behind it
    assert got == [("x", [], 100, -(1 << 63)), ("y", [("r", 1)], 300, 100)]

    class OnlySubtask2(F.BroadcastProcessFunction):
        def process_broadcast_element(self, rule, ctx, out):
            st = ctx.get_broadcast_state(RULES)
            if self.n == 2:
                st.put("here", True)
            self.n += 1

        def process_element(self, v, ctx, out):
            out.collect(ctx.get_broadcast_state(RULES).contains("here"))

    fn = OnlySubtask2()
    fn.n = 0
    op = _open(BroadcastProcessOp(None, fn, (RULES,)))
    out = op.process([Rec((1, ("r",)), 5, 0)] + [Rec((0, ("v",)), 6, s) for s in range(P)])
    assert [(r.value, r.subtask) for r in out] == [(False, 0), (False, 1), (True, 2), (False, 3)]
    assert op.snapshot().keys() == {"wm", "broadcast"}


# ---- checkpoints -----------------------------------------------------------------------------------
class Both(F.KeyedBroadcastProcessFunction):
    """Keyed state, broadcast state, timers and the watermark in one function."""

    def open(self, parameters=None):
        self.count = self.get_runtime_context().get_state(COUNT)

    def process_broadcast_element(self, rule, ctx, out):
        ctx.get_broadcast_state(RULES).put(rule[0], rule[1])

    def process_element(self, v, ctx, out):
        self.count.update((self.count.value() or 0) + 1)
        ctx.timer_service().register_event_time_timer(ctx.timestamp() + 25)
        out.collect((v[0], self.count.value(),
                     sorted(ctx.get_broadcast_state(RULES).immutable_entries()),
                     ctx.current_watermark()))

    def on_timer(self, timestamp, ctx, out):
        out.collect(("timer", timestamp, ctx.get_broadcast_state(RULES).get("r1")))


def _items(lo, hi):
    from mxstream.runtime.operators import WM, Rec

    out = []
    for t in range(lo, hi, 10):
        if (t // 10) % 4 == 3:
            out.append(Rec((1, (f"r{t % 3}", t)), t, 0))
        else:
            out.append(Rec((0, (f"k{t % 7}", t)), t, 0))
        if t % 30 == 0:
            out.append(WM(t - 15))
    return out


def _flat(out):
    from mxstream.runtime.operators import WM

    return [it if isinstance(it, WM) else (it.value, it.ts, it.subtask) for it in out]


def test_snapshot_in_mid_stream_restore_and_continue():
    from mxstream.runtime.operators import WM, BroadcastProcessOp

    make = lambda p=P: _open(BroadcastProcessOp(lambda v: v[0], Both(), (RULES,)), p)  # noqa: E731
    ref = make()
    first, second = _flat(ref.process(_items(0, 200))), _flat(ref.process(_items(200, 400)))
    tail = _flat(ref.process([WM((1 << 63) - 1)]))
    assert any(isinstance(x, tuple) and x[0][0] == "timer" for x in tail)
    op = make()
    assert _flat(op.process(_items(0, 200))) == first
    snap = op.snapshot()
    assert snap["wm"] == 165 and snap["timers"]["event"] and snap["keyed"]
    assert len(snap["broadcast"]) == P and all(c == snap["broadcast"][0] for c in snap["broadcast"])
    op = make()
    op.restore(snap)
    snap["broadcast"][0]["rules"]["r0"] = "changed later"   # the operator holds copies of its own
    assert _flat(op.process(_items(200, 400))) == second
    assert _flat(op.process([WM((1 << 63) - 1)])) == tail


def test_restore_at_parallelism_2_of_a_snapshot_at_4():
    from mxstream.runtime.operators import WM, BroadcastProcessOp

    def make(p):
        return _open(BroadcastProcessOp(lambda v: v[0], Both(), (RULES,)), p)

    def values(out):
        return [it if isinstance(it, WM) else (it.value, it.ts) for it in out]

    ref = make(2)
    ref.process(_items(0, 200))
    second = ref.process(_items(200, 400))
    op = make(4)
    op.process(_items(0, 200))
    snap = op.snapshot()
    op = make(2)
    op.restore(snap)
    assert len(op.copies) == 2 and op.copies[1] == snap["broadcast"][1]
    got = op.process(_items(200, 400))
    assert values(got) == values(second)
    assert [it.subtask for it in got if not isinstance(it, WM)] \
        == [it.subtask for it in second if not isinstance(it, WM)]


def test_more_than_one_rank_raises():
    from mxstream.runtime.operators import BroadcastProcessOp

    class TwoRanks:
        world, rank = 2, 0

    with pytest.raises(NotImplementedError, match="broadcast state"):
        _open(BroadcastProcessOp(lambda v: v[0], Keyed(), (RULES,)), comm=TwoRanks())
