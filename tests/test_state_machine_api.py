"""``stream.key_by(0).process(StateMachineAlert(field, bounds, table, initial, report))``
(api/functions.py): the job on the native operator against the host KeyedProcessOp (a subclass,
native off, a key selector, a table beyond 16 states), the planner's choice, event-time order in
front of it, NativeStateMachineOp's fallbacks and its checkpoints."""
from __future__ import annotations

import numpy as np
import pytest

from mxstream.api import functions as F
from mxstream.api.time import Time
from mxstream.api.tuples import Tuple2, Tuple3
from mxstream.ops import kernels as K

BOUNDS, TABLE = [80.0, 90.0], [[0, 0, 1], [0, 1, 1]]      # on at 90, off only below 80


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


def _samples(ints=False):
    """Five hosts report every 10 s for 15 min. host1 climbs over 90 and hovers between 80 and
    90 before it falls; host2 spikes for single samples; host3 hovers around 90 without ever
    falling below 80; host4 goes up at 700 s and stays there."""
    events = []
    for i in range(450):
        h, t = i % 5, (i // 5) * 10_000 + (i % 5) * 7
        usage = 40.0 + (i % 7)
        if h == 1 and 100_000 <= t < 500_000:
            usage = 97.0 if t < 200_000 else 85.0
        if h == 2 and (i // 5) % 9 == 0:
            usage = 99.5
        if h == 3 and t >= 50_000:
            usage = 88.0 + (i // 5) % 4
        if h == 4 and t >= 700_000:
            usage = 93.0
        events.append((f"host{h}", int(usage) if ints else usage, t))
    return events


class HostAlert(F.StateMachineAlert):
    """A subclass keeps the host path: the planner lowers exactly StateMachineAlert."""


def first(v):
    """A key selector: the planner cannot see that it is field 0."""
    return v[0]


def _job(fn, native="auto", device="cpu", key=0, samples=None, int_keys=False):
    from mxstream.api.watermarks import BoundedOutOfOrdernessTimestampExtractor

    env, out = _env(native, device=device)
    samples = _samples() if samples is None else samples
    name = (lambda h: int(h[4:])) if int_keys else (lambda h: h)
    env.from_timed_collection([(e[2] + 10, e) for e in samples]) \
        .assign_timestamps_and_watermarks(BoundedOutOfOrdernessTimestampExtractor(
            Time.milliseconds(0), extractor=lambda e: e[2])) \
        .map(lambda e: Tuple3(name(e[0]), "cpu", e[1])).key_by(key) \
        .process(fn).print()
    env.execute("state-machine")
    return out


def _rule(cls=F.StateMachineAlert, bounds=BOUNDS, table=TABLE, **kw):
    return cls(2, bounds, table, **kw)


def _expected(samples, bounds=BOUNDS, table=TABLE, initial=0, report=None) -> list:
    """The direct loop."""
    state, out = {}, []
    for host, usage, t in samples:
        since, st = state.get(host) or (t, initial)
        to = table[st][sum(float(usage) >= b for b in bounds)]
        if (st != to) if report is None else ((st, to) in report):
            out.append(f"({host},{st},{to},{since},{usage})")
        state[host] = (t if to != st else since, to)
    return out


def _wide(states=17):
    """A counter of `states` states: a sample at or above 90 steps it, one below 80 resets it."""
    return [[0, s, (s + 1) % states] for s in range(states)]


@pytest.fixture
def route(monkeypatch):
    from mxstream.runtime.fsm_operator import KeyedStateMachineOperator
    from mxstream.runtime.native_ops import NativeStateMachineOp

    seen = {"built": 0, "fallback": 0}
    init, to_fb = KeyedStateMachineOperator.__init__, NativeStateMachineOp._to_fallback

    def spy_init(self, *a, **kw):
        seen["built"] += 1
        init(self, *a, **kw)

    def spy_fb(self):
        seen["fallback"] += 1
        to_fb(self)

    monkeypatch.setattr(KeyedStateMachineOperator, "__init__", spy_init)
    monkeypatch.setattr(NativeStateMachineOp, "_to_fallback", spy_fb)
    return seen


def _tail(lines):
    return [ln[ln.index("("):] for ln in lines]


def test_the_host_path_equals_a_direct_loop(route):
    host = _job(_rule(HostAlert))
    rows = _tail(host)
    assert rows == _expected(_samples())
    # host1 goes on once and off once although it hovers at 85 for five minutes; host3 hovers
    # around 90 and is reported once; host2's spikes are a line up and a line down each
    assert [r for r in rows if r.startswith("(host1")] == [
        "(host1,0,1,7,97.0)", "(host1,1,0,100007,46.0)"]
    assert len([r for r in rows if r.startswith("(host3")]) == 1
    assert len([r for r in rows if r.startswith("(host2")]) == 20
    assert _job(_rule(), "off") == host
    assert _job(_rule(), key=first) == host                      # a key selector
    big = _wide()                                                  # S = 17: the host operator
    got = _tail(_job(_rule(table=big, report=[(16, 0), (3, 4)])))
    assert got == _expected(_samples(), table=big, report={(16, 0), (3, 4)}) and len(got) >= 2
    assert route == {"built": 0, "fallback": 0}


def test_the_planner_lowers_the_exact_class_with_a_positional_key_on_one_rank():
    from mxstream.api import planner
    from mxstream.runtime.native_ops import NativeStateMachineOp
    from mxstream.runtime.operators import KeyedProcessOp

    class Comm:
        world, rank = 2, 0

    ops = {}
    for name, fn, key, world in (
            ("exact", _rule(), 0, 1), ("sub", _rule(HostAlert), 0, 1),
            ("selector", _rule(), first, 1), ("ranks", _rule(), 0, 2),
            ("s16", _rule(table=_wide(16)), 0, 1), ("s17", _rule(table=_wide(17)), 0, 1),
            ("c16", _rule(bounds=list(range(15)), table=[[0] * 16]), 0, 1),
            ("ordered", F.EventTimeOrdered(_rule()), 0, 1),
            ("ordered_sub", F.EventTimeOrdered(_rule(HostAlert)), 0, 1),
            ("ordered_s17", F.EventTimeOrdered(_rule(table=_wide(17))), 0, 1)):
        env, _ = _env()
        if world > 1:
            env._comm = Comm()
        s = env.from_collection([("a", "b", 1.0)]).key_by(key).process(fn)
        assert s.t.meta["kind"] == "keyed_process" and s.t.meta["fn"] is fn
        planner._lower_keyed_process(env, s.t, s.t.meta)
        op = s.t.factory()
        ops[name] = (type(op), bool(s.t.meta.get("native")), getattr(op, "ordered", None))
    assert ops["exact"] == ops["s16"] == ops["c16"] == (NativeStateMachineOp, True, False)
    assert ops["ordered"] == (NativeStateMachineOp, True, True)
    for name in ("sub", "selector", "ranks", "s17", "ordered_sub", "ordered_s17"):
        assert ops[name] == (KeyedProcessOp, False, None)


@pytest.mark.parametrize("ints,int_keys", [(False, False), (True, False), (False, True)])
def test_the_native_job_on_cpu_equals_the_host_path(route, ints, int_keys):
    samples = _samples(ints)
    host = _job(_rule(HostAlert), samples=samples, int_keys=int_keys)
    assert route == {"built": 0, "fallback": 0}
    native = _job(_rule(), samples=samples, int_keys=int_keys)
    assert route == {"built": 1, "fallback": 0}
    assert native == host and len({ln[0] for ln in native}) > 1   # several subtasks print
    if not int_keys:
        assert _tail(native) == _expected(samples)
    sev = dict(bounds=[80, 90], table=[[0, 1, 2]] * 3, initial=1, report=[(1, 2), (2, 2), (0, 1)])
    got = _job(_rule(**sev), samples=samples, int_keys=int_keys)
    assert got == _job(_rule(HostAlert, **sev), samples=samples, int_keys=int_keys)
    assert sum(",2,2," in ln for ln in got) > 20                   # the self-loop is reported


def test_event_time_order_lowers_and_equals_the_host_wrapper(route, monkeypatch):
    """Every 7th sample arrives 25 s late -- behind the two samples that follow it, inside the
    30 s bound -- and every 31st 70 s late, beyond it."""
    from collections import Counter

    from mxstream.api.watermarks import BoundedOutOfOrdernessTimestampExtractor
    from mxstream.runtime.native_ops import NativeStateMachineOp

    events = sorted((e[2] + (70_000 if i % 31 == 5 else 25_000 if i % 7 == 3 else 0), i, e)
                    for i, e in enumerate(_samples()))
    timed = [(a + 10, e) for a, _, e in events]
    ops = []
    init = NativeStateMachineOp.__init__

    def spy(self, *a, **kw):
        ops.append(self)
        init(self, *a, **kw)

    monkeypatch.setattr(NativeStateMachineOp, "__init__", spy)

    def job(fn):
        env, out = _env()
        env.from_timed_collection(timed) \
            .assign_timestamps_and_watermarks(BoundedOutOfOrdernessTimestampExtractor(
                Time.seconds(30), extractor=lambda e: e[2])) \
            .map(lambda e: Tuple3(e[0], "cpu", e[1])).key_by(0).process(fn).print()
        env.execute("ordered-state-machine")
        return out

    def per_key(lines):
        rows = _tail(lines)
        return {k: [r for r in rows if r.startswith(f"({k},")] for k in
                {r[1:r.index(",")] for r in rows}}

    wrapper = F.EventTimeOrdered(_rule(HostAlert))    # the rule's subclass keeps the host wrapper
    host = job(wrapper)
    assert not ops and route == {"built": 0, "fallback": 0}
    assert wrapper.late_dropped >= 5 and len(host) > 20
    native = job(F.EventTimeOrdered(_rule()))
    assert len(ops) == 1 and ops[0].ordered and route == {"built": 1, "fallback": 0}
    assert Counter(native) == Counter(host) and per_key(native) == per_key(host)
    assert ops[0].num_late_records_dropped == wrapper.late_dropped
    # the wrapper matters on this stream: the plain rule reports other rows
    assert Counter(_tail(job(_rule()))) != Counter(_tail(host))


def test_records_without_timestamps_raise_on_both_paths():
    from mxstream.runtime.executor import JobExecutionException

    for fn, native in ((_rule(), "auto"), (_rule(HostAlert), "auto"), (_rule(), "off")):
        env, _ = _env(native)
        env.from_collection([("a", "cpu", 95.0)]).key_by(0).process(fn).print()
        with pytest.raises(JobExecutionException, match="ValueError: StateMachineAlert: a "
                                                        "record without an event timestamp") as e:
            env.execute("no-timestamps")
        assert isinstance(e.value.__cause__, ValueError)


def test_constructor_validation():
    fn = F.StateMachineAlert(2, [80, 90.0], [[0, 0, 1], [0, 1, 1]])
    assert (fn.field, fn.bounds, fn.table, fn.initial) == (2, (80.0, 90.0),
                                                            ((0, 0, 1), (0, 1, 1)), 0)
    assert fn.report == ((0, 1), (1, 0))
    assert fn.native == ("state_machine", 2, (80.0, 90.0), ((0, 0, 1), (0, 1, 1)), 0,
                         ((0, 1), (1, 0)))
    assert all(type(b) is float for b in fn.native[2])
    same = F.StateMachineAlert(2, (80.0, 90), ([0, 0, 1], (0, 1, 1)), 0, [(1, 0), [0, 1], (1, 0)])
    from mxstream.runtime.native_ops import _same_spec

    assert same.native == fn.native and _same_spec(same.native, fn.native)
    assert not _same_spec(fn.native, F.StateMachineAlert(2, [80, 91], TABLE).native)
    assert not _same_spec(fn.native, F.StateMachineAlert(2, BOUNDS, TABLE, report=()).native)
    assert F.StateMachineAlert(0, [1], [[0, 0]], report=()).report == ()
    assert F.StateMachineAlert(0, [1], [[0, 0]], report=[(0, 0)]).report == ((0, 0),)
    assert isinstance(fn, F.KeyedProcessFunction)
    assert len(F.StateMachineAlert(0, list(range(15)), [[0] * 16] * 40).table) == 40
    for bad in (-1, True, 1.5, "2", None):
        with pytest.raises(ValueError, match="field"):
            F.StateMachineAlert(bad, BOUNDS, TABLE)
    for bad in ([], list(range(16)), [90.0, 80.0], [80.0, 80.0], [80.0, float("nan")],
                [float("inf")], [-float("inf"), 1.0], [2 ** 53, 2 ** 53 + 1]):
        with pytest.raises(ValueError, match="bounds"):
            F.StateMachineAlert(2, bad, [[0] * (len(bad) + 1)])
    for bad in (["80"], [True, 90.0], [None], 80.0):
        with pytest.raises(TypeError, match="bound"):
            F.StateMachineAlert(2, bad, [[0, 0]])
    for bad in ([], [[0, 0]], [[0, 0, 1], [0, 1]], [[0, 0, 2], [0, 1, 1]], [[0, 0, -1], [0, 1, 1]],
                [[0, 0, True], [0, 1, 1]], [[0, 0, 1.0], [0, 1, 1]]):
        with pytest.raises(ValueError, match="table"):
            F.StateMachineAlert(2, BOUNDS, bad)
    for bad in (3, [0, 1]):
        with pytest.raises(TypeError, match="table"):
            F.StateMachineAlert(2, BOUNDS, bad)
    for bad in (2, -1, True, 0.0, None):
        with pytest.raises(ValueError, match="initial"):
            F.StateMachineAlert(2, BOUNDS, TABLE, bad)
    for bad in ("changes", [(0, 2)], [(-1, 0)], [(0, 1, 1)], [(0, True)], [(0, 1.0)]):
        with pytest.raises(ValueError, match="report"):
            F.StateMachineAlert(2, BOUNDS, TABLE, report=bad)
    for bad in (1, [1, 2]):
        with pytest.raises(TypeError, match="report"):
            F.StateMachineAlert(2, BOUNDS, TABLE, report=bad)


def test_a_value_that_is_no_number_is_a_type_error_on_the_host_path():
    from mxstream.runtime.operators import Rec

    op = _host()
    for bad in ("97", True, None):
        with pytest.raises(TypeError, match="value"):
            op.process([Rec(Tuple2("a", bad), 5, 0)])


# ---- NativeStateMachineOp against the host operator --------------------------------------------
SEV = dict(bounds=(62.0, 78.0), table=((0, 1, 2),) * 3, initial=0, report="change")


def _ctx():
    from mxstream.runtime.operators import OpContext

    return OpContext("state-machine", 4, 128, lambda: 0, "EventTime")


def _fn(field=1, **kw):
    return F.StateMachineAlert(field, **{**SEV, **kw})


def _host(key_pos=0, **kw):
    from mxstream.runtime.operators import KeyedProcessOp

    op = KeyedProcessOp(lambda v: v[key_pos], _fn(**kw))
    op.open(_ctx())
    return op


def _native(key_pos=0, device="cpu", dense_limit=1 << 26, **kw):
    from mxstream.runtime.native_ops import NativeStateMachineOp

    op = NativeStateMachineOp(fn=_fn(**kw), key_pos=key_pos, device=device,
                              dense_limit=dense_limit,
                              fallback_factory=lambda: _host(key_pos, **kw))
    op.open(_ctx())
    return op


def _lines(items) -> list:
    """Output as the watermarks and the (text, ts, subtask) rows, in order."""
    from mxstream.runtime.columnar import expand_columns
    from mxstream.runtime.operators import WM

    return [it if isinstance(it, WM) else (str(it.value), it.ts, it.subtask)
            for it in expand_columns(list(items))]


def _passes(seed, mode, passes=12, ints=False):
    """Passes of records ("recs"), column batches ("str" / "int" keys) or both, with watermarks;
    values ~ base[key] + N(0, 8) around the bounds, as doubles or as longs."""
    from mxstream.ops.native import load
    from mxstream.ops.text import FK_DOUBLE, FK_LONG, FK_STR
    from mxstream.runtime.columnar import ColumnBatch
    from mxstream.runtime.operators import WM, Rec

    rng = np.random.default_rng(seed)
    sd = load().StringDict()
    str_keys = mode in ("recs", "str")
    key = (lambda i: f"host{i}") if str_keys else (lambda i: int(i) * 3)
    base = rng.uniform(50, 95, 25)
    now = 1_000
    for _ in range(passes):
        items = []
        for _ in range(int(rng.integers(1, 5))):
            n = int(rng.integers(1, 40))
            ks = rng.integers(0, 25, n)
            tsa = (now + rng.integers(-20, 20, n)).astype(np.int64)
            vals = np.round(base[ks] + rng.normal(0, 8, n), 1)
            vals = vals.astype(np.int64) if ints else vals
            now += int(rng.integers(5, 50))
            if mode != "recs" and rng.integers(0, 3):
                kcol = (np.array([sd.intern(key(k)) for k in ks]) if str_keys
                        else np.array([key(k) for k in ks], dtype=np.int64))
                items.append(ColumnBatch(n, [kcol, vals],
                                         (FK_STR if str_keys else FK_LONG,
                                          FK_LONG if ints else FK_DOUBLE),
                                         sd if str_keys else None, tsa, np.zeros(n, np.int32)))
            else:
                items.extend(Rec(Tuple2(key(k), v), int(t), 0)
                             for k, v, t in zip(ks, vals.tolist(), tsa))
            if rng.integers(0, 2):
                items.append(WM(now - int(rng.integers(0, 60))))
        yield items


@pytest.mark.parametrize("mode,ints", [("recs", False), ("str", False), ("int", False),
                                       ("recs", True), ("int", True)])
def test_native_operator_equals_the_host_operator(mode, ints):
    from mxstream.ops.text import FK_DOUBLE, FK_LONG, FK_STR
    from mxstream.runtime.columnar import ColumnBatch, expand_columns
    from mxstream.runtime.operators import WM

    native, host = _native(), _host()
    rows = 0
    pairs = set()
    for items in list(_passes(17, mode, ints=ints)) + [[WM(K.I64_MAX)]]:
        got, want = native.process(list(items)), host.process(expand_columns(list(items)))
        assert all(isinstance(it, (ColumnBatch, WM)) for it in got)
        # the host operator emits a record's rows at the record; the native one before the
        # watermark that follows: the same rows in the same order between the same watermarks
        assert _lines(got) == _lines(want)
        for cb in got:
            if isinstance(cb, ColumnBatch):
                assert cb.kinds == (FK_STR if mode != "int" else FK_LONG, FK_LONG, FK_LONG,
                                    FK_LONG, FK_LONG if ints else FK_DOUBLE)
                rows += cb.n
                pairs.update(zip(cb.cols[1].tolist(), cb.cols[2].tolist()))
    assert native.fallback is None and native.op is not None and rows >= 50
    assert pairs == {(a, b) for a in range(3) for b in range(3) if a != b}
    assert native.finish() == host.finish() == []


def _rec(value, ts=5):
    from mxstream.runtime.operators import Rec

    return Rec(value, ts, 0)


def _column_batch(kinds, cols, ts=(5, 6)):
    from mxstream.runtime.columnar import ColumnBatch

    return [ColumnBatch(2, [np.asarray(c) for c in cols], kinds, None,
                        None if ts is None else np.array(ts, dtype=np.int64),
                        np.zeros(2, np.int32))]


def _fallbacks():
    from mxstream.ops.text import FK_DOUBLE, FK_LONG

    big = 1 << 62
    return {
        "non_tuple": (lambda: [_rec(["a", 80.0])], None),
        "text_value": (lambda: [_rec(Tuple2("a", "80"))], TypeError),
        "bool_value": (lambda: [_rec(Tuple2("a", True))], TypeError),
        "mixed_values": (lambda: [_rec(Tuple2("a", 80.0)), _rec(Tuple2("a", 60), 60)], None),
        "mixed_value_columns": (
            lambda: _column_batch((FK_LONG, FK_DOUBLE), [[3, 3], [80.0, 61.0]], (5, 50))
            + _column_batch((FK_LONG, FK_LONG), [[3, 3], [80, 10]], (60, 70)), None),
        "key_at_dense_limit": (lambda: [_rec(Tuple2(100, 80.0)), _rec(Tuple2(100, 61.0), 50)],
                               None),
        "no_timestamp": (lambda: [_rec(Tuple2("a", 80.0), K.I64_MIN)], ValueError),
        "timestamp_at_2_62": (lambda: [_rec(Tuple2("a", 80.0), 0), _rec(Tuple2("a", 61.0), big)],
                              None),
    }


FALLBACKS = _fallbacks()


@pytest.mark.parametrize("case", sorted(FALLBACKS))
def test_unsupported_data_falls_back_before_state_exists_and_raises_after(case):
    from mxstream.runtime.columnar import expand_columns
    from mxstream.runtime.operators import WM

    make, host_error = FALLBACKS[case]
    int_keys = case in ("key_at_dense_limit", "mixed_value_columns")
    good = [_rec(Tuple3(3, 80.0, 3) if int_keys else Tuple3("b", 80.0, "b"), 1)]
    tail = [WM(50), WM(K.I64_MAX)]
    # before native state exists: the host operator, told the watermark that was pending
    op = _native(dense_limit=100)
    assert op.process([WM(-7)]) == [WM(-7)] and op.op is None
    if host_error is not None:
        with pytest.raises(host_error):
            op.process(make() + tail)
        assert op.fallback is not None and op.op is None and op.fallback.wm == -7
    else:
        host = _host()
        host.process([WM(-7)])
        got = op.process(make() + tail)
        assert op.fallback is not None and op.op is None
        assert _lines(got) == _lines(host.process(expand_columns(make()) + tail))
        if case != "non_tuple":
            assert sum(not isinstance(x, WM) for x in _lines(got)) >= 1
    # afterwards: an error
    op = _native(dense_limit=100)
    op.process(good + [WM(2)])
    assert op.op is not None and op.fallback is None
    with pytest.raises(ValueError if case == "no_timestamp" else TypeError):
        op.process(make() + tail)
    assert op.fallback is None


def test_checkpoint_in_mid_stream_gives_the_uninterrupted_output_and_a_foreign_one_raises():
    passes = list(_passes(23, "str", passes=10))
    ref, op = _native(), _native()
    want = [_lines(ref.process(list(p))) for p in passes]
    assert sum(len(w) for w in want) > 30
    for i, p in enumerate(passes):
        if i == 5:
            snap = op.snapshot()
            assert snap["state_machine"] == _fn().native
            assert snap["engine"]["meta"]["kind"] == "state_machine"
            assert snap["engine"]["columns"]["key"].size >= 10
            assert set(snap["engine"]["columns"]["state"].tolist()) == {0, 1, 2}
            op = _native()
            op.restore(snap)
        assert _lines(op.process(list(p))) == want[i]
    others = (dict(bounds=(62.0, 79.0)), dict(table=((0, 1, 2), (0, 1, 2), (0, 1, 1))),
              dict(initial=1), dict(report=((0, 1),)), dict(field=0),
              dict(bounds=(62.0,), table=((0, 1),) * 3))
    for other in others:
        with pytest.raises(ValueError, match="checkpoint of a different state-machine function"):
            _native(**other).restore(snap)
    _native(bounds=(62, 78)).restore(snap)     # the same doubles: the same function
    ordered = _native()
    ordered.ordered = True
    with pytest.raises(ValueError, match="without event-time order"):
        ordered.restore(snap)
    with pytest.raises(RuntimeError, match="pending"):
        op.pending.append(_rec(Tuple2("a", 1.0)))
        op.snapshot()


def test_several_ranks_fall_back_in_open():
    from mxstream.runtime.native_ops import NativeStateMachineOp

    class Comm:
        world = 2

    ctx = _ctx()
    ctx.comm = Comm()
    op = NativeStateMachineOp(fn=_fn(), key_pos=0, device="cpu", fallback_factory=_host)
    op.open(ctx)
    assert op.fallback is not None and op.op is None


# ---- GPU ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_job_equals_the_host_path(gpu_device, route):
    host = _job(_rule(HostAlert))
    got = _job(_rule(), device="cuda")
    assert route == {"built": 1, "fallback": 0}
    assert got == host and len(got) > 20
    sev = dict(bounds=[80, 90], table=[[0, 1, 2]] * 3, initial=1, report=[(1, 2), (2, 2), (0, 1)])
    ints = _samples(True)
    assert _job(_rule(**sev), device="cuda", samples=ints) == _job(_rule(HostAlert, **sev),
                                                                   samples=ints)


@pytest.mark.gpu
def test_gpu_native_operator_takes_device_batches_and_restores(gpu_device):
    import torch

    from mxstream.ops.text import FK_DOUBLE, FK_LONG
    from mxstream.runtime.columnar import DeviceColumnBatch, expand_columns
    from mxstream.runtime.operators import WM

    def dev(a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(gpu_device)

    native, host = _native(device=gpu_device), _host()
    rng = np.random.default_rng(4)
    base = rng.uniform(50, 95, 60)
    rows = 0
    for step in range(6):
        n = 500
        keys = rng.integers(0, 60, n).astype(np.int64)
        ts = (1_000 + 40 * step + rng.integers(-20, 20, n)).astype(np.int64)
        vals = np.round(base[keys] + rng.normal(0, 8, n), 1)
        cb = DeviceColumnBatch(n, [dev(keys, torch.int64), dev(vals, torch.float64)],
                               (FK_LONG, FK_DOUBLE), None, dev(ts, torch.int64), parallelism=4)
        items = [cb, WM(1_000 + 40 * step)]
        if step == 3:
            snap = native.snapshot()
            native = _native(device=gpu_device)
            native.restore(snap)
        got = _lines(native.process(list(items)))
        assert got == _lines(host.process(expand_columns(list(items))))
        rows += len(got) - 1
    assert native.fallback is None and native.op.device.type == "cuda" and rows > 50
