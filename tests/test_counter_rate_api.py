"""``stream.key_by(0).process(CounterRate(field, per, when, threshold, max_gap))``
(api/functions.py): the job on the native operator against the host KeyedProcessOp (a subclass,
native off, a key selector), the planner's choice, event-time order in front of it,
NativeCounterRateOp's fallbacks and its checkpoints."""
from __future__ import annotations

import numpy as np
import pytest

from mxstream.api import functions as F
from mxstream.api.time import Time
from mxstream.api.tuples import Tuple2, Tuple3
from mxstream.ops import kernels as K

RULE = dict(per=Time.seconds(1), when="<", threshold=400.0, max_gap=Time.seconds(25))


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


def _samples(ints=True):
    """Five hosts report a byte counter every 10 s for 15 min. host1 restarts twice; host2 stalls
    (the counter stands still) for a while; host3 is silent for a minute; every 11th sample is
    sent twice and every 13th arrives behind its successor."""
    events, total = [], [0] * 5
    for i in range(450):
        h, t = i % 5, (i // 5) * 10_000 + (i % 5) * 7
        step = 3000 + 997 * ((i * 7) % 11)
        if h == 2 and 300_000 <= t < 400_000:
            step = 0
        if h == 1 and (i // 5) in (30, 60):
            total[h] = 0
        total[h] += step
        if h == 3 and 500_000 <= t < 560_000:
            continue
        v = total[h] if ints else total[h] / 8.0
        events.append((f"host{h}", v, t))
        if i % 11 == 4:
            events.append((f"host{h}", v, t))
    for j in range(13, len(events) - 6, 13):      # behind the same host's next sample
        e = events.pop(j)
        nxt = next(x for x in range(j, len(events)) if events[x][0] == e[0])
        events.insert(nxt + 1, e)
    return events


class HostRate(F.CounterRate):
    """A subclass keeps the host path: the planner lowers exactly CounterRate."""


def first(v):
    """A key selector: the planner cannot see that it is field 0."""
    return v[0]


def _job(fn, native="auto", device="cpu", key=0, samples=None, int_keys=False):
    from mxstream.api.watermarks import BoundedOutOfOrdernessTimestampExtractor

    env, out = _env(native, device=device)
    samples = _samples() if samples is None else samples
    name = (lambda h: int(h[4:])) if int_keys else (lambda h: h)
    env.from_timed_collection([(i + 10, e) for i, e in enumerate(samples)]) \
        .assign_timestamps_and_watermarks(BoundedOutOfOrdernessTimestampExtractor(
            Time.seconds(15), extractor=lambda e: e[2])) \
        .map(lambda e: Tuple3(name(e[0]), "eth0", e[1])).key_by(key) \
        .process(fn).print()
    env.execute("counter-rate")
    return out


def _rate(cls=F.CounterRate, **kw):
    return cls(2, **kw)


def _expected(samples, per=1000, when=None, threshold=None, max_gap=None):
    """The direct loop -> (lines, ignored samples)."""
    import operator

    cmp = {"<": operator.lt, ">": operator.gt, "!=": operator.ne}
    state, out, ignored = {}, [], 0
    for host, v, t in samples:
        cur = state.get(host)
        if cur is None:
            state[host] = (t, v)
            continue
        if t <= cur[0]:
            ignored += 1
            continue
        dt = t - cur[0]
        inc = v - cur[1] if v >= cur[1] else v
        state[host] = (t, v)
        if max_gap is not None and dt > max_gap:
            continue
        rate = float(inc) * float(per) / float(dt)
        if when is None or cmp[when](rate, float(threshold)):
            out.append(f"({host},{rate},{inc},{dt})")
    return out, ignored


@pytest.fixture
def route(monkeypatch):
    from mxstream.runtime.native_ops import NativeCounterRateOp
    from mxstream.runtime.rate_operator import KeyedRateOperator

    seen = {"built": 0, "fallback": 0, "ops": []}
    init, to_fb = KeyedRateOperator.__init__, NativeCounterRateOp._to_fallback

    def spy_init(self, *a, **kw):
        seen["built"] += 1
        seen["ops"].append(self)
        init(self, *a, **kw)

    def spy_fb(self):
        seen["fallback"] += 1
        to_fb(self)

    monkeypatch.setattr(KeyedRateOperator, "__init__", spy_init)
    monkeypatch.setattr(NativeCounterRateOp, "_to_fallback", spy_fb)
    return seen


def _tail(lines):
    return [ln[ln.index("("):] for ln in lines]


def _routes(route):
    return {k: route[k] for k in ("built", "fallback")}


def test_the_host_path_equals_a_direct_loop(route):
    fn = _rate(HostRate)
    host = _job(fn)
    rows = _tail(host)
    want, ignored = _expected(_samples())
    assert rows == want and fn.out_of_order == ignored and ignored > 40
    # host1's restarts are increases of the new reading, never negative
    assert len(rows) > 300 and not any(",-" in r for r in rows)
    ruled = _rate(HostRate, **RULE)
    got = _tail(_job(ruled))
    assert got == _expected(_samples(), 1000, "<", 400.0, 25_000)[0] and 5 < len(got) < 100
    assert any(r.startswith("(host2,0.0,0,") for r in got)       # the stalled counter
    assert _job(_rate(), "off") == host
    assert _job(_rate(), key=first) == host                      # a key selector
    assert _routes(route) == {"built": 0, "fallback": 0}


def test_the_planner_lowers_the_exact_class_with_a_positional_key_on_one_rank():
    from mxstream.api import planner
    from mxstream.runtime.native_ops import NativeCounterRateOp
    from mxstream.runtime.operators import KeyedProcessOp

    class Comm:
        world, rank = 2, 0

    ops = {}
    for name, fn, key, world in (
            ("exact", _rate(), 0, 1), ("ruled", _rate(**RULE), 0, 1),
            ("sub", _rate(HostRate), 0, 1), ("selector", _rate(), first, 1),
            ("ranks", _rate(), 0, 2), ("ordered", F.EventTimeOrdered(_rate()), 0, 1),
            ("ordered_sub", F.EventTimeOrdered(_rate(HostRate)), 0, 1),
            ("ordered_ranks", F.EventTimeOrdered(_rate()), 0, 2)):
        env, _ = _env()
        if world > 1:
            env._comm = Comm()
        s = env.from_collection([("a", "b", 1.0)]).key_by(key).process(fn)
        assert s.t.meta["kind"] == "keyed_process" and s.t.meta["fn"] is fn
        planner._lower_keyed_process(env, s.t, s.t.meta)
        op = s.t.factory()
        ops[name] = (type(op), bool(s.t.meta.get("native")), getattr(op, "ordered", None))
    assert ops["exact"] == ops["ruled"] == (NativeCounterRateOp, True, False)
    assert ops["ordered"] == (NativeCounterRateOp, True, True)
    for name in ("sub", "selector", "ranks", "ordered_sub", "ordered_ranks"):
        assert ops[name] == (KeyedProcessOp, False, None)


@pytest.mark.parametrize("ints,int_keys", [(True, False), (False, False), (True, True),
                                           (False, True)])
def test_the_native_job_on_cpu_equals_the_host_path(route, ints, int_keys):
    samples = _samples(ints)
    hfn = _rate(HostRate)
    host = _job(hfn, samples=samples, int_keys=int_keys)
    assert _routes(route) == {"built": 0, "fallback": 0}
    native = _job(_rate(), samples=samples, int_keys=int_keys)
    assert _routes(route) == {"built": 1, "fallback": 0}
    assert native == host and len({ln[0] for ln in native}) > 1   # several subtasks print
    assert route["ops"][0].out_of_order == hfn.out_of_order > 40
    if not int_keys:
        assert _tail(native) == _expected(samples)[0]
    got = _job(_rate(**RULE), samples=samples, int_keys=int_keys)
    assert got == _job(_rate(HostRate, **RULE), samples=samples, int_keys=int_keys)
    # (the double counters are an eighth of the long ones: all but the gaps are below 400)
    assert 5 < len(got) < (100 if ints else len(native))


def test_event_time_order_lowers_and_equals_the_host_wrapper(route, monkeypatch):
    """Every 7th sample arrives 25 s late -- behind the two samples that follow it, inside the
    30 s bound -- and every 31st 70 s late, beyond it. Behind the reorder buffer the rule sees
    no straggler: what it ignores are the samples that were sent twice."""
    from collections import Counter

    from mxstream.api.watermarks import BoundedOutOfOrdernessTimestampExtractor
    from mxstream.runtime.native_ops import NativeCounterRateOp

    events = sorted((e[2] + (70_000 if i % 31 == 5 else 25_000 if i % 7 == 3 else 0), i, e)
                    for i, e in enumerate(_samples()))
    timed = [(a + 10, e) for a, _, e in events]
    ops = []
    init = NativeCounterRateOp.__init__

    def spy(self, *a, **kw):
        ops.append(self)
        init(self, *a, **kw)

    monkeypatch.setattr(NativeCounterRateOp, "__init__", spy)

    def job(fn):
        env, out = _env()
        env.from_timed_collection(timed) \
            .assign_timestamps_and_watermarks(BoundedOutOfOrdernessTimestampExtractor(
                Time.seconds(30), extractor=lambda e: e[2])) \
            .map(lambda e: Tuple3(e[0], "eth0", e[1])).key_by(0).process(fn).print()
        env.execute("ordered-counter-rate")
        return out

    def per_key(lines):
        rows = _tail(lines)
        return {k: [r for r in rows if r.startswith(f"({k},")] for k in
                {r[1:r.index(",")] for r in rows}}

    inner = _rate(HostRate)
    wrapper = F.EventTimeOrdered(inner)    # the rule's subclass keeps the host wrapper
    host = job(wrapper)
    assert not ops and _routes(route) == {"built": 0, "fallback": 0}
    assert wrapper.late_dropped >= 5 and len(host) > 300
    native = job(F.EventTimeOrdered(_rate()))
    assert len(ops) == 1 and ops[0].ordered and _routes(route) == {"built": 1, "fallback": 0}
    assert Counter(native) == Counter(host) and per_key(native) == per_key(host)
    assert ops[0].num_late_records_dropped == wrapper.late_dropped
    # in event-time order only equal timestamps are ignored: the samples sent twice
    ordered = [e for _, e in timed]
    kept = sorted(ordered, key=lambda e: e[2])
    twice = sum(a[0] == b[0] and a[2] == b[2] for a, b in zip(kept, kept[1:]))
    assert 0 < ops[0].out_of_order == inner.out_of_order <= twice
    plain = _rate(HostRate)
    assert Counter(_tail(job(plain))) != Counter(_tail(host))    # the wrapper matters here
    assert plain.out_of_order > inner.out_of_order


def test_records_without_timestamps_raise_on_both_paths():
    from mxstream.runtime.executor import JobExecutionException

    for fn, native in ((_rate(), "auto"), (_rate(HostRate), "auto"), (_rate(), "off")):
        env, _ = _env(native)
        env.from_collection([("a", "eth0", 95)]).key_by(0).process(fn).print()
        with pytest.raises(JobExecutionException, match="ValueError: CounterRate: a "
                                                        "record without an event timestamp") as e:
            env.execute("no-timestamps")
        assert isinstance(e.value.__cause__, ValueError)


def test_constructor_validation():
    from mxstream.runtime.native_ops import _same_spec

    fn = F.CounterRate(2)
    assert (fn.field, fn.per_ms, fn.when, fn.threshold, fn.max_gap_ms) == (2, 1000, None, None,
                                                                         None)
    assert fn.native == ("counter_rate", 2, 1000, None, None, None) and fn.out_of_order == 0
    assert isinstance(fn, F.KeyedProcessFunction)
    ruled = F.CounterRate(2, **RULE)
    assert ruled.native == ("counter_rate", 2, 1000, "<", 400.0, 25_000)
    assert _same_spec(ruled.native, F.CounterRate(2, 1000, "<", 400.0, 25_000).native)
    assert not _same_spec(ruled.native, F.CounterRate(2, 1000, "<", 400, 25_000).native)
    assert not _same_spec(ruled.native, fn.native)
    assert F.CounterRate(0, per=Time.minutes(1)).per_ms == 60_000
    assert F.CounterRate(0, max_gap=(1 << 62) - 1).max_gap_ms == (1 << 62) - 1
    nan = F.CounterRate(0, when="!=", threshold=float("nan"))
    assert _same_spec(nan.native, F.CounterRate(0, when="!=", threshold=float("nan")).native)
    for bad in (-1, True, 1.5, "2", None):
        with pytest.raises(ValueError, match="field"):
            F.CounterRate(bad)
    for bad in (0, -5, True, 1.5, "1", None):
        with pytest.raises(ValueError, match="per"):
            F.CounterRate(2, per=bad)
    for bad in (0, -1, True, 2.5, "1", 1 << 62):
        with pytest.raises(ValueError, match="max_gap"):
            F.CounterRate(2, max_gap=bad)
    for bad in ("=", "lt", 1, "=<"):
        with pytest.raises(ValueError, match="when"):
            F.CounterRate(2, when=bad, threshold=1.0)
    with pytest.raises(ValueError, match="threshold"):
        F.CounterRate(2, when="<")
    with pytest.raises(ValueError, match="threshold"):
        F.CounterRate(2, threshold=1.0)
    for bad in ("1", True, [1.0]):
        with pytest.raises(TypeError, match="threshold"):
            F.CounterRate(2, when="<", threshold=bad)


def test_the_host_path_wraps_longs_and_refuses_what_is_no_counter():
    from mxstream.runtime.operators import Rec

    op = _host()
    for bad in ("97", True, None, 1 << 63):
        with pytest.raises(TypeError, match="value"):
            op.process([Rec(Tuple2("a", bad), 5, 0)])
    op.process([Rec(Tuple2("a", 5), 5, 0)])
    with pytest.raises(TypeError, match="all ints or all floats"):
        op.process([Rec(Tuple2("a", 6.0), 6, 0)])
    got = op.process([Rec(Tuple2("w", K.I64_MIN + 5), 1, 0), Rec(Tuple2("w", K.I64_MAX), 2, 0),
                      Rec(Tuple2("n", 1.0), 1, 0), Rec(Tuple2("n", float("nan")), 2, 0),
                      Rec(Tuple2("n", 2.0), 3, 0)])
    assert [str(r.value) for r in got] == ["(w,-6000.0,-6,1)", "(n,NaN,NaN,1)",
                                           "(n,2000.0,2.0,1)"]


# ---- NativeCounterRateOp against the host operator ---------------------------------------------
def _ctx():
    from mxstream.runtime.operators import OpContext

    return OpContext("counter-rate", 4, 128, lambda: 0, "EventTime")


def _fn(field=1, **kw):
    return F.CounterRate(field, **kw)


def _host(key_pos=0, **kw):
    from mxstream.runtime.operators import KeyedProcessOp

    op = KeyedProcessOp(lambda v: v[key_pos], _fn(**kw))
    op.open(_ctx())
    return op


def _native(key_pos=0, device="cpu", dense_limit=1 << 26, **kw):
    from mxstream.runtime.native_ops import NativeCounterRateOp

    op = NativeCounterRateOp(fn=_fn(**kw), key_pos=key_pos, device=device,
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
    the values are a running counter per key with a few resets, as longs or as doubles."""
    from mxstream.ops.native import load
    from mxstream.ops.text import FK_DOUBLE, FK_LONG, FK_STR
    from mxstream.runtime.columnar import ColumnBatch
    from mxstream.runtime.operators import WM, Rec

    rng = np.random.default_rng(seed)
    sd = load().StringDict()
    str_keys = mode in ("recs", "str")
    key = (lambda i: f"host{i}") if str_keys else (lambda i: int(i) * 3)
    counter = np.zeros(25, dtype=np.int64)
    now = 1_000
    for _ in range(passes):
        items = []
        for _ in range(int(rng.integers(1, 5))):
            n = int(rng.integers(1, 40))
            ks = rng.integers(0, 25, n)
            tsa = (now + rng.integers(-20, 20, n)).astype(np.int64)
            vals = np.empty(n, dtype=np.int64)
            for i, k in enumerate(ks):
                counter[k] = 3 if rng.random() < 0.03 else counter[k] + int(rng.integers(0, 900))
                vals[i] = counter[k]
            vals = vals if ints else vals * 0.1
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


@pytest.mark.parametrize("ruled", [False, True])
@pytest.mark.parametrize("mode,ints", [("recs", False), ("str", False), ("int", False),
                                       ("recs", True), ("int", True)])
def test_native_operator_equals_the_host_operator(mode, ints, ruled):
    from mxstream.ops.text import FK_DOUBLE, FK_LONG, FK_STR
    from mxstream.runtime.columnar import ColumnBatch, expand_columns
    from mxstream.runtime.operators import WM

    kw = dict(per=7, when=">", threshold=300.0 if ints else 30.0, max_gap=60) if ruled else {}
    native, host = _native(**kw), _host(**kw)
    rows = 0
    for items in list(_passes(17, mode, ints=ints)) + [[WM(K.I64_MAX)]]:
        got, want = native.process(list(items)), host.process(expand_columns(list(items)))
        assert all(isinstance(it, (ColumnBatch, WM)) for it in got)
        # the host operator emits a record's rows at the record; the native one before the
        # watermark that follows: the same rows in the same order between the same watermarks
        assert _lines(got) == _lines(want)
        for cb in got:
            if isinstance(cb, ColumnBatch):
                assert cb.kinds == (FK_STR if mode != "int" else FK_LONG, FK_DOUBLE,
                                    FK_LONG if ints else FK_DOUBLE, FK_LONG)
                rows += cb.n
    assert native.fallback is None and native.op is not None and rows >= 50
    assert native.out_of_order == host.fn.out_of_order > 10
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
        # a key's counter is of one kind: the host operator raises at the second sample
        "mixed_values": (lambda: [_rec(Tuple2("a", 80.0)), _rec(Tuple2("a", 60), 60)], TypeError),
        # two keys of two kinds are two counters on the host path
        "mixed_values_of_two_keys": (
            lambda: [_rec(Tuple2("a", 80.0)), _rec(Tuple2("c", 60), 60),
                     _rec(Tuple2("a", 90.0), 70), _rec(Tuple2("c", 70), 80)], None),
        "mixed_value_columns": (
            lambda: _column_batch((FK_LONG, FK_DOUBLE), [[3, 3], [80.0, 91.0]], (5, 50))
            + _column_batch((FK_LONG, FK_LONG), [[4, 4], [80, 90]], (60, 70)), None),
        "key_at_dense_limit": (lambda: [_rec(Tuple2(100, 80.0)), _rec(Tuple2(100, 91.0), 50)],
                               None),
        "no_timestamp": (lambda: [_rec(Tuple2("a", 80.0), K.I64_MIN)], ValueError),
        "timestamp_at_2_62": (lambda: [_rec(Tuple2("a", 80.0), 0), _rec(Tuple2("a", 91.0), big)],
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
    kw = dict(per=7, max_gap=80)
    passes = list(_passes(23, "str", passes=10))
    ref, op = _native(**kw), _native(**kw)
    want = [_lines(ref.process(list(p))) for p in passes]
    assert sum(len(w) for w in want) > 100
    for i, p in enumerate(passes):
        if i == 5:
            snap = op.snapshot()
            assert snap["counter_rate"] == _fn(**kw).native
            assert snap["engine"]["meta"]["kind"] == "counter_rate"
            assert snap["engine"]["meta"]["out_of_order"] == op.out_of_order > 5
            assert snap["engine"]["meta"]["value_kind"] == K.SUSTAIN_DOUBLE
            assert snap["engine"]["columns"]["key"].size >= 10
            op = _native(**kw)
            op.restore(snap)
        assert _lines(op.process(list(p))) == want[i]
    assert op.out_of_order == ref.out_of_order
    others = (dict(per=8, max_gap=80), dict(per=7), dict(per=7, max_gap=81),
              dict(per=7, max_gap=80, when="<", threshold=1.0), dict(kw, field=0))
    for other in others:
        with pytest.raises(ValueError, match="checkpoint of a different counter-rate function"):
            _native(**other).restore(snap)
    _native(per=Time.milliseconds(7), max_gap=Time.milliseconds(80)).restore(snap)
    ordered = _native(**kw)
    ordered.ordered = True
    with pytest.raises(ValueError, match="without event-time order"):
        ordered.restore(snap)
    with pytest.raises(RuntimeError, match="pending"):
        op.pending.append(_rec(Tuple2("a", 1.0)))
        op.snapshot()


def test_several_ranks_fall_back_in_open():
    from mxstream.runtime.native_ops import NativeCounterRateOp

    class Comm:
        world = 2

    ctx = _ctx()
    ctx.comm = Comm()
    op = NativeCounterRateOp(fn=_fn(), key_pos=0, device="cpu", fallback_factory=_host)
    op.open(ctx)
    assert op.fallback is not None and op.op is None


# ---- GPU ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_job_equals_the_host_path(gpu_device, route):
    host = _job(_rate(HostRate))
    got = _job(_rate(), device="cuda")
    assert _routes(route) == {"built": 1, "fallback": 0}
    assert got == host and len(got) > 300
    floats = _samples(False)
    got = _job(_rate(**RULE), device="cuda", samples=floats)
    assert got == _job(_rate(HostRate, **RULE), samples=floats) and len(got) > 5


@pytest.mark.gpu
def test_gpu_native_operator_takes_device_batches_and_restores(gpu_device):
    import torch

    from mxstream.ops.text import FK_DOUBLE, FK_LONG
    from mxstream.runtime.columnar import DeviceColumnBatch, expand_columns
    from mxstream.runtime.operators import WM

    def dev(a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(gpu_device)

    kw = dict(per=7, max_gap=90)
    native, host = _native(device=gpu_device, **kw), _host(**kw)
    rng = np.random.default_rng(4)
    counter = np.zeros(60)
    rows = 0
    for step in range(6):
        n = 500
        keys = rng.integers(0, 60, n).astype(np.int64)
        ts = (1_000 + 40 * step + rng.integers(-20, 20, n)).astype(np.int64)
        vals = np.empty(n)
        for i, k in enumerate(keys):
            counter[k] = 0.3 if rng.random() < 0.03 else counter[k] + rng.integers(0, 900) * 0.1
            vals[i] = counter[k]
        cb = DeviceColumnBatch(n, [dev(keys, torch.int64), dev(vals, torch.float64)],
                               (FK_LONG, FK_DOUBLE), None, dev(ts, torch.int64), parallelism=4)
        items = [cb, WM(1_000 + 40 * step)]
        if step == 3:
            snap = native.snapshot()
            native = _native(device=gpu_device, **kw)
            native.restore(snap)
        got = _lines(native.process(list(items)))
        assert got == _lines(host.process(expand_columns(list(items))))
        rows += len(got) - 1
    assert native.fallback is None and native.op.device.type == "cuda" and rows > 50
    assert native.out_of_order == host.fn.out_of_order > 100
