"""``stream.key_by(0).process(EventTimeOrdered(rule))`` (api/functions.py): what the wrapper
changes on a disordered stream, the job on the native operators (the device reorder buffer in
front of the rule) against the host KeyedProcessOp, the planner's choice, fallbacks and
checkpoints."""
from __future__ import annotations

from collections import Counter

import numpy as np
import pytest
import torch

from mxstream.api import functions as F
from mxstream.api.time import Time
from mxstream.api.tuples import Tuple2, Tuple3
from mxstream.ops import kernels as K

B, Q = 95.0, 40.0   # a breaching and a quiet value under "> 90"


def _ctx():
    from mxstream.runtime.operators import OpContext

    return OpContext("ordered", 4, 128, lambda: 0, "EventTime")


def _host(fn, key_pos=0):
    from mxstream.runtime.operators import KeyedProcessOp

    op = KeyedProcessOp(lambda v: v[key_pos], fn)
    op.open(_ctx())
    return op


def _sustained(cls=F.SustainedAlert, threshold=90.0, for_=5, field=1):
    return cls(field, ">", threshold, for_)


def _burst(cls=F.BurstAlert, threshold=90.0, times=3, within=25, field=1):
    return cls(field, ">", threshold, times, within)


RULES = {"sustained": _sustained, "burst": _burst}


def _native(rule="sustained", ordered=True, key_pos=0, device="cpu", **kw):
    from mxstream.runtime.native_ops import NativeBurstOp, NativeSustainOp

    make = RULES[rule]
    rule_kw = {k: kw.pop(k) for k in ("threshold", "for_", "times", "within", "field") if k in kw}
    fn = make(**rule_kw)
    wrap = (lambda f: F.EventTimeOrdered(f)) if ordered else (lambda f: f)
    op = (NativeSustainOp if rule == "sustained" else NativeBurstOp)(
        fn=fn, key_pos=key_pos, device=device, ordered=ordered,
        fallback_factory=lambda: _host(wrap(make(**rule_kw)), key_pos), **kw)
    op.open(_ctx())
    return op


def _lines(items) -> list:
    """Output as the watermarks and the (text, ts, subtask) rows, in order."""
    from mxstream.runtime.columnar import expand_columns
    from mxstream.runtime.operators import WM

    return [it if isinstance(it, WM) else (str(it.value), it.ts, it.subtask)
            for it in expand_columns(list(items))]


def _rec(value, ts):
    from mxstream.runtime.operators import Rec

    return Rec(value, ts, 0)


# ---- the wrapper matters ---------------------------------------------------------------------
def _straggler_stream():
    """Key "a" breaches at 10, 20 and 30; its quiet sample of 15 straggles in behind them. "b" is
    in order. After the watermark 36 a sample of 33 is late."""
    from mxstream.runtime.operators import WM

    return [_rec(Tuple2("a", B), 10), _rec(Tuple2("b", B), 12), _rec(Tuple2("a", B), 20),
            _rec(Tuple2("a", B), 30), _rec(Tuple2("a", Q), 15), _rec(Tuple2("b", B), 22),
            WM(16), _rec(Tuple2("a", B), 36), _rec(Tuple2("b", Q), 31), WM(36),
            _rec(Tuple2("a", B), 41), _rec(Tuple2("a", B), 41), _rec(Tuple2("a", Q), 33),
            _rec(Tuple2("a", Q), 38), WM(K.I64_MAX)]


def _presorted(items) -> list:
    """The records that are not late, sorted by (ts, arrival), in front of the last watermark."""
    from mxstream.runtime.operators import WM

    wm, recs = K.I64_MIN, []
    for it in items:
        if isinstance(it, WM):
            wm = it.ts
        elif it.ts > wm:
            recs.append(it)
    return sorted(recs, key=lambda r: r.ts) + [items[-1]]   # (sorted() is stable)


def _rows(lines) -> list:
    return [ln for ln in lines if isinstance(ln, tuple)]


def test_a_straggler_splits_a_run_in_arrival_order_and_not_in_event_time_order():
    items = _straggler_stream()
    plain = _rows(_lines(_host(_sustained()).process(list(items))))
    # arrival order: the quiet sample of 15 arrives after the breach of 30: a resolve, a re-fire
    assert [(v, t) for v, t, _ in plain if v.startswith("(a")] == [
        ("(a,1,10,95.0)", 20), ("(a,0,10,40.0)", 15), ("(a,1,36,95.0)", 41),
        ("(a,0,36,40.0)", 33)]
    fn = F.EventTimeOrdered(_sustained())
    ordered = _rows(_lines(_host(fn).process(list(items))))
    want = _rows(_lines(_host(_sustained()).process(_presorted(items))))
    assert sorted(ordered) == sorted(want) and fn.late_dropped == 1
    for key in ("(a", "(b"):
        assert [r for r in ordered if r[0].startswith(key)] == \
            [r for r in want if r[0].startswith(key)]
    # event time: 15 closes the run of 10 before it fired; the run of 20 fires at 30 and is
    # resolved by 38 (33 is late); rows carry their element's timestamp, not the timer's
    assert [(v, t) for v, t, _ in ordered if v.startswith("(a")] == [
        ("(a,1,20,95.0)", 30), ("(a,0,20,40.0)", 38)]
    assert [(v, t) for v, t, _ in ordered if v.startswith("(b")] == [
        ("(b,1,12,95.0)", 22), ("(b,0,12,40.0)", 31)]


def test_a_straggler_fakes_a_burst_in_arrival_order_and_not_in_event_time_order():
    from mxstream.runtime.operators import WM

    # three breaches within 25 ms need 10, 20, 30; in event time the third is 50 ms away
    items = [_rec(Tuple2("a", B), 10), _rec(Tuple2("a", B), 20), _rec(Tuple2("a", B), 80),
             _rec(Tuple2("a", B), 30), _rec(Tuple2("a", Q), 35), WM(40),
             _rec(Tuple2("a", B), 90), _rec(Tuple2("a", B), 85), _rec(Tuple2("a", Q), 39),
             WM(K.I64_MAX)]
    plain = _rows(_lines(_host(_burst()).process(list(items))))
    # arrival order: 80 - 10 is not dense, but 30 - 20 = 10 with (20, 80, 30) held is; 85 - 30
    # with (30, 90, 85) held ends a burst that never was
    assert [(v, t) for v, t, _ in plain] == [("(a,1,20,95.0)", 30), ("(a,0,20,95.0)", 85)]
    fn = F.EventTimeOrdered(_burst())
    ordered = _rows(_lines(_host(fn).process(list(items))))
    assert ordered == _rows(_lines(_host(_burst()).process(_presorted(items))))
    assert fn.late_dropped == 1
    assert [(v, t) for v, t, _ in ordered] == [
        ("(a,1,10,95.0)", 30), ("(a,0,10,95.0)", 80), ("(a,1,80,95.0)", 90)]


def test_refusals_and_the_native_spec():
    fn = F.EventTimeOrdered(F.SustainedAlert(2, ">", 90.0, Time.minutes(5)))
    assert fn.native == ("event_time_ordered", "sustained", 2, ">", 90.0, 300_000)
    assert F.EventTimeOrdered(_burst()).native == ("event_time_ordered", "burst", 1, ">", 90.0, 3,
                                                   25)
    assert isinstance(fn, F.KeyedProcessFunction) and fn.late_dropped == 0

    class Quiet(F.KeyedProcessFunction):
        def process_element(self, value, ctx, out):
            out.collect(value)

    assert not hasattr(F.EventTimeOrdered(Quiet()), "native")

    class Timed(Quiet):
        def on_timer(self, timestamp, ctx, out):
            pass

    for bad in (F.CountWithTimeout(5), Timed(), fn, lambda v: v, None, F.MapFunction()):
        with pytest.raises(ValueError, match="EventTimeOrdered"):
            F.EventTimeOrdered(bad)

    class Arms(F.KeyedProcessFunction):
        def process_element(self, value, ctx, out):
            ctx.timer_service().register_event_time_timer(ctx.timestamp() + 1)

    from mxstream.runtime.operators import WM

    op = _host(F.EventTimeOrdered(Arms()))
    op.process([_rec(Tuple2("a", B), 5)])
    with pytest.raises(RuntimeError, match="timer service"):
        op.process([WM(5)])
    with pytest.raises(ValueError, match="EventTimeOrdered: a record without an event timestamp"):
        _host(F.EventTimeOrdered(Quiet())).process([_rec(Tuple2("a", B), K.I64_MIN)])
    # any wrapped function: its output carries the element's timestamp and key
    op = _host(F.EventTimeOrdered(Quiet()))
    got = _lines(op.process([_rec(Tuple2("a", 2.0), 7), _rec(Tuple2("a", 1.0), 3), WM(9)]))
    assert [(v, t) for v, t, _ in got[:-1]] == [("(a,1.0)", 3), ("(a,2.0)", 7)]


# ---- native against the host operator -----------------------------------------------------------
def _passes(seed, mode, passes=14, ints=False):
    """Passes of records ("recs"), column batches ("str" / "int" keys) or both, with watermarks
    that run up to 60 ms behind rows disordered by +-20 ms: some rows are late. Values ~
    base[key] + N(0, 8) around the threshold 70."""
    from mxstream.ops.native import load
    from mxstream.ops.text import FK_DOUBLE, FK_LONG, FK_STR
    from mxstream.runtime.columnar import ColumnBatch
    from mxstream.runtime.operators import WM

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
                items.extend(_rec(Tuple2(key(k), v), int(t))
                             for k, v, t in zip(ks, vals.tolist(), tsa))
            if rng.integers(0, 2):
                items.append(WM(now - int(rng.integers(0, 60))))
        yield items


def _segments(lines) -> list:
    """[(rows up to a watermark, the watermark)], the rest with None."""
    segs, cur = [], []
    for ln in lines:
        if isinstance(ln, tuple):
            cur.append(ln)
        else:
            segs.append((cur, ln))
            cur = []
    return segs + [(cur, None)]


def _key_of(row) -> str:
    return row[0][1:row[0].index(",")]


def _equal_up_to_the_order_across_keys(got, want):
    """The same watermarks; between two of them the same rows, every key's in the same order, the
    native ones in timestamp order."""
    gs, ws = _segments(got), _segments(want)
    assert [w for _, w in gs] == [w for _, w in ws]
    for (g, _), (w, _) in zip(gs, ws):
        assert Counter(g) == Counter(w)
        for key in {_key_of(r) for r in w}:
            assert [r for r in g if _key_of(r) == key] == [r for r in w if _key_of(r) == key]
        assert [r[1] for r in g] == sorted(r[1] for r in g)


@pytest.mark.parametrize("rule", sorted(RULES))
@pytest.mark.parametrize("mode,ints", [("recs", False), ("str", False), ("int", False),
                                       ("int", True)])
def test_native_operator_equals_the_host_operator(rule, mode, ints):
    from mxstream.runtime.columnar import ColumnBatch, expand_columns
    from mxstream.runtime.operators import WM

    kw = dict(threshold=70.0, **({"for_": 60} if rule == "sustained" else {"within": 120}))
    native = _native(rule, **kw)
    fn = F.EventTimeOrdered(RULES[rule](**kw))
    host = _host(fn)
    rows = codes = 0
    for items in list(_passes(17, mode, ints=ints)) + [[WM(K.I64_MAX)]]:
        got, want = native.process(list(items)), host.process(expand_columns(list(items)))
        assert all(isinstance(it, (ColumnBatch, WM)) for it in got)
        _equal_up_to_the_order_across_keys(_lines(got), _lines(want))
        for cb in got:
            if isinstance(cb, ColumnBatch):
                rows += cb.n
                codes += int((cb.cols[1] == 0).sum())
    assert native.fallback is None and native.op is not None and native.buf is not None
    assert rows >= 20 and 0 < codes < rows
    assert native.num_late_records_dropped == fn.late_dropped > 0
    assert native.buf.rows_buffered == 0 and native.finish() == host.finish() == []


@pytest.mark.parametrize("rule", sorted(RULES))
def test_native_operator_is_the_twin_buffer_followed_by_the_twin_rule(rule):
    """Order included: integer keys are their own ids."""
    from mxstream.runtime.burst_operator import KeyedBurstOperator
    from mxstream.runtime.columnar import expand_columns
    from mxstream.runtime.operators import WM
    from mxstream.runtime.reorder_operator import EventOrderBuffer
    from mxstream.runtime.sustain_operator import KeyedSustainOperator

    kw = dict(threshold=70.0, **({"for_": 60} if rule == "sustained" else {"within": 120}))
    native = _native(rule, **kw)
    buf = EventOrderBuffer()
    eng = (KeyedSustainOperator(">", 70.0, 60) if rule == "sustained"
           else KeyedBurstOperator(">", 70.0, 3, 120))
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64))  # noqa: E731
    total = 0
    for items in list(_passes(29, "int")) + [[WM(K.I64_MAX)]]:
        want, pend = [], []

        def flush():
            if pend:
                buf.push(T([r.value[0] for r in pend]), T([r.ts for r in pend]),
                         T(np.array([r.value[1] for r in pend], dtype=np.float64).view(np.int64)))
                pend.clear()

        for it in expand_columns(list(items)):
            if not isinstance(it, WM):
                pend.append(it)
                continue
            flush()
            cols = buf.release(it.ts)
            if cols is not None:
                for ch in eng.process(cols[0], cols[2], cols[1]):
                    key, code, since, val, ts = (c.numpy() for c in ch)
                    want.extend((f"({k},{c},{s},{v})", t) for k, c, s, v, t in zip(
                        key.tolist(), code.tolist(), since.tolist(),
                        val.view(np.float64).tolist(), ts.tolist()))
            want.append(it)
        flush()
        got = [ln if isinstance(ln, WM) else ln[:2] for ln in _lines(native.process(list(items)))]
        assert got == want
        total += len(got)
    assert total > 40 and buf.metrics == native.buf.metrics
    assert native.num_late_records_dropped == buf.metrics.num_late_records_dropped > 0


# ---- the job ---------------------------------------------------------------------------------
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


def _samples():
    """Five hosts report every 10 s for 15 min; host1 breaches from 100 s to 300 s, host3 twice in
    a row every 80 s, host4 from 700 s on. Every 7th sample arrives 25 s late -- behind the two
    samples that follow it, inside the 30 s bound -- and every 31st 70 s late, beyond it."""
    events = []
    for i in range(450):
        h, j = i % 5, i // 5
        t = j * 10_000 + h * 7
        usage = 40.0 + (i % 7)
        if h == 1 and 100_000 <= t < 300_000:
            usage = 97.0
        if h == 3 and j % 8 < 2:
            usage = 91.0 + (i % 3)
        if h == 4 and t >= 700_000:
            usage = 93.0
        arrival = t + (70_000 if i % 31 == 5 else 25_000 if i % 7 == 3 else 0)
        events.append((arrival, i, (f"host{h}", usage, t)))
    return [(a + 10, e) for a, _, e in sorted(events)]


SAMPLES = _samples()


class HostOrdered(F.EventTimeOrdered):
    """A subclass keeps the host path: the planner lowers exactly EventTimeOrdered."""


class HostAlert(F.SustainedAlert):
    """A subclass of the rule: the wrapper around it keeps the host path too."""


def first(v):
    return v[0]


def _job(fn, native="auto", device="cpu", key=0):
    from mxstream.api.watermarks import BoundedOutOfOrdernessTimestampExtractor

    env, out = _env(native, device=device)
    env.from_timed_collection(SAMPLES) \
        .assign_timestamps_and_watermarks(BoundedOutOfOrdernessTimestampExtractor(
            Time.seconds(30), extractor=lambda e: e[2])) \
        .map(lambda e: Tuple3(e[0], "cpu", e[1])).key_by(key) \
        .process(fn).print()
    env.execute("ordered-usage")
    return out


def _job_rule(name):
    return (F.SustainedAlert(2, ">", 90.0, Time.seconds(20)) if name == "sustained"
            else F.BurstAlert(2, ">", 90.0, 3, Time.seconds(25)))


@pytest.fixture
def route(monkeypatch):
    from mxstream.runtime.native_ops import NativeSustainOp
    from mxstream.runtime.reorder_operator import EventOrderBuffer

    seen = {"buffers": 0, "fallback": 0, "ops": []}
    init, to_fb, op_init = (EventOrderBuffer.__init__, NativeSustainOp._to_fallback,
                            NativeSustainOp.__init__)

    def spy_init(self, *a, **kw):
        seen["buffers"] += 1
        init(self, *a, **kw)

    def spy_fb(self):
        seen["fallback"] += 1
        to_fb(self)

    def spy_op(self, *a, **kw):
        seen["ops"].append(self)
        op_init(self, *a, **kw)

    monkeypatch.setattr(EventOrderBuffer, "__init__", spy_init)
    monkeypatch.setattr(NativeSustainOp, "_to_fallback", spy_fb)
    monkeypatch.setattr(NativeSustainOp, "__init__", spy_op)
    return seen


def _job_agrees(rule, route, device):
    def per_key(lines):
        rows = [ln[ln.index("("):] for ln in lines]
        return {k: [r for r in rows if r.startswith(f"({k},")] for k in
                {r[1:r.index(",")] for r in rows}}

    host_fn = HostOrdered(_job_rule(rule))
    host = _job(host_fn)
    assert (route["buffers"], route["fallback"], route["ops"]) == (0, 0, [])
    assert host_fn.late_dropped >= 5 and len(host) >= 3
    assert Counter(_job(F.EventTimeOrdered(_job_rule(rule)), "off")) == Counter(host)
    assert route["buffers"] == 0
    native = _job(F.EventTimeOrdered(_job_rule(rule)), device=device)
    assert (route["buffers"], route["fallback"], len(route["ops"])) == (1, 0, 1)
    op = route["ops"][0]
    assert op.ordered and op.buf is not None and op.buf.device.type == device
    assert Counter(native) == Counter(host) and per_key(native) == per_key(host)
    assert op.num_late_records_dropped == host_fn.late_dropped
    # the wrapper matters on this stream: the plain rule reports other rows
    assert Counter(ln[ln.index("("):] for ln in _job(_job_rule(rule))) != \
        Counter(ln[ln.index("("):] for ln in host)


@pytest.mark.parametrize("rule", sorted(RULES))
def test_job_native_on_cpu_equals_the_host_path(rule, route):
    _job_agrees(rule, route, "cpu")


def test_the_planner_lowers_the_two_rules_and_nothing_else():
    from mxstream.api import planner
    from mxstream.runtime.native_ops import NativeBurstOp, NativeSustainOp
    from mxstream.runtime.operators import KeyedProcessOp

    class Comm:
        world, rank = 2, 0

    class Quiet(F.KeyedProcessFunction):
        def process_element(self, value, ctx, out):
            pass

    O = F.EventTimeOrdered
    ops = {}
    for name, fn, key, world in (
            ("sustained", O(_sustained()), 0, 1), ("burst", O(_burst()), 0, 1),
            ("times_16", O(_burst(times=16)), 0, 1), ("times_17", O(_burst(times=17)), 0, 1),
            ("sub", HostOrdered(_sustained()), 0, 1), ("rule_sub", O(_sustained(HostAlert)), 0, 1),
            ("selector", O(_sustained()), first, 1), ("ranks", O(_sustained()), 0, 2),
            ("other", O(Quiet()), 0, 1), ("plain", _sustained(), 0, 1)):
        env, _ = _env()
        if world > 1:
            env._comm = Comm()
        s = env.from_collection([("a", 1.0)]).key_by(key).process(fn)
        assert s.t.meta["kind"] == "keyed_process" and s.t.meta["fn"] is fn
        planner._lower_keyed_process(env, s.t, s.t.meta)
        op = s.t.factory()
        ops[name] = (type(op), bool(s.t.meta.get("native")), getattr(op, "ordered", None))
        if name in ("sustained", "burst"):
            assert op.fn_spec == fn.fn.native
            fb = op.fallback_factory()
            assert type(fb) is KeyedProcessOp and fb.fn is fn   # the host wrapper
    assert ops["sustained"] == (NativeSustainOp, True, True)
    assert ops["burst"] == ops["times_16"] == (NativeBurstOp, True, True)
    assert ops["plain"] == (NativeSustainOp, True, False)
    for name in ("times_17", "sub", "rule_sub", "selector", "ranks", "other"):
        assert ops[name] == (KeyedProcessOp, False, None), name
    with pytest.raises(ValueError, match="does not override on_timer"):
        O(F.CountWithTimeout(Time.seconds(60)))


def test_subclasses_and_selector_keys_keep_the_host_operator(route):
    host = _job(HostOrdered(_job_rule("sustained")))
    assert _job(F.EventTimeOrdered(_job_rule("sustained")), key=first) == host
    assert _job(F.EventTimeOrdered(HostAlert(2, ">", 90.0, Time.seconds(20)))) == host
    assert (route["buffers"], route["fallback"], route["ops"]) == (0, 0, [])


def test_records_without_timestamps_raise_on_both_paths():
    from mxstream.runtime.executor import JobExecutionException

    for fn, native in ((F.EventTimeOrdered(_sustained()), "auto"),
                       (HostOrdered(_sustained()), "auto"),
                       (F.EventTimeOrdered(_sustained()), "off")):
        env, _ = _env(native)
        env.from_collection([("a", 95.0)]).key_by(0).process(fn).print()
        with pytest.raises(JobExecutionException, match="ValueError: EventTimeOrdered: a record "
                                                        "without an event timestamp") as e:
            env.execute("no-timestamps")
        assert isinstance(e.value.__cause__, ValueError)


# ---- fallbacks ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["text_value", "mixed_values", "double_key", "timestamp_at_2_62"])
def test_unsupported_data_falls_back_before_state_exists_and_raises_after(case):
    from mxstream.runtime.columnar import expand_columns
    from mxstream.runtime.operators import WM

    make = {"text_value": lambda: [_rec(Tuple2("a", "80"), 5)],
            "mixed_values": lambda: [_rec(Tuple2("a", 95.0), 5), _rec(Tuple2("a", 95), 60)],
            "double_key": lambda: [_rec(Tuple2(1.5, 95.0), 5)],
            "timestamp_at_2_62": lambda: [_rec(Tuple2("a", 95.0), 1 << 62),
                                          _rec(Tuple2("a", 96.0), 0)]}[case]
    tail = [WM(50), WM(K.I64_MAX)]
    op = _native(for_=0)
    assert op.process([WM(-7)]) == [WM(-7)] and op.buf is None and op.op is None
    if case == "text_value":
        with pytest.raises(TypeError):
            op.process(make() + tail)
        assert op.fallback is not None   # (the host wrapper met the value at the watermark 50)
    else:
        host = _host(F.EventTimeOrdered(_sustained(for_=0)))
        host.process([WM(-7)])
        got = op.process(make() + tail)
        assert op.fallback is not None and op.buf is None and op.op is None
        assert _lines(got) == _lines(host.process(expand_columns(make()) + tail))
        if case != "double_key":
            assert len(_rows(_lines(got))) >= 1
    # a buffer with rows and no rule state yet is native state: an error
    op = _native(for_=0)
    op.process([_rec(Tuple2(3 if case == "double_key" else "b", 95.0), 1)])
    assert op.buf is not None and op.buf.rows_buffered == 1 and op.op is None
    with pytest.raises(TypeError):
        op.process(make() + tail)
    assert op.fallback is None


# ---- checkpoints ---------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", sorted(RULES))
def test_checkpoint_in_mid_stream_gives_the_uninterrupted_output(rule):
    kw = dict(threshold=70.0, **({"for_": 60} if rule == "sustained" else {"within": 120}))
    passes = list(_passes(23, "str", passes=10))
    ref, op = _native(rule, **kw), _native(rule, **kw)
    want = [_lines(ref.process(list(p))) for p in passes]
    assert sum(len(w) for w in want) > 30
    for i, p in enumerate(passes):
        if i == 5:
            snap = op.snapshot()
            assert snap["ordered"] is True and snap["reorder"]["meta"]["kind"] == "reorder"
            assert snap["reorder"]["columns"]["key"].size >= 1   # rows are buffered across it
            assert snap["engine"]["columns"]["key"].size >= 1
            assert snap["late"] == snap["reorder"]["meta"]["late"]
            op = _native(rule, **kw)
            op.restore(snap)
            assert op.num_late_records_dropped == snap["late"]
        assert _lines(op.process(list(p))) == want[i]
    assert op.buf.metrics.num_late_records_dropped == ref.num_late_records_dropped > 0
    with pytest.raises(ValueError, match="event-time order"):
        _native(rule, ordered=False, **kw).restore(snap)
    plain = _native(rule, ordered=False, **kw)
    plain.process(list(passes[0]))
    assert "ordered" not in plain.snapshot() and "reorder" not in plain.snapshot()
    with pytest.raises(ValueError, match="event-time order"):
        _native(rule, **kw).restore(plain.snapshot())
    with pytest.raises(ValueError, match="different"):
        _native(rule, **{**kw, "threshold": 71.0}).restore(snap)


def test_checkpoint_with_buffered_rows_and_no_rule_state_yet():
    from mxstream.runtime.operators import WM

    first_pass = [_rec(Tuple2("a", B), 30), _rec(Tuple2("b", B), 10), _rec(Tuple2("a", B), 20)]
    rest = [WM(25), _rec(Tuple2("a", B), 22), _rec(Tuple2("a", Q), 40), WM(K.I64_MAX)]
    ref = _native(for_=5)
    assert ref.process(list(first_pass)) == []
    op = _native(for_=5)
    op.process(list(first_pass))
    assert op.op is None and op.buf.rows_buffered == 3
    snap = op.snapshot()
    assert "engine" not in snap and snap["ordered"] is True
    assert sorted(snap["reorder"]["columns"]["ts"].tolist()) == [10, 20, 30]
    fresh = _native(for_=5)
    fresh.restore(snap)
    assert fresh.op is None and fresh.buf.rows_buffered == 3 and fresh.str_keys is True
    want = _lines(ref.process(list(rest)))
    assert _lines(fresh.process(list(rest))) == want
    assert [v for v, _, _ in _rows(want)] == ["(a,1,20,95.0)", "(a,0,20,40.0)"]
    assert fresh.num_late_records_dropped == 1
    # an ordered operator that has seen nothing yet
    empty = _native().snapshot()
    assert empty["ordered"] is True and "reorder" not in empty and "engine" not in empty
    _native().restore(empty)


# ---- GPU ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("rule", sorted(RULES))
def test_gpu_job_equals_the_host_path(gpu_device, rule, route):
    _job_agrees(rule, route, "cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("rule", sorted(RULES))
def test_gpu_native_operator_takes_device_batches_and_restores(gpu_device, rule):
    from mxstream.ops.text import FK_DOUBLE, FK_LONG
    from mxstream.runtime.columnar import ColumnBatch, DeviceColumnBatch
    from mxstream.runtime.operators import WM

    def dev(a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(gpu_device)

    kw = dict(threshold=70.0, **({"for_": 60} if rule == "sustained" else {"within": 120}))
    native, twin = _native(rule, device=gpu_device, **kw), _native(rule, **kw)
    rng = np.random.default_rng(4)
    base = rng.uniform(50, 95, 60)
    rows = 0
    for step in range(8):
        n = 500
        keys = rng.integers(0, 60, n).astype(np.int64)
        ts = (1_000 + 40 * step + rng.integers(-100, 100, n)).astype(np.int64)   # some are late
        vals = np.round(base[keys] + rng.normal(0, 8, n), 1)
        cb = DeviceColumnBatch(n, [dev(keys, torch.int64), dev(vals, torch.float64)],
                               (FK_LONG, FK_DOUBLE), None, dev(ts, torch.int64), parallelism=4)
        hb = ColumnBatch(n, [keys, vals], (FK_LONG, FK_DOUBLE), None, ts, np.zeros(n, np.int32))
        wm = WM(K.I64_MAX if step == 7 else 1_000 + 40 * step - 30)
        if step == 3:
            snap = native.snapshot()
            assert snap["reorder"]["columns"]["key"].size > 0
            native = _native(rule, device=gpu_device, **kw)
            native.restore(snap)
        got = _lines(native.process([cb, wm]))
        assert got == _lines(twin.process([hb, wm]))
        rows += len(got) - 1
    assert native.fallback is None and native.buf.device.type == "cuda" and rows > 50
    assert native.op.device.type == "cuda"
    assert native.num_late_records_dropped == twin.num_late_records_dropped > 0
