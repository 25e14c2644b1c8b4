"""``stream.key_by(0).process(BurstAlert(field, when, threshold, times, within))``
(api/functions.py): the job on the native operator against the host KeyedProcessOp (a subclass,
native off, a key selector), the planner's choice, NativeBurstOp's fallbacks and its
checkpoints."""
from __future__ import annotations

import numpy as np
import pytest

from mxstream.api import functions as F
from mxstream.api.time import Time
from mxstream.api.tuples import Tuple1, Tuple2, Tuple3
from mxstream.ops import kernels as K


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
    """Five hosts report every 10 s for 15 min. host1 flaps: above 90 % at every other sample
    from 100 s to 300 s, never twice in a row; host2 spikes for single samples 90 s apart; host3
    breaches twice in a row every 80 s; host4 goes up at 700 s and stays there."""
    events = []
    for i in range(450):
        h, j = i % 5, i // 5
        t = j * 10_000 + h * 7
        usage = 40.0 + (i % 7)
        if h == 1 and 100_000 <= t < 300_000 and j % 2 == 0:
            usage = 97.0
        if h == 2 and j % 9 == 0:
            usage = 99.5
        if h == 3 and j % 8 < 2:
            usage = 91.0 + (i % 3)
        if h == 4 and t >= 700_000:
            usage = 93.0
        events.append((f"host{h}", usage, t))
    return events


SAMPLES = _samples()


class HostAlert(F.BurstAlert):
    """A subclass keeps the host path: the planner lowers exactly BurstAlert."""


def first(v):
    """A key selector: the planner cannot see that it is field 0."""
    return v[0]


def _job(fn, native="auto", device="cpu", key=0):
    from mxstream.api.watermarks import BoundedOutOfOrdernessTimestampExtractor

    env, out = _env(native, device=device)
    env.from_timed_collection([(e[2] + 10, e) for e in SAMPLES]) \
        .assign_timestamps_and_watermarks(BoundedOutOfOrdernessTimestampExtractor(
            Time.milliseconds(0), extractor=lambda e: e[2])) \
        .map(lambda e: Tuple3(e[0], "cpu", e[1])).key_by(key) \
        .process(fn).print()
    env.execute("flapping-usage")
    return out


def _rule(cls=F.BurstAlert, times=3, within=Time.minutes(1)):
    return cls(2, ">", 90.0, times, within)


def _expected(times: int, within_ms: int) -> list:
    state, out = {}, []
    for host, usage, t in SAMPLES:
        recent, since, firing = state.get(host, ((), None, False))
        breach = usage > 90.0
        if breach:
            recent = (recent + (t,))[-times:]
        dense = len(recent) == times and t - recent[0] <= within_ms
        if breach and dense and not firing:
            since, firing = recent[0], True
            out.append(f"({host},1,{since},{usage})")
        elif not dense and firing:
            out.append(f"({host},0,{since},{usage})")
            firing = False
        state[host] = (recent, since, firing)
    return out


@pytest.fixture
def route(monkeypatch):
    from mxstream.runtime.burst_operator import KeyedBurstOperator
    from mxstream.runtime.native_ops import NativeBurstOp

    seen = {"built": 0, "fallback": 0}
    init, to_fb = KeyedBurstOperator.__init__, NativeBurstOp._to_fallback

    def spy_init(self, *a, **kw):
        seen["built"] += 1
        init(self, *a, **kw)

    def spy_fb(self):
        seen["fallback"] += 1
        to_fb(self)

    monkeypatch.setattr(KeyedBurstOperator, "__init__", spy_init)
    monkeypatch.setattr(NativeBurstOp, "_to_fallback", spy_fb)
    return seen


def test_usage_job_native_on_cpu_equals_the_host_path(route):
    host = _job(_rule(HostAlert))
    assert route == {"built": 0, "fallback": 0}
    rows = [ln[ln.index("("):] for ln in host]
    assert rows == _expected(3, 60_000)
    # host1's flapping is two lines -- its third breach, and the first sample more than a minute
    # behind the third from last --, host2's spikes and host3's pairs none, host4 never ends
    assert rows == ["(host1,1,100007,97.0)", "(host1,0,100007,42.0)", "(host4,1,700028,93.0)"]
    assert _job(_rule(), "off") == host
    assert route == {"built": 0, "fallback": 0}
    native = _job(_rule())
    assert route == {"built": 1, "fallback": 0}
    assert native == host and len({ln[0] for ln in native}) > 1   # several subtasks print
    assert _job(_rule(within=60_000)) == host
    # the flapping host never breaches twice in a row: SustainedAlert stays silent on it
    assert not any("host1" in ln for ln in _job(F.SustainedAlert(2, ">", 90.0, 10_000)))


def test_edge_triggered_rule_prints_one_line_per_burst(route):
    host = _job(_rule(HostAlert, 2, Time.seconds(10)))
    native = _job(_rule(times=2, within=Time.seconds(10)))
    assert route == {"built": 1, "fallback": 0}
    assert native == host
    rows = [ln[ln.index("("):] for ln in host]
    assert rows == _expected(2, 10_000)
    # every pair of host3: a line, and its end at the next sample (the last pair has none);
    # host4's twenty breaches in a row are one line
    assert sum(r.startswith("(host3,1,") for r in rows) == 12
    assert sum(r.startswith("(host3,0,") for r in rows) == 11
    assert [r for r in rows if r.startswith("(host4")] == ["(host4,1,700028,93.0)"]
    assert len(rows) == 24


def test_selector_keys_keep_the_host_operator(route):
    got = _job(_rule(), key=first)
    assert route == {"built": 0, "fallback": 0}
    assert got == _job(_rule(HostAlert))


def test_the_planner_lowers_only_the_exact_class_with_a_positional_key_on_one_rank():
    from mxstream.api import planner
    from mxstream.runtime.native_ops import NativeBurstOp, NativeSustainOp
    from mxstream.runtime.operators import KeyedProcessOp

    class Comm:
        world, rank = 2, 0

    ops = {}
    for name, fn, key, world in (("exact", _rule(), 0, 1), ("sub", _rule(HostAlert), 0, 1),
                                 ("selector", _rule(), first, 1), ("ranks", _rule(), 0, 2),
                                 ("times_16", _rule(times=16), 0, 1),
                                 ("times_17", _rule(times=17), 0, 1),
                                 ("sustained", F.SustainedAlert(2, ">", 90.0, 5), 0, 1)):
        env, _ = _env()
        if world > 1:
            env._comm = Comm()
        s = env.from_collection([("a", "b", 1.0)]).key_by(key).process(fn)
        assert s.t.meta["kind"] == "keyed_process" and s.t.meta["fn"] is fn
        planner._lower_keyed_process(env, s.t, s.t.meta)
        ops[name] = (type(s.t.factory()), bool(s.t.meta.get("native")))
    assert ops["exact"] == ops["times_16"] == (NativeBurstOp, True)
    assert ops["sub"] == ops["selector"] == ops["ranks"] == ops["times_17"] \
        == (KeyedProcessOp, False)
    assert ops["sustained"] == (NativeSustainOp, True)


def test_more_times_than_the_ring_holds_run_on_the_host_operator(route):
    got = _job(_rule(times=17, within=Time.minutes(5)))
    assert route == {"built": 0, "fallback": 0}
    assert [ln[ln.index("("):] for ln in got] == _expected(17, 300_000) \
        == ["(host4,1,700028,93.0)"]


def test_records_without_timestamps_raise_on_both_paths():
    from mxstream.runtime.executor import JobExecutionException

    for fn, native in ((_rule(), "auto"), (_rule(HostAlert), "auto"), (_rule(), "off")):
        env, _ = _env(native)
        env.from_collection([("a", "cpu", 95.0)]).key_by(0).process(fn).print()
        with pytest.raises(JobExecutionException, match="ValueError: BurstAlert: a record "
                                                        "without an event timestamp") as e:
            env.execute("no-timestamps")
        assert isinstance(e.value.__cause__, ValueError)


def test_constructor_validation():
    fn = F.BurstAlert(2, ">=", 500, 5, Time.seconds(10))
    assert (fn.field, fn.when, fn.threshold, fn.times, fn.within_ms) == (2, ">=", 500, 5, 10_000)
    assert fn.native == ("burst", 2, ">=", 500, 5, 10_000)
    assert F.BurstAlert(0, "!=", 7.5, 2, 0).native == ("burst", 0, "!=", 7.5, 2, 0)
    assert F.BurstAlert(0, ">", 1, 1000, (1 << 62) - 1).times == 1000
    assert isinstance(fn, F.KeyedProcessFunction)
    for when in (">", ">=", "<", "<=", "==", "!="):
        F.BurstAlert(1, when, 1, 2, 1)
    for bad in (-1, True, 1.5, "2", None):
        with pytest.raises(ValueError, match="field"):
            F.BurstAlert(bad, ">", 90.0, 2, 1)
    for bad in (None, "=>", "", 1, ["<"]):
        with pytest.raises(ValueError, match="when"):
            F.BurstAlert(2, bad, 90.0, 2, 1)
    for bad in (True, "90", None, [90.0]):
        with pytest.raises(TypeError, match="threshold"):
            F.BurstAlert(2, ">", bad, 2, 1)
    for bad in (1, 0, -3, True, 2.0, "2", None):
        with pytest.raises(ValueError, match="times"):
            F.BurstAlert(2, ">", 90.0, bad, 1)
    for bad in (-1, True, 1.5, "60", None, Time.seconds(-1), 1 << 62):
        with pytest.raises(ValueError, match="within"):
            F.BurstAlert(2, ">", 90.0, 2, bad)


def test_a_value_that_is_no_number_is_a_type_error_on_the_host_path():
    from mxstream.runtime.operators import Rec

    op = _host()
    for bad in ("97", True, None):
        with pytest.raises(TypeError, match="value"):
            op.process([Rec(Tuple2("a", bad), 5, 0)])


# ---- NativeBurstOp against the host operator ---------------------------------------------------
def _ctx():
    from mxstream.runtime.operators import OpContext

    return OpContext("burst", 4, 128, lambda: 0, "EventTime")


def _host(threshold=70.0, times=3, within=120, key_pos=0, field=1):
    from mxstream.runtime.operators import KeyedProcessOp

    op = KeyedProcessOp(lambda v: v[key_pos], F.BurstAlert(field, ">", threshold, times, within))
    op.open(_ctx())
    return op


def _native(threshold=70.0, times=3, within=120, key_pos=0, field=1, **kw):
    from mxstream.runtime.native_ops import NativeBurstOp

    op = NativeBurstOp(fn=F.BurstAlert(field, ">", threshold, times, within), key_pos=key_pos,
                       device=kw.pop("device", "cpu"),
                       fallback_factory=lambda: _host(threshold, times, within, key_pos, field),
                       **kw)
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
    values ~ base[key] + N(0, 8) around the threshold 70, as doubles or as longs."""
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
    rows = codes = 0
    for items in list(_passes(17, mode, ints=ints)) + [[WM(K.I64_MAX)]]:
        got, want = native.process(list(items)), host.process(expand_columns(list(items)))
        assert all(isinstance(it, (ColumnBatch, WM)) for it in got)
        # the host operator emits a record's rows at the record; the native one before the
        # watermark that follows: the same rows in the same order between the same watermarks
        assert _lines(got) == _lines(want)
        for cb in got:
            if isinstance(cb, ColumnBatch):
                assert cb.kinds == (FK_STR if mode != "int" else FK_LONG, FK_LONG, FK_LONG,
                                    FK_LONG if ints else FK_DOUBLE)
                rows += cb.n
                codes += int((cb.cols[1] == 0).sum())
    assert native.fallback is None and native.op is not None and rows >= 20 and 0 < codes < rows
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
        "non_tuple": (lambda: [_rec(["a", 80.0])], 0, None),
        "no_value_field": (lambda: [_rec(Tuple1("a"))], 0, IndexError),
        "no_key_field": (lambda: [_rec(Tuple2("a", 80.0))], 2, IndexError),
        "text_value": (lambda: [_rec(Tuple2("a", "80"))], 0, TypeError),
        "bool_value": (lambda: [_rec(Tuple2("a", True))], 0, TypeError),
        "mixed_values": (lambda: [_rec(Tuple2("a", 80.0)), _rec(Tuple2("a", 80), 60)], 0, None),
        "mixed_value_columns": (
            lambda: _column_batch((FK_LONG, FK_DOUBLE), [[3, 3], [80.0, 81.0]], (5, 50))
            + _column_batch((FK_LONG, FK_LONG), [[3, 3], [80, 10]], (60, 70)), 0, None),
        "double_key": (lambda: [_rec(Tuple2(1.5, 80.0))], 0, None),
        "double_key_column": (
            lambda: _column_batch((FK_DOUBLE, FK_DOUBLE), [[1.5, 1.5], [80.0, 81.0]], (5, 50)),
            0, None),
        "mixed_keys": (lambda: [_rec(Tuple2("a", 80.0)), _rec(Tuple2(3, 80.0))], 0, None),
        "negative_key": (lambda: [_rec(Tuple2(-1, 80.0))], 0, None),
        "key_at_dense_limit": (lambda: [_rec(Tuple2(100, 80.0)), _rec(Tuple2(100, 81.0), 50)],
                               0, None),
        "no_timestamp": (lambda: [_rec(Tuple2("a", 80.0), K.I64_MIN)], 0, ValueError),
        "timestamp_at_2_62": (lambda: [_rec(Tuple2("a", 80.0), big), _rec(Tuple2("a", 81.0), 0)],
                              0, None),
        "timestamp_at_minus_2_62": (lambda: [_rec(Tuple2("a", 80.0), 0),
                                             _rec(Tuple2("a", 81.0), -big)], 0, None),
    }


FALLBACKS = _fallbacks()


@pytest.mark.parametrize("case", sorted(FALLBACKS))
def test_unsupported_data_falls_back_before_state_exists_and_raises_after(case):
    from mxstream.runtime.columnar import expand_columns
    from mxstream.runtime.operators import WM

    make, key_pos, host_error = FALLBACKS[case]
    int_keys = case in ("negative_key", "key_at_dense_limit", "double_key_column",
                        "mixed_value_columns")
    good = [_rec(Tuple3(3, 80.0, 3) if int_keys else Tuple3("b", 80.0, "b"), 1)]
    tail = [WM(50), WM(K.I64_MAX)]
    rule = dict(times=2, within=100)
    # before native state exists: the host operator, told the watermark that was pending
    op = _native(key_pos=key_pos, dense_limit=100, **rule)
    assert op.process([WM(-7)]) == [WM(-7)] and op.op is None
    if host_error is not None:
        with pytest.raises(host_error):
            op.process(make() + tail)
        assert op.fallback is not None and op.op is None and op.fallback.wm == -7
    else:
        host = _host(key_pos=key_pos, **rule)
        host.process([WM(-7)])
        got = op.process(make() + tail)
        assert op.fallback is not None and op.op is None
        assert _lines(got) == _lines(host.process(expand_columns(make()) + tail))
        if case not in ("non_tuple", "double_key", "negative_key", "mixed_keys"):
            # two breaches within 100 ms, or in disorder: the burst was reported
            assert sum(not isinstance(x, WM) for x in _lines(got)) >= 1
    # afterwards: an error
    op = _native(key_pos=key_pos, dense_limit=100, **rule)
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
            assert snap["burst"] == ("burst", 1, ">", 70.0, 3, 120)
            assert snap["engine"]["meta"]["kind"] == "burst"
            cols = snap["engine"]["columns"]
            assert cols["key"].size >= 1 and cols["firing"].any()   # bursts are open across it
            assert (cols["held"] == 3).any() and (cols["held"] < 3).any()
            op = _native()
            op.restore(snap)
        assert _lines(op.process(list(p))) == want[i]
    for other in (dict(threshold=71.0), dict(threshold=70), dict(within=121), dict(times=4),
                  dict(field=0)):
        with pytest.raises(ValueError, match="different burst"):
            _native(**other).restore(snap)
    from mxstream.runtime.native_ops import NativeBurstOp, NativeSustainOp

    lt = NativeBurstOp(fn=F.BurstAlert(1, "<", 70.0, 3, 120), key_pos=0, device="cpu",
                       fallback_factory=_host)
    lt.open(_ctx())
    with pytest.raises(ValueError, match="different burst"):
        lt.restore(snap)
    sustained = NativeSustainOp(fn=F.SustainedAlert(1, ">", 70.0, 120), key_pos=0, device="cpu",
                                fallback_factory=_host)
    sustained.open(_ctx())
    with pytest.raises(ValueError, match="different sustained"):
        sustained.restore(snap)
    with pytest.raises(RuntimeError, match="pending"):
        op.pending.append(_rec(Tuple2("a", 1.0)))
        op.snapshot()


def test_several_ranks_fall_back_in_open():
    from mxstream.runtime.native_ops import NativeBurstOp

    class Comm:
        world = 2

    ctx = _ctx()
    ctx.comm = Comm()
    op = NativeBurstOp(fn=F.BurstAlert(1, ">", 70.0, 3, 120), key_pos=0, device="cpu",
                       fallback_factory=_host)
    op.open(ctx)
    assert op.fallback is not None and op.op is None


# ---- GPU ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_usage_job_equals_the_host_path(gpu_device, route):
    host = _job(_rule(HostAlert))
    got = _job(_rule(), device="cuda")
    assert route == {"built": 1, "fallback": 0}
    assert got == host and len(got) == 3
    assert _job(_rule(times=2, within=10_000), device="cuda") == \
        _job(_rule(HostAlert, 2, 10_000))


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
