"""Broadcast rule set: the C++ twins (csrc/ruleset_cpu.cpp), the engine operator
(runtime/ruleset_operator.py) and NativeRuleSetOp against a dict-based per-record model and
against the host BroadcastProcessOp; the job through env.execute; the gfx950 kernels against the
twins. Every comparison is exact (doubles are compared, never computed with); outputs compare as
lists, in order."""
from __future__ import annotations

import operator
import subprocess

import numpy as np
import pytest
import torch

from mxstream.api import functions as F
from mxstream.api.tuples import Tuple2, Tuple3
from mxstream.ops import kernels as K
from mxstream.runtime.ruleset_operator import RuleSetOperator

WHENS = [">", ">=", "<", "<=", "==", "!="]
CMP = {">": operator.gt, ">=": operator.ge, "<": operator.lt, "<=": operator.le,
       "==": operator.eq, "!=": operator.ne}
SIZES = [0, 1, 63, 64, 65, 4095, 4096, 4097, 2 * 4096 + 1]
NAN = float("nan")
POOL = [0.0, -0.0, 0.5, 1.0, 1.5, 2.0, -3.0, NAN, 1e300, -1e300]   # the lookup test's pool


def bits(x) -> np.ndarray:
    return np.atleast_1d(np.asarray(x, dtype=np.float64)).view(np.int64).copy()


def bit(x: float) -> int:
    return int(bits(x)[0])


def f64(b: int) -> float:
    return float(np.array([b], dtype=np.int64).view(np.float64)[0])


def T(a, dev="cpu") -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev)


class Model:
    """The per-record definition: a dict id -> (when, threshold bits). Values are bit patterns,
    so NaNs and signed zeros compare as what they are."""

    def __init__(self, rules=None):
        self.rules = dict(rules or {})

    def update(self, rid, when, tbits):
        if when is None:
            self.rules.pop(rid, None)
        else:
            self.rules[rid] = (when, tbits)

    def rows(self, keys, vals, ts) -> list:
        out = []
        for k, v, t in zip(np.asarray(keys).tolist(), np.asarray(vals).tolist(),
                           np.asarray(ts).tolist()):
            for rid in sorted(self.rules):
                when, tb = self.rules[rid]
                if CMP[when](f64(v), f64(tb)):
                    out.append((k, v, rid, tb, t))
        return out

    def table(self, dev="cpu") -> torch.Tensor:
        tab = np.zeros((K.RULESET_MAX, 2), dtype=np.int64)
        for rid, (when, tb) in self.rules.items():
            tab[rid] = (tb, K.LOOKUP_WHENS[when])
        return torch.from_numpy(tab).to(dev)


def rows_of(cols) -> list:
    return list(zip(*(c.cpu().numpy().tolist() for c in cols)))


def _probe(table, keys, vals, ts):
    dev = table.device
    rc = K.ruleset_count(table, T(vals, dev))
    return rc, K.ruleset_emit(rc, T(keys, dev), T(ts, dev))


def _check(model: Model, keys, vals, ts) -> int:
    """The twin against the model: the rows, the group sums, the tile counts and the total."""
    rc, out = _probe(model.table(), keys, vals, ts)
    want = model.rows(keys, vals, ts)
    assert rows_of(out) == want
    assert int(rc.counts.sum()) == rc.total == len(want)
    per_sample = np.zeros(len(vals), dtype=np.int64)
    for v in set(np.asarray(vals).tolist()):
        per_sample[np.asarray(vals) == v] = len(model.rows([0], [v], [0]))
    pad = np.zeros(-(-len(vals) // 64) * 64 if len(vals) else 0, dtype=np.int64)
    pad[:len(vals)] = per_sample
    g = rc.gsum.numpy()[:pad.size // 64]
    assert g.tolist() == pad.reshape(-1, 64).sum(1).tolist() and not rc.gsum.numpy()[g.size:].any()
    assert rc.counts.numpy().tolist() == rc.gsum.numpy().reshape(-1, 64).sum(1).tolist()
    assert rc.offsets.numpy().tolist() == (np.cumsum(rc.counts.numpy()) - rc.counts.numpy()).tolist()
    return rc.total


RULE_SETS = {
    "empty": {},
    "one": {7: (">", bit(1.0))},
    "ids_0_5_63": {0: (">", bit(1.0)), 5: ("<=", bit(0.0)), 63: ("!=", bit(NAN))},
    "all_64": {r: (WHENS[r % 6], bit(POOL[r % len(POOL)])) for r in range(64)},
    **{f"every_threshold_{w}": {r: (w, bit(t)) for r, t in enumerate(POOL)} for w in WHENS},
}


# ---- twins against the model -------------------------------------------------------------------
@pytest.mark.parametrize("name", list(RULE_SETS))
def test_twin_equals_the_dict_model(name):
    rng = np.random.default_rng(3)
    pool = bits(POOL)
    model = Model(RULE_SETS[name])
    for n in (0, 1, 10, 300, 5000):
        vals = pool[rng.integers(0, pool.size, n)]
        total = _check(model, rng.integers(0, 50, n), vals, np.arange(n) + 1000)
        if name == "empty" or n == 0:
            assert total == 0
        elif n >= 300:          # (a single sample may break nothing)
            assert total > n // 10


def test_nan_and_signed_zero_follow_java():
    zero = Model({1: ("==", bit(0.0))})
    assert _check(zero, [1, 2, 3], bits([-0.0, 0.0, NAN]), [1, 2, 3]) == 2
    assert _check(Model({1: ("!=", bit(NAN))}), [1, 2], bits([1.0, NAN]), [1, 2]) == 2
    for w in WHENS[:5]:
        assert _check(Model({1: (w, bit(NAN))}), [1, 2], bits([1.0, NAN]), [1, 2]) == 0
        assert _check(Model({1: (w, bit(1.0))}), [1], bits([NAN]), [1]) == 0


def test_withdrawn_and_set_again_and_the_last_rule_of_an_id_wins():
    op = RuleSetOperator("cpu")
    model = Model()
    vals = bits([0.0, 1.0, 2.0, 5.0])
    keys, ts = np.arange(4), np.arange(4) + 10
    steps = [[(3, ">", 1.0), (3, "<", 1.0)],            # the last rule of id 3 wins
             [(3, None, 0.0)],                          # withdrawn: nothing is emitted
             [(3, ">=", 2.0), (9, "==", 5.0)],          # set again
             [(9, None, 7.0), (9, "!=", 0.0), (0, "<", 9.0), (0, None, 0.0)]]
    seen = []
    for rules in steps:
        op.update([r[0] for r in rules], [K.LOOKUP_WHENS[r[1]] for r in rules],
                  bits([r[2] for r in rules]))
        for rid, when, thr in rules:
            model.update(rid, when, bit(thr))
        assert torch.equal(op.table, model.table()) and op.rules().keys() == model.rules.keys()
        got = [r for cols in op.probe(T(keys), T(vals), T(ts)) for r in rows_of(cols)]
        assert got == model.rows(keys, vals, ts)
        _check(model, keys, vals, ts)
        seen.append(len(got))
    assert seen == [1, 0, 3, 5]


@pytest.mark.parametrize("pattern", ["nothing", "everything", "alternating"])
@pytest.mark.parametrize("n", SIZES)
def test_sizes_at_the_group_and_tile_edges(n, pattern):
    hi, lo = np.full(n, 99.0), np.full(n, -1.0)
    vals = {"nothing": lo, "everything": hi,
            "alternating": np.where(np.arange(n) % 2 == 1, 99.0, -1.0)}[pattern]
    broken = {"nothing": 0, "everything": n, "alternating": n // 2}[pattern]
    sets = [Model({0: (">", bit(50.0)), 5: (">=", bit(50.0)), 63: (">", bit(0.0))})]
    if n in (0, 65, 4097):
        sets.append(Model({r: (">", bit(float(r))) for r in range(64)}))   # 64 rows a sample
    for model in sets:
        total = _check(model, np.arange(n) % 7, bits(vals), np.arange(n))
        assert total == broken * len(model.rules)
    if n == 4097 and pattern == "everything":
        assert total == 262_208


def test_wrappers_refuse_bad_operands():
    table = Model(RULE_SETS["one"]).table()
    k, v = T([1, 2]), T(bits([1.0, 2.0]))
    rc = K.ruleset_count(table, v)
    for bad in (torch.zeros((32, 2), dtype=torch.int64), torch.zeros((64, 3), dtype=torch.int64),
                torch.zeros(128, dtype=torch.int64), torch.zeros((128, 2), dtype=torch.int64)[::2]):
        with pytest.raises(ValueError, match=r"\[64, 2\]"):
            K.ruleset_count(bad, v)
    with pytest.raises(TypeError):
        K.ruleset_count(table.to(torch.int32), v)
    with pytest.raises(TypeError):
        K.ruleset_count(table, v.double())
    with pytest.raises(ValueError):
        K.ruleset_emit(rc, k[:1], k)                   # length
    with pytest.raises(TypeError):
        K.ruleset_emit(rc, k.to(torch.int32), k)       # dtype
    with pytest.raises(ValueError):
        K.ruleset_emit(rc, k.to("meta"), k)            # device
    with pytest.raises(ValueError):
        K.ruleset_emit(K.RuleSetCount(table, v, rc.gsum, rc.counts, rc.offsets, 129), k, k)
    with pytest.raises(ValueError):
        K.ruleset_emit(K.RuleSetCount(table, v, rc.gsum[:63], rc.counts, rc.offsets, 1), k, k)
    op = RuleSetOperator("cpu")
    with pytest.raises(TypeError, match="outside"):
        op.update([64], [1], [0])
    with pytest.raises(TypeError, match="outside"):
        op.update([-1], [1], [0])
    with pytest.raises(ValueError):
        op.update([1], [7], [0])
    with pytest.raises(TypeError):
        op.probe(k, v.double(), k)
    with pytest.raises(ValueError):
        RuleSetOperator("cpu", row_chunk=0)


# ---- engine operator against the model ---------------------------------------------------------
def _runs(seed: int, steps: int, max_rows: int = 3000):
    """Random interleaving of rule runs (side 1: ids, whens, threshold bits) and sample runs."""
    rng = np.random.default_rng(seed)
    pool = bits(POOL)
    t0 = 0
    for _ in range(steps):
        if rng.integers(0, 3) == 0:
            n = int(rng.integers(0, 12))
            ids = rng.integers(0, 64, n)
            whens = [None if rng.integers(0, 4) == 0 else WHENS[int(rng.integers(0, 6))]
                     for _ in range(n)]
            yield 1, ids, whens, pool[rng.integers(0, pool.size, n)]
            continue
        n = int(rng.integers(0, max_rows))
        ts = t0 + np.arange(n, dtype=np.int64)
        t0 += n
        yield 0, rng.integers(0, 1000, n).astype(np.int64), ts, pool[rng.integers(0, pool.size, n)]


def _engine_vs_model(dev="cpu", steps=30, seed=5, snapshot_at=None, row_chunk=1 << 24):
    op, model, total, slices = RuleSetOperator(dev, row_chunk), Model(), 0, 0
    for step, (side, a, b, c) in enumerate(_runs(seed, steps)):
        if step == snapshot_at:
            snap = op.snapshot_state()
            assert snap.kg.size == 0 and not snap.columns          # operator state: no key groups
            assert {r: (c_, t) for r, c_, t in snap.meta["rules"]} \
                == {r: (K.LOOKUP_WHENS[w], t) for r, (w, t) in model.rules.items()}
            op = RuleSetOperator(dev, row_chunk)
            op.restore_state(snap.columns, snap.meta)
        if side == 1:
            assert op.process(1, a, [K.LOOKUP_WHENS[w] for w in b], c) == []
            for rid, when, tb in zip(a.tolist(), b, c.tolist()):
                model.update(rid, when, tb)
            continue
        want = model.rows(a, c, b)
        got = op.process(0, T(a, dev), T(b, dev), T(c, dev))
        assert all(0 < cols[0].numel() <= max(row_chunk, len(model.rules)) for cols in got)
        assert [r for cols in got for r in rows_of(cols)] == want
        total += len(want)
        slices += len(got)
    assert total > 1000 and op.metrics.num_records_out == total
    return op, slices


def test_engine_equals_model_and_continues_after_restore():
    _engine_vs_model()
    _engine_vs_model(snapshot_at=14)


def test_row_chunk_forces_slices_and_gives_the_same_rows():
    _, one = _engine_vs_model()
    _, many = _engine_vs_model(row_chunk=1000)
    assert many > one


def test_no_rules_launch_nothing_and_a_foreign_checkpoint_is_refused(monkeypatch):
    op = RuleSetOperator("cpu")
    monkeypatch.setattr(K, "ruleset_count", lambda *a: pytest.fail("launched without a rule"))
    assert op.process(0, T([1]), T([1]), T(bits(1.0))) == [] and op.advance_watermark(5) == []
    monkeypatch.undo()
    from mxstream.runtime.lookup_operator import KeyedLookupOperator

    foreign = KeyedLookupOperator(">", None).snapshot_state()
    with pytest.raises(ValueError, match="not a rule set"):
        op.restore_state(foreign.columns, foreign.meta)
    with pytest.raises(ValueError, match="different lookup"):
        KeyedLookupOperator(">", None).restore_state({}, op.snapshot_state().meta)


# ---- NativeRuleSetOp against the host operator ---------------------------------------------------
def _ctx():
    from mxstream.runtime.operators import OpContext

    return OpContext("ruleset", 4, 128, lambda: 0, "EventTime")


def _host(fn=None):
    from mxstream.runtime.operators import BroadcastProcessOp

    op = BroadcastProcessOp(lambda v: v[0], fn or F.RuleSetAlert(1), (F.RuleSetAlert.DESCRIPTOR,))
    op.open(_ctx())
    return op


def _native(fn=None, **kw):
    from mxstream.runtime.native_ops import NativeRuleSetOp

    fn = fn or F.RuleSetAlert(1)
    op = NativeRuleSetOp(fn=fn, key_pos=0, device=kw.pop("device", "cpu"),
                         fallback_factory=lambda: _host(type(fn)(*fn.native[1:])), **kw)
    op.open(_ctx())
    return op


def _flat(items) -> list:
    """Records as (text, ts, subtask) and watermarks, column batches expanded."""
    from mxstream.runtime.columnar import expand_columns
    from mxstream.runtime.operators import WM

    return [it if isinstance(it, WM) else (str(it.value), it.ts, it.subtask)
            for it in expand_columns(list(items))]


def _tagged_passes(seed, str_keys, float_vals, passes=12):
    """Passes of tagged rule records and sample records / column batches with watermarks."""
    from mxstream.ops.native import load
    from mxstream.ops.text import FK_DOUBLE, FK_LONG, FK_STR
    from mxstream.runtime.columnar import ColumnBatch
    from mxstream.runtime.operators import WM, Rec

    rng = np.random.default_rng(seed)
    sd = load().StringDict()
    key = (lambda i: f"host{i}") if str_keys else (lambda i: int(i) * 3)
    val = (lambda x: float(x) / 2) if float_vals else (lambda x: int(x) - 8)
    ts = 0
    for _ in range(passes):
        items = []
        for _ in range(int(rng.integers(1, 6))):
            if rng.integers(0, 3) == 0:
                for _ in range(int(rng.integers(1, 5))):
                    when = None if rng.integers(0, 5) == 0 else WHENS[int(rng.integers(0, 6))]
                    items.append(Rec((1, Tuple3(int(rng.integers(0, 64)), when,
                                                val(rng.integers(0, 16)))), ts, 0))
                    ts += 1
                continue
            n = int(rng.integers(1, 40))
            ks, vs = rng.integers(0, 25, n), rng.integers(0, 16, n)
            tsa = ts + np.arange(n, dtype=np.int64)
            ts += n
            if rng.integers(0, 2):
                kcol = (np.array([sd.intern(key(k)) for k in ks]) if str_keys
                        else np.array([key(k) for k in ks], dtype=np.int64))
                vcol = np.array([val(v) for v in vs], dtype=np.float64 if float_vals else np.int64)
                items.append(ColumnBatch(n, [kcol, vcol],
                                         (FK_STR if str_keys else FK_LONG,
                                          FK_DOUBLE if float_vals else FK_LONG),
                                         sd if str_keys else None, tsa,
                                         np.zeros(n, np.int32), side=0))
            else:
                items.extend(Rec((0, Tuple2(key(k), val(v))), int(t), 0)
                             for k, v, t in zip(ks, vs, tsa))
            if rng.integers(0, 3) == 0:
                items.append(WM(ts - 1))
        yield items


@pytest.mark.parametrize("float_vals", [True, False], ids=["float", "int"])
@pytest.mark.parametrize("str_keys", [True, False], ids=["str_keys", "int_keys"])
def test_native_operator_equals_the_host_operator(str_keys, float_vals):
    from mxstream.runtime.columnar import ColumnBatch, expand_columns
    from mxstream.runtime.operators import WM

    native, host = _native(), _host()
    rows = 0
    for items in _tagged_passes(11, str_keys, float_vals):
        got, want = native.process(list(items)), host.process(expand_columns(list(items)))
        assert all(isinstance(it, (ColumnBatch, WM)) for it in got)
        assert _flat(got) == _flat(want)          # lists: the same order, ts and subtasks
        rows += len(want)
    assert native.fallback is None and native.op is not None and rows > 50
    assert _flat(native.finish()) == _flat(host.finish()) == []


def test_native_operator_snapshot_restore_and_foreign_function():
    passes = list(_tagged_passes(23, True, True, passes=10))
    ref, op = _native(), _native()
    want = [_flat(ref.process(list(p))) for p in passes]
    for i, p in enumerate(passes):
        if i == 5:
            snap = op.snapshot()
            assert snap["ruleset"] == (1, 0, 1, 2) and snap["engine"]["meta"]["kind"] == "ruleset"
            op = _native()
            op.restore(snap)
        assert _flat(op.process(list(p))) == want[i]
    for other in (F.RuleSetAlert(0), F.RuleSetAlert(1, 0, 1, 3), F.RuleSetAlert(1, 1, 0, 2)):
        with pytest.raises(ValueError, match="different rule-set"):
            _native(other).restore(snap)


def test_integers_at_2_53_come_back_as_longs_and_beyond_switch_to_the_host():
    from mxstream.runtime.operators import Rec

    big = 1 << 53
    items = [Rec((1, Tuple3(1, "<", big)), 1, 0), Rec((0, Tuple2("a", -big)), 2, 0),
             Rec((1, Tuple3(2, ">=", -big)), 3, 0), Rec((0, Tuple2("b", big)), 4, 0)]
    op = _native()
    got = _flat(op.process(list(items)))
    assert [g[0] for g in got] == [f"(a,-{big},1,{big})", f"(b,{big},2,-{big})"]
    assert op.fallback is None and got == _flat(_host().process(list(items)))
    # 2**53 + 1 is no double: the host operator, before native state exists ...
    for over in ([Rec((1, Tuple3(1, "<=", big + 1)), 1, 0), Rec((0, Tuple2("a", big)), 2, 0)],
                 [Rec((1, Tuple3(1, ">=", big)), 1, 0), Rec((0, Tuple2("a", big + 1)), 2, 0)]):
        op = _native()
        got = _flat(op.process(list(over)))
        assert op.fallback is not None and op.op is None
        assert len(got) == 1 and got == _flat(_host().process(list(over)))  # compared as doubles
    # ... and an error afterwards
    op = _native()
    op.process(list(items))
    with pytest.raises(TypeError):
        op.process(list(over))


def test_rule_id_64_and_mixed_threshold_kinds_fall_back_then_raise():
    from mxstream.runtime.operators import Rec

    ok = [Rec((1, Tuple3(63, ">", 1.0)), 1, 0), Rec((0, Tuple2("a", 2.0)), 2, 0)]
    for bad in ([Rec((1, Tuple3(64, ">", 1.0)), 1, 0), Rec((0, Tuple2("a", 2.0)), 2, 0)],
                [Rec((1, Tuple3(-1, ">", 1.0)), 1, 0), Rec((0, Tuple2("a", 2.0)), 2, 0)],
                [Rec((1, Tuple3(1, ">", 1.0)), 1, 0), Rec((1, Tuple3(2, ">", 1)), 2, 0),
                 Rec((0, Tuple2("a", 2.0)), 3, 0)],
                [Rec((1, Tuple3(1, ">", 1.0)), 1, 0), Rec((0, Tuple2("a", "high")), 3, 0)]):
        op = _native()
        try:
            want = _flat(_host().process(list(bad)))
        except TypeError:           # a non-numeric value is the host function's error too
            with pytest.raises(TypeError, match="int or a float"):
                op.process(list(bad))
            assert op.fallback is not None
            continue
        assert _flat(op.process(list(bad))) == want and len(want) >= 1
        assert op.fallback is not None and op.op is None
        op = _native()
        assert [g[0] for g in _flat(op.process(list(ok)))] == ["(a,2.0,63,1.0)"]
        with pytest.raises(TypeError):
            op.process(list(bad))
    # a withdrawal's threshold is not stored: its kind does not matter
    op = _native()
    got = _flat(op.process(ok + [Rec((1, Tuple3(63, None, 0)), 3, 0),
                                 Rec((0, Tuple2("a", 2.0)), 4, 0)]))
    assert got == [("(a,2.0,63,1.0)", 2, _host().subtask_of("a"))] and op.fallback is None


def test_a_malformed_rule_raises_before_the_state_is_touched():
    from mxstream.runtime.operators import Rec

    for rule, err in ((Tuple3(True, ">", 1.0), TypeError), (Tuple3(1.0, ">", 1.0), TypeError),
                      (Tuple3(1, "=>", 1.0), ValueError), (Tuple3(1, 1, 1.0), ValueError),
                      (Tuple3(1, ">", "x"), TypeError), (Tuple3(1, ">", True), TypeError)):
        host = _host()
        with pytest.raises(err):
            host.process([Rec((1, rule), 1, 0)])
        assert all(c == {"rule-set": {}} for c in host.copies)
    with pytest.raises(ValueError):
        F.RuleSetAlert(-1)
    with pytest.raises(ValueError):
        F.RuleSetAlert(1, threshold_field=True)


# ---- the job ---------------------------------------------------------------------------------------
SAMPLES = [(f"host{i % 5}", "cpu", float((i * 37) % 100), i * 10) for i in range(300)]
RULES = [(1, ">", 80.0, 5), (2, ">", 95.0, 5), (3, "<", 1.0, 5), (1, ">", 90.0, 1005),
         (2, None, 0.0, 1505), (4, "==", 50.0, 2005), (1, None, 0, 2505)]


class HostRuleSet(F.RuleSetAlert):
    """A subclass keeps the host path: the planner lowers exactly RuleSetAlert."""


def _job(fn, native="auto", device="cpu", int_vals=False, selector=False):
    from mxstream.api.environment import StreamExecutionEnvironment
    from mxstream.api.time import Time, TimeCharacteristic
    from mxstream.api.watermarks import BoundedOutOfOrdernessTimestampExtractor
    from mxstream.runtime.executor import ManualClock

    out = []
    env = StreamExecutionEnvironment(4, clock=ManualClock(0)).set_output(out.append)
    env.config.native, env.config.device = native, device
    env.set_stream_time_characteristic(TimeCharacteristic.EventTime)

    def stream(events, ts_field):
        return env.from_timed_collection([(e[ts_field] + 10, e) for e in events]) \
            .assign_timestamps_and_watermarks(BoundedOutOfOrdernessTimestampExtractor(
                Time.milliseconds(0), extractor=lambda e: e[ts_field]))

    conv = int if int_vals else float
    s = stream(SAMPLES, 3).map(lambda e: Tuple3(e[0], e[1], conv(e[2])))
    r = stream(RULES, 3).map(lambda e: Tuple3(e[0], e[1], conv(e[2])))
    s.key_by((lambda v: v[0]) if selector else 0).connect(r.broadcast(F.RuleSetAlert.DESCRIPTOR)) \
        .process(fn).print()
    env.execute("rule set")
    return out


def _expected(int_vals=False):
    conv = int if int_vals else float
    events = sorted([(e[3], 0, e) for e in SAMPLES] + [(e[3], 1, e) for e in RULES])
    state, rows = {}, []
    for _, side, e in events:
        if side == 1:
            if e[1] is None:
                state.pop(e[0], None)
            else:
                state[e[0]] = (e[1], conv(e[2]))
            continue
        rows.extend(f"({e[0]},{conv(e[2])},{rid},{t})" for rid, (w, t) in sorted(state.items())
                    if CMP[w](conv(e[2]), t))
    return rows


@pytest.fixture
def route(monkeypatch):
    from mxstream.runtime.native_ops import NativeRuleSetOp

    seen = {"built": 0, "fallback": 0}
    init, to_fb = RuleSetOperator.__init__, NativeRuleSetOp._to_fallback

    def spy_init(self, *a, **kw):
        seen["built"] += 1
        init(self, *a, **kw)

    def spy_fb(self):
        seen["fallback"] += 1
        to_fb(self)

    monkeypatch.setattr(RuleSetOperator, "__init__", spy_init)
    monkeypatch.setattr(NativeRuleSetOp, "_to_fallback", spy_fb)
    return seen


@pytest.mark.parametrize("int_vals", [False, True], ids=["float", "int"])
def test_job_native_on_cpu_equals_the_host_paths(route, int_vals):
    want = _expected(int_vals)
    host = _job(HostRuleSet(2), int_vals=int_vals)
    assert [ln[ln.index("("):] for ln in host] == want and len(want) > 40
    assert _job(F.RuleSetAlert(2), "off", int_vals=int_vals) == host
    assert _job(F.RuleSetAlert(2), selector=True, int_vals=int_vals) == host   # a key selector
    assert route == {"built": 0, "fallback": 0}
    native = _job(F.RuleSetAlert(2), int_vals=int_vals)
    assert route == {"built": 1, "fallback": 0}
    assert native == host and len({ln[0] for ln in native}) > 1     # lists: the same order


def test_job_quick_start_lines():
    got = _job(F.RuleSetAlert(2))
    # warning at 80, critical at 95, idle below 1: host0's 85.0 at t = 50 is a warning, host3's
    # 96.0 at t = 80 a warning and critical (ascending rule id), host0's 0.0 at t = 1000 idle
    assert got[:4] == ["1> (host0,85.0,1,80.0)", "4> (host3,96.0,1,80.0)",
                       "4> (host3,96.0,2,95.0)", "4> (host3,81.0,1,80.0)"]
    assert "1> (host0,0.0,3,1.0)" in got and "1> (host0,50.0,4,50.0)" in got
    # rule 1 moves to 90 at t = 1005 and is withdrawn at t = 2505
    last_80 = max(i for i, ln in enumerate(got) if ln.endswith(",1,80.0)"))
    assert last_80 < min(i for i, ln in enumerate(got) if ln.endswith(",1,90.0)"))


# ---- sanitizer, benchmark --------------------------------------------------------------------------
def test_sanitizer_harness_runs_clean():
    from mxstream.build import build_sanitize_ruleset

    res = subprocess.run([str(build_sanitize_ruleset())], capture_output=True, text=True,
                         timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.strip().splitlines()[-1] == "ruleset sanitize ok"


def test_bench_config_20_runs_on_the_cpu_at_a_tiny_shape():
    from mxstream.models.bench_configs import config20

    r = config20(steps=2, warmup=1, batch=10_000, keys=100, device="cpu")
    assert r["config"] == 20 and r["rules"] == 8 and 0.03 < r["rows_per_sample"] < 0.08
    assert r["native_over_torch_time"] > 0 and r["native_ms"]["median"] > 0
    d = config20(steps=2, warmup=1, batch=3_000, keys=100, rules=5, dense=True, device="cpu")
    assert d["rows_per_step"] == 15_000 and d["rows_per_sample"] == 5.0 and d["dense"]


# ---- GPU -------------------------------------------------------------------------------------------
def _both(dev, model: Model, keys, vals, ts) -> int:
    """The probe on the twin and on the device from the same table: every array equal."""
    res = []
    for d in ("cpu", dev):
        rc, out = _probe(model.table(d), keys, vals, ts)
        res.append((rc.gsum.cpu(), rc.counts.cpu(), rc.offsets.cpu(), rc.total,
                    [c.cpu() for c in out]))
    (g0, c0, o0, t0, out0), (g1, c1, o1, t1, out1) = res
    assert torch.equal(g0, g1) and torch.equal(c0, c1) and torch.equal(o0, o1) and t0 == t1
    assert all(torch.equal(a, b) for a, b in zip(out0, out1))
    return t0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["empty", "one", "ids_0_5_63", "all_64", "every_threshold_>=",
                                  "every_threshold_!="])
def test_gpu_kernels_equal_the_twin(gpu_device, name):
    rng = np.random.default_rng(2)
    pool = bits(POOL + [50.0, 99.0])
    model = Model(RULE_SETS[name])
    for n in SIZES:
        vals = pool[rng.integers(0, pool.size, n)]
        if n > 3:
            vals[::7] = bit(NAN)
        _both(gpu_device, model, rng.integers(0, 1200, n), vals, np.arange(n))


@pytest.mark.gpu
def test_gpu_every_comparison_and_all_64_rules_broken(gpu_device):
    six = Model({10 * i + 3: (w, bit(1.0)) for i, w in enumerate(WHENS)})
    vals = bits(np.resize(np.array(POOL), 4097))
    _both(gpu_device, six, np.arange(4097), vals, np.arange(4097))
    every = Model({r: (">", bit(float(r))) for r in range(64)})
    for pattern in (np.full(4097, 99.0), np.full(4097, -1.0),
                    np.where(np.arange(4097) % 2 == 1, 99.0, -1.0)):
        total = _both(gpu_device, every, np.arange(4097) % 64, bits(pattern), np.arange(4097))
        assert total == 64 * int((pattern > 63).sum())
    assert total == 64 * 2048 and _both(gpu_device, every, np.arange(4097), bits(np.full(4097, 99.0)),
                                        np.arange(4097)) == 262_208


@pytest.mark.gpu
def test_gpu_more_tiles_than_one_scan_round(gpu_device):
    """1025 tiles with one row each: the scan's carry round."""
    ntiles = 1025
    n = ntiles * K.LOOKUP_TILE
    vals = np.full(n, 1.0)
    hot = np.arange(ntiles) * K.LOOKUP_TILE + (np.arange(ntiles) * 37) % K.LOOKUP_TILE
    vals[hot] = 99.0
    model = Model({9: (">", bit(50.0)), 20: ("<", bit(0.0))})
    assert _both(gpu_device, model, np.arange(n) % 1000, bits(vals), np.arange(n)) == ntiles


@pytest.mark.gpu
def test_gpu_engine_equals_model_with_a_snapshot_in_the_middle(gpu_device):
    _engine_vs_model(dev=gpu_device, snapshot_at=14)
    _engine_vs_model(dev=gpu_device, row_chunk=1000, seed=6)


@pytest.mark.gpu
def test_gpu_job_equals_the_host_path(gpu_device, route):
    host = _job(HostRuleSet(2))
    got = _job(F.RuleSetAlert(2), device="cuda")
    assert route == {"built": 1, "fallback": 0}
    assert got == host and len(got) > 40
