"""Keyed latest-value lookup: the C++ twins (csrc/lookup_cpu.cpp), the engine operator
(runtime/lookup_operator.py) and NativeLookupOp against a dict-based per-record model and against
the host CoProcessOp; the gfx950 kernels against the twins. Outputs compare as lists, in order."""
from __future__ import annotations

import functools
import operator
import subprocess

import numpy as np
import pytest
import torch

from mxstream.api import functions as F
from mxstream.api.tuples import Tuple2
from mxstream.ops import kernels as K
from mxstream.runtime.lookup_operator import KeyedLookupOperator

WHENS = [None, ">", ">=", "<", "<=", "==", "!="]
CMP = {None: lambda a, b: True, ">": operator.gt, ">=": operator.ge, "<": operator.lt,
       "<=": operator.le, "==": operator.eq, "!=": operator.ne}
SIZES = [1, 63, 64, 65, 4095, 4096, 4097, 2 * 4096 + 1]
NAN = float("nan")


def bits(x) -> np.ndarray:
    return np.atleast_1d(np.asarray(x, dtype=np.float64)).view(np.int64).copy()


def bit(x: float) -> int:
    return int(bits(x)[0])


def f64(b: int) -> float:
    return float(np.array([b], dtype=np.int64).view(np.float64)[0])


def T(a, dev="cpu") -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev)


class Model:
    """The per-record definition: a dict of the latest rule per key. Values are bit patterns, so
    NaNs and signed zeros compare as what they are."""

    def __init__(self, when, default_bits=None):
        self.when, self.default_bits, self.state = when, default_bits, {}

    def run(self, side, keys, vals, ts) -> list:
        out = []
        for k, v, t in zip(keys.tolist(), vals.tolist(), ts.tolist()):
            if side == 1:
                self.state[k] = v
                continue
            tb = self.state.get(k, self.default_bits)
            if tb is not None and CMP[self.when](f64(v), f64(tb)):
                out.append((k, v, tb, t))
        return out


def rows_of(cols) -> list:
    return list(zip(*(c.cpu().numpy().tolist() for c in cols)))


def _runs(seed: int, steps: int, nkeys: int, max_rows: int = 300, rule_keys: int | None = None):
    """Random interleaving of rule (side 1) and sample (side 0) runs; values from a small set so
    that every comparison meets equal pairs, with NaN and both zeros among them."""
    rng = np.random.default_rng(seed)
    pool = bits([0.0, -0.0, 0.5, 1.0, 1.5, 2.0, -3.0, NAN, 1e300, -1e300])
    t0 = 0
    for _ in range(steps):
        side = int(rng.integers(0, 2))
        n = int(rng.integers(0, max_rows if side == 0 else max_rows // 4))
        hi = nkeys if side == 0 or rule_keys is None else rule_keys
        keys = rng.integers(0, hi, n).astype(np.int64)
        vals = pool[rng.integers(0, pool.size, n)]
        ts = t0 + np.arange(n, dtype=np.int64)
        t0 += n
        yield side, keys, vals, ts


def _table(cap: int, dev="cpu") -> torch.Tensor:
    return torch.zeros((cap, 2), dtype=torch.int64, device=dev)


def _probe(table, keys, vals, ts, when, dbits):
    dev = table.device
    keys, vals, ts = T(keys, dev), T(vals, dev), T(ts, dev)
    lm = K.lookup_mask(table, keys, vals, when, dbits)
    out = K.lookup_emit(lm, ts)
    if when is None and dbits is not None:  # the gather-only path gives the same rows
        g = K.lookup_gather(table, keys, vals, ts, dbits)
        assert rows_of(g) == rows_of(out)
    return lm, out


# ---- twins against the model -------------------------------------------------------------------
@pytest.mark.parametrize("default", [None, 1.0, NAN], ids=["nodefault", "default", "nandefault"])
@pytest.mark.parametrize("when", WHENS, ids=[str(w) for w in WHENS])
def test_twin_equals_the_dict_model(when, default):
    dbits = None if default is None else bit(default)
    table, model = _table(64), Model(when, dbits)
    # sample keys reach beyond the table (64 .. 95 never have a rule)
    for side, keys, vals, ts in _runs(seed=3, steps=40, nkeys=96, rule_keys=64):
        want = model.run(side, keys, vals, ts)
        if side == 1:
            K.lookup_upsert(table, T(keys), T(vals))
            continue
        lm, out = _probe(table, keys, vals, ts, when, dbits)
        assert rows_of(out) == want
        assert lm.kept == len(want) == int(lm.counts.sum())
    present = np.nonzero(table.numpy()[:, 1])[0].tolist()
    assert present == sorted(model.state) and len(present) > 32
    assert table.numpy()[present, 0].tolist() == [model.state[k] for k in present]


def test_last_rule_wins():
    table = _table(8)
    K.lookup_upsert(table, T(np.full(1000, 5)), T(bits(np.arange(1000.0))))
    assert table[5].tolist() == [bit(999.0), 1] and int(table[:, 1].sum()) == 1
    keys = np.concatenate([np.arange(8), np.arange(8)[::-1]])     # every key twice
    K.lookup_upsert(table, T(keys), T(bits(np.arange(16.0))))
    assert table[:, 0].tolist() == [bit(15.0 - k) for k in range(8)]
    K.lookup_upsert(table, T(np.array([3])), T(bits(-1.0)))       # one row: no sort
    assert table[3].tolist() == [bit(-1.0), 1]
    with pytest.raises(ValueError):
        K.lookup_upsert(table, T(np.array([8])), T(bits(1.0)))    # outside the table
    with pytest.raises(ValueError):
        K.lookup_upsert(table, T(np.array([-1])), T(bits(1.0)))


def test_keys_without_a_rule_and_beyond_the_table():
    table = _table(1)  # cap = 1
    K.lookup_upsert(table, T([0]), T(bits(50.0)))
    keys = np.array([0, 1, 2, 1 << 40, -1, K.I64_MAX, K.I64_MIN, 0])
    vals = bits(np.full(keys.size, 60.0))
    ts = np.arange(keys.size)
    _, out = _probe(table, keys, vals, ts, ">", None)
    assert rows_of(out) == [(0, bit(60.0), bit(50.0), 0), (0, bit(60.0), bit(50.0), 7)]
    _, out = _probe(table, keys, vals, ts, ">", bit(55.0))     # the others take the default
    assert [r[2] for r in rows_of(out)] == [bit(50.0)] + [bit(55.0)] * 6 + [bit(50.0)]
    _, out = _probe(table, keys, vals, ts, None, bit(55.0))
    assert len(rows_of(out)) == keys.size
    _, out = _probe(_table(4), keys, vals, ts, None, None)     # an empty table keeps nothing
    assert rows_of(out) == []


def test_growth_across_three_doublings_keeps_the_old_rows():
    op = KeyedLookupOperator(">", None, "cpu", capacity=4)
    model = {}
    for k in (3, 7, 15, 31):  # 4 -> 8 -> 16 -> 32
        op.upsert(T([k, 0]), T(bits([float(k), float(-k)])))
        model[k], model[0] = bit(float(k)), bit(float(-k))
        assert op.cap == k + 1
        ids, vals = op.entries()
        assert dict(zip(ids.tolist(), vals.tolist())) == model
    out = op.probe(T([3, 7, 15, 31, 32, 0]), T(bits([9.0] * 6)), T(np.arange(6)))
    assert [r[0] for r in rows_of(out)] == [3, 7, 0]


@pytest.mark.parametrize("when", WHENS[1:], ids=WHENS[1:])
def test_nan_and_signed_zero_follow_java(when):
    """A NaN sample, a NaN rule and a NaN default are false for every operator but !=;
    -0.0 == 0.0."""
    table = _table(4)
    K.lookup_upsert(table, T([0, 1, 2]), T(bits([NAN, 0.0, -0.0])))
    keys = np.array([0, 0, 1, 1, 2, 2, 3, 3, 1])
    vals = bits([1.0, NAN, -0.0, NAN, 0.0, 1.0, 1.0, NAN, 0.0])
    for dbits in (None, bit(NAN)):
        _, out = _probe(table, keys, vals, np.arange(9), when, dbits)
        got = [r[3] for r in rows_of(out)]
        # rows 0, 1, 3 (and 6, 7 with the NaN default) have a NaN on one side
        nan_rows = [0, 1, 3] + ([6, 7] if dbits is not None else [])
        zero_rows = [2, 4, 8]                      # +-0.0 against +-0.0: equal
        want = set()
        if when == "!=":
            want |= set(nan_rows)
        if when in ("==", ">=", "<="):
            want |= set(zero_rows)
        if when in (">", ">=", "!="):
            want.add(5)                            # 1.0 against -0.0
        assert got == sorted(want)


@pytest.mark.parametrize("pattern", ["all", "none", "alternating"])
@pytest.mark.parametrize("n", [0] + SIZES)
def test_sizes_at_the_word_and_tile_edges(n, pattern):
    table = _table(128)
    K.lookup_upsert(table, T(np.arange(64)), T(bits(np.full(64, 50.0))))
    keys = np.arange(n) % 64
    v = {"all": np.full(n, 99.0), "none": np.full(n, 1.0),
         "alternating": np.where(np.arange(n) % 2 == 1, 99.0, 1.0)}[pattern]
    ts = np.arange(n) + 7
    lm, out = _probe(table, keys, bits(v), ts, ">", None)
    keep = np.nonzero(v > 50.0)[0]
    assert lm.kept == keep.size == {"all": n, "none": 0, "alternating": n // 2}[pattern]
    assert rows_of(out) == [(int(keys[i]), bit(v[i]), bit(50.0), int(ts[i])) for i in keep]
    ntiles = -(-n // K.LOOKUP_TILE)
    assert lm.counts.numel() == ntiles and lm.words.numel() == 64 * ntiles
    assert lm.offsets.tolist() == np.concatenate(
        [[0], np.cumsum(lm.counts.numpy())[:-1]]).astype(int).tolist()[:ntiles]
    w = lm.words.numpy().view(np.uint64)
    assert sum(bin(int(x)).count("1") for x in w) == keep.size


def test_empty_batches_on_either_side():
    op = KeyedLookupOperator("<", bit(1.0), "cpu")
    e = T([])
    op.upsert(e, e)
    assert [c.numel() for c in op.probe(e, e, e)] == [0] * 4 and op.process(0, e, e, e) == []
    op.upsert(T([2]), T(bits(5.0)))
    assert op.process(1, e, e, e) == [] and op.entries()[0].tolist() == [2]


def test_wrappers_refuse_bad_operands():
    table = _table(4)
    k, v = T([1, 2]), T(bits([1.0, 2.0]))
    with pytest.raises(ValueError, match="when must be one of"):
        K.lookup_mask(table, k, v, "=>")
    with pytest.raises(ValueError):
        K.lookup_mask(torch.zeros((4, 3), dtype=torch.int64), k, v, ">")
    with pytest.raises(ValueError):
        K.lookup_mask(table[:, :1], k, v, ">")
    with pytest.raises(TypeError):
        K.lookup_mask(table, k.to(torch.int32), v, ">")
    with pytest.raises(ValueError):
        K.lookup_mask(table, k, v[:1], ">")
    with pytest.raises(ValueError):
        KeyedLookupOperator("~", None, "cpu")
    with pytest.raises(TypeError):
        KeyedLookupOperator(">", None, "cpu").upsert(k, v.double())


# ---- engine operator against the model ---------------------------------------------------------
def _engine_vs_model(when, default, dev="cpu", steps=20, seed=5, snapshot_at=None):
    dbits = None if default is None else bit(default)
    op = KeyedLookupOperator(when, dbits, dev, capacity=4)
    model = Model(when, dbits)
    caps, total = {op.cap}, 0
    for step, (side, keys, vals, ts) in enumerate(
            _runs(seed, steps, nkeys=3000, max_rows=6000, rule_keys=2000)):
        if step == snapshot_at:
            snap = op.snapshot_state()
            assert sorted(snap.columns["key"].tolist()) == sorted(model.state)
            assert snap.kg.size == len(model.state)
            op = KeyedLookupOperator(when, dbits, dev, capacity=4)
            op.restore_state(snap.columns, snap.meta)
        want = model.run(side, keys, vals, ts)
        got = op.process(side, T(keys, dev), T(ts, dev), T(vals, dev))
        assert [r for cols in got for r in rows_of(cols)] == want
        caps.add(op.cap)
        total += len(want)
    assert len(caps) >= 2 and total > 0  # the table grew on the way
    return op


@pytest.mark.parametrize("default", [None, 1.0], ids=["nodefault", "default"])
@pytest.mark.parametrize("when", WHENS, ids=[str(w) for w in WHENS])
def test_engine_equals_model_and_continues_after_restore(when, default):
    _engine_vs_model(when, default)
    _engine_vs_model(when, default, snapshot_at=11)


def test_foreign_checkpoint_is_refused():
    op = _engine_vs_model(">", None, steps=6)
    snap = op.snapshot_state()
    for other in (KeyedLookupOperator(">=", None), KeyedLookupOperator(">", bit(1.0))):
        with pytest.raises(ValueError, match="different lookup"):
            other.restore_state(snap.columns, snap.meta)
    with pytest.raises(ValueError, match="different lookup"):
        KeyedLookupOperator(">", None).restore_state(snap.columns, {"kind": "interval_join"})


def test_dense_limit_refuses_a_rule_key():
    op = KeyedLookupOperator(">", None, "cpu", dense_limit=100)
    op.upsert(T([99]), T(bits(1.0)))
    with pytest.raises(TypeError, match="not dense"):
        op.upsert(T([100]), T(bits(1.0)))
    assert op.cap <= 100
    out = op.probe(T([99, 100, 1 << 50]), T(bits([2.0] * 3)), T([1, 2, 3]))   # samples may
    assert [r[0] for r in rows_of(out)] == [99]


# ---- NativeLookupOp against the host operator ----------------------------------------------------
def _ctx():
    from mxstream.runtime.operators import OpContext

    return OpContext("lookup", 4, 128, lambda: 0, "EventTime")


def _native(fn, host=None, **kw):
    from mxstream.runtime.native_ops import NativeLookupOp

    kp, vp = (0, 0), (fn.value_field, fn.state_field)
    op = NativeLookupOp(fn=fn, key_pos=kp, val_pos=vp,
                        ok_arities=tuple(range(max(kp[s], vp[s]) + 1, 64) for s in (0, 1)),
                        device=kw.pop("device", "cpu"),
                        fallback_factory=host or (lambda: _host(type(fn)(*fn.native[1:]))), **kw)
    op.open(_ctx())
    return op


def _host(fn):
    from mxstream.runtime.operators import CoProcessOp

    op = CoProcessOp(lambda tv: tv[1][0], fn)
    op.open(_ctx())
    return op


def _flat(items) -> list:
    """Records as (text, ts, subtask) and watermarks, column batches expanded."""
    from mxstream.runtime.columnar import expand_columns
    from mxstream.runtime.operators import WM

    return [it if isinstance(it, WM) else (str(it.value), it.ts, it.subtask)
            for it in expand_columns(items)]


def _tagged_passes(seed, str_keys, float_vals, passes=12, batches=True):
    """Passes of tagged records and column batches of both sides with watermarks in between."""
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
            side = int(rng.integers(0, 2))
            n = int(rng.integers(1, 40))
            ks, vs = rng.integers(0, 25, n), rng.integers(0, 16, n)
            tsa = ts + np.arange(n, dtype=np.int64)
            ts += n
            if batches and rng.integers(0, 2):
                kcol = (np.array([sd.intern(key(k)) for k in ks]) if str_keys
                        else np.array([key(k) for k in ks], dtype=np.int64))
                vcol = np.array([val(v) for v in vs], dtype=np.float64 if float_vals else np.int64)
                items.append(ColumnBatch(n, [kcol, vcol],
                                         (FK_STR if str_keys else FK_LONG,
                                          FK_DOUBLE if float_vals else FK_LONG),
                                         sd if str_keys else None, tsa,
                                         np.zeros(n, np.int32), side=side))
            else:
                items.extend(Rec((side, Tuple2(key(k), val(v))), int(t), 0)
                             for k, v, t in zip(ks, vs, tsa))
            if rng.integers(0, 3) == 0:
                items.append(WM(ts - 1))
        yield items


@pytest.mark.parametrize("when,default", [(">", None), ("<=", None), (None, None), ("!=", 3),
                                          (None, 2), ("==", 2.5)])
@pytest.mark.parametrize("float_vals", [True, False], ids=["float", "int"])
@pytest.mark.parametrize("str_keys", [True, False], ids=["str_keys", "int_keys"])
def test_native_operator_equals_the_host_operator(str_keys, float_vals, when, default):
    from mxstream.runtime.columnar import ColumnBatch
    from mxstream.runtime.operators import WM

    if default is not None and isinstance(default, float) != float_vals:
        default = float(default) if float_vals else int(default)
    fn = F.LookupLatest(1, 1, when=when, default=default)
    native, host = _native(fn), _host(F.LookupLatest(1, 1, when=when, default=default))
    rows = 0
    for items in _tagged_passes(11, str_keys, float_vals):
        got, want = native.process(list(items)), host.process(_expand(items))
        assert all(isinstance(it, (ColumnBatch, WM)) for it in got)
        assert _flat(got) == _flat(want)
        rows += len(want)
    assert native.fallback is None and native.op is not None and rows > 10
    assert _flat(native.finish()) == _flat(host.finish()) == []


def _expand(items):
    from mxstream.runtime.columnar import expand_columns

    return expand_columns(list(items))


def test_native_operator_snapshot_restore_and_foreign_function():
    fn = F.LookupLatest(1, 1, when=">", default=4.0)
    passes = list(_tagged_passes(23, True, True, passes=10))
    ref, op = _native(fn), _native(fn)
    want = [_flat(ref.process(list(p))) for p in passes]
    for i, p in enumerate(passes):
        if i == 5:
            snap = op.snapshot()
            assert snap["lookup"] == (1, 1, ">", 4.0) and snap["engine"]["meta"]["kind"] == "lookup"
            op = _native(fn)
            op.restore(snap)
        assert _flat(op.process(list(p))) == want[i]
    for other in (F.LookupLatest(1, 1, when=">="), F.LookupLatest(1, 1, when=">", default=4),
                  F.LookupLatest(0, 1, when=">", default=4.0)):
        with pytest.raises(ValueError, match="different lookup"):
            _native(other).restore(snap)


def test_integers_at_2_53_come_back_as_longs_and_beyond_switch_to_the_host():
    from mxstream.runtime.operators import Rec

    big = 1 << 53
    fn = F.LookupLatest(1, 1, when="<")
    items = [Rec((1, Tuple2("a", big)), 1, 0), Rec((0, Tuple2("a", -big)), 2, 0),
             Rec((1, Tuple2("b", -big)), 3, 0), Rec((0, Tuple2("b", big)), 4, 0),
             Rec((0, Tuple2("b", -big)), 5, 0)]
    op = _native(fn)
    got = _flat(op.process(list(items)))
    assert [g[0] for g in got] == [f"(a,-{big},{big})"] and op.fallback is None
    assert got == _flat(_host(F.LookupLatest(1, 1, when="<")).process(list(items)))
    # 2**53 + 1 is no double: the host operator, before native state exists ...
    over = [Rec((1, Tuple2("a", big + 1)), 1, 0), Rec((0, Tuple2("a", big)), 2, 0)]
    for when, want in (("<", []), ("<=", [f"(a,{big},{big + 1})"])):  # compared as doubles
        op = _native(F.LookupLatest(1, 1, when=when))
        got = _flat(op.process(list(over)))
        assert op.fallback is not None and op.op is None
        assert [g[0] for g in got] == want
    # ... and an error afterwards
    op = _native(fn)
    op.process(list(items))
    with pytest.raises(TypeError):
        op.process(list(over))


def test_rule_key_beyond_dense_limit_falls_back_then_raises():
    from mxstream.runtime.operators import Rec

    fn = F.LookupLatest(1, 1, when=">")
    far = [Rec((1, Tuple2(100, 1.0)), 1, 0), Rec((0, Tuple2(100, 2.0)), 2, 0)]
    near = [Rec((1, Tuple2(99, 1.0)), 1, 0), Rec((0, Tuple2(99, 2.0)), 2, 0),
            Rec((0, Tuple2(1 << 40, 2.0)), 3, 0)]  # a sample key may lie anywhere
    op = _native(fn, dense_limit=100)
    assert [g[0] for g in _flat(op.process(list(far)))] == ["(100,2.0,1.0)"]
    assert op.fallback is not None and op.op is None
    op = _native(fn, dense_limit=100)
    assert [g[0] for g in _flat(op.process(list(near)))] == ["(99,2.0,1.0)"]
    assert op.fallback is None
    with pytest.raises(TypeError):
        op.process(list(far))


# ---- sanitizer -----------------------------------------------------------------------------
def test_sanitizer_harness_runs_clean():
    from mxstream.build import build_sanitize_lookup

    res = subprocess.run([str(build_sanitize_lookup())], capture_output=True, text=True,
                         timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.strip().splitlines()[-1] == "lookup sanitize ok"


# ---- GPU ---------------------------------------------------------------------------------------
def _both(dev, table_rows, keys, vals, ts, when, dbits, cap):
    """The probe on the twin and on the device from the same table: every array equal."""
    res = []
    for d in ("cpu", dev):
        table = _table(cap, d)
        if len(table_rows[0]):
            K.lookup_upsert(table, T(table_rows[0], d), T(table_rows[1], d))
        lm, out = _probe(table, keys, vals, ts, when, dbits)
        res.append((table.cpu(), lm.words.cpu(), lm.counts.cpu(), lm.offsets.cpu(), lm.kept,
                    [c.cpu() for c in out]))
    (t0, w0, c0, o0, k0, out0), (t1, w1, c1, o1, k1, out1) = res
    assert torch.equal(t0, t1) and torch.equal(w0, w1) and torch.equal(c0, c1)
    assert torch.equal(o0, o1) and k0 == k1
    assert all(torch.equal(a, b) for a, b in zip(out0, out1))
    return k0


@functools.lru_cache(maxsize=None)
def _gpu_rules():
    rng = np.random.default_rng(1)
    keys = rng.integers(0, 1000, 5000).astype(np.int64)     # every key several times
    return keys, bits(rng.integers(0, 100, 5000).astype(np.float64))


@pytest.mark.gpu
@pytest.mark.parametrize("when,default", [(">", None), ("==", 50.0), ("!=", NAN), (None, 7.0),
                                          (None, None), ("<=", None)])
def test_gpu_kernels_equal_the_twin(gpu_device, when, default):
    dbits = None if default is None else bit(default)
    rng = np.random.default_rng(2)
    for n in [0] + SIZES:
        keys = rng.integers(0, 1200, n).astype(np.int64)     # 1000 .. 1199 beyond cap
        vals = bits(rng.integers(0, 100, n).astype(np.float64))
        if n > 3:
            vals[::7] = bit(NAN)
            keys[1], keys[2] = -1, K.I64_MAX
        _both(gpu_device, _gpu_rules(), keys, vals, np.arange(n), when, dbits, cap=1000)
    for pattern in (np.full(4097, 99.0), np.full(4097, -1.0),
                    np.where(np.arange(4097) % 2 == 1, 99.0, -1.0)):
        kept = _both(gpu_device, (np.arange(64), bits(np.full(64, 50.0))), np.arange(4097) % 64,
                     bits(pattern), np.arange(4097), ">", None, cap=64)
        assert kept == int((pattern > 50).sum())


@pytest.mark.gpu
def test_gpu_upsert_last_rule_wins(gpu_device):
    dev = gpu_device
    for keys, vals in (_gpu_rules(), (np.full(1000, 5), bits(np.arange(1000.0))),
                       (np.array([7]), bits([3.0])),
                       (np.concatenate([np.arange(999), np.arange(999)[::-1]]),
                        bits(np.arange(1998.0)))):
        a, b = _table(1000), _table(1000, dev)
        K.lookup_upsert(a, T(keys), T(vals))
        K.lookup_upsert(b, T(keys, dev), T(vals, dev))
        assert torch.equal(a, b.cpu())


@pytest.mark.gpu
def test_gpu_more_tiles_than_one_scan_round_cap_one_and_one_key(gpu_device):
    """1025 tiles with one kept row each (the scan's carry round); a table of one row; a batch
    whose keys all lie beyond the table; a batch of one key."""
    ntiles = 1025
    n = ntiles * K.LOOKUP_TILE
    vals = np.full(n, 1.0)
    hot = np.arange(ntiles) * K.LOOKUP_TILE + (np.arange(ntiles) * 37) % K.LOOKUP_TILE
    vals[hot] = 99.0
    keys = np.arange(n) % 1000
    rules = (np.arange(1000), bits(np.full(1000, 50.0)))
    assert _both(gpu_device, rules, keys, bits(vals), np.arange(n), ">", None, 1000) == ntiles
    one = (np.array([0]), bits([50.0]))
    m = 3 * K.LOOKUP_TILE + 5
    v = bits(np.where(np.arange(m) % 3 == 0, 99.0, 1.0))
    assert _both(gpu_device, one, np.arange(m) % 2, v, np.arange(m), ">", None, cap=1) \
        == int(((np.arange(m) % 3 == 0) & (np.arange(m) % 2 == 0)).sum())
    assert _both(gpu_device, one, np.arange(m) + 1, v, np.arange(m), ">", None, cap=1) == 0
    assert _both(gpu_device, one, np.arange(m) + 1, v, np.arange(m), ">", bit(2.0), cap=1) \
        == -(-m // 3)
    assert _both(gpu_device, one, np.zeros(m), v, np.arange(m), ">", None, cap=1) == -(-m // 3)
    assert _both(gpu_device, one, np.zeros(m), v, np.arange(m), None, bit(0.0), cap=1) == m


@pytest.mark.gpu
@pytest.mark.parametrize("when", WHENS, ids=[str(w) for w in WHENS])
def test_gpu_operator_equals_model(gpu_device, when):
    _engine_vs_model(when, None if when in (">", "<") else 1.0, dev=gpu_device, steps=20,
                     seed=9, snapshot_at=11)
