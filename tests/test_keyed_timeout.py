"""Keyed event-time timers (csrc/mxs_timeout.h): the C++ twins and the engine operator
(runtime/timeout_operator.py) against a per-record model of CountWithTimeout, NativeTimeoutOp
against the host KeyedProcessOp, and the gfx950 kernels against the twins array for array.
Everything is an integer and compares exactly; one watermark advance compares as a sorted
multiset (ties between keys are unspecified) whose native rows have non-decreasing deadlines."""
from __future__ import annotations

import functools
import heapq
import subprocess

import numpy as np
import pytest
import torch

from mxstream.api import functions as F
from mxstream.api.tuples import Tuple1, Tuple2
from mxstream.ops import kernels as K
from mxstream.runtime.timeout_operator import KeyedTimeoutOperator

TILE = K.TIMEOUT_TILE
NONE = K.TIMEOUT_NONE
KEY_SPACES = [1, 7, 300, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]


def T(a, dev="cpu") -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev)


class Model:
    """CountWithTimeout record by record: a dict per key and a heap of de-duplicated (ts, key)
    timers; a timer emits when it still equals last + timeout."""

    def __init__(self, timeout: int):
        self.timeout, self.state, self.heap, self.seen, self.wm = timeout, {}, [], set(), K.I64_MIN

    def process(self, keys, ts) -> None:
        for k, t in zip(keys.tolist(), ts.tolist()):
            self.state[k] = (self.state.get(k, (0, 0))[0] + 1, t)
            timer = (t + self.timeout, k)
            if timer not in self.seen:
                self.seen.add(timer)
                heapq.heappush(self.heap, timer)

    def advance(self, wm: int) -> list:
        self.wm = max(self.wm, wm)
        out = []
        while self.heap and self.heap[0][0] <= self.wm:
            t, k = heapq.heappop(self.heap)
            self.seen.discard((t, k))
            count, last = self.state[k]
            if t == last + self.timeout:
                out.append((k, count, last, t))
        return out

    def armed(self) -> dict:
        """key -> deadline of the keys whose live timer is still registered."""
        return {k: last + self.timeout for k, (_, last) in self.state.items()
                if (last + self.timeout, k) in self.seen}


@functools.lru_cache(maxsize=None)
def _stream(seed: int, nkeys: int, steps: int = 24):
    """("p", keys, ts) and ("w", wm) calls: disorder within and across batches, equal timestamps
    for one key, late elements whose deadline is already below the watermark, keys that arm again
    after firing, repeated equal watermarks, empty batches and a key range that grows with the
    steps (the capacity doubles across tile boundaries)."""
    rng = np.random.default_rng(seed)
    calls, now, wm = [], 1_000, 0
    for s in range(steps):
        hi = max(1, min(nkeys, 1 + nkeys * (s + 2) // 12))
        n = 0 if s % 7 == 3 else int(rng.integers(1, 400))
        keys = rng.integers(0, hi, n).astype(np.int64)
        ts = now + rng.integers(-30, 30, n)              # disorder, many equal timestamps
        late = rng.random(n) < 0.1
        ts = np.where(late, ts - 500, ts).astype(np.int64)  # deadline already behind the watermark
        if n > 2:
            ts[1] = ts[0]
            keys[1] = keys[0]
        calls.append(("p", keys, ts))
        if s % 5 == 4:
            calls.append(("p", np.zeros(0, np.int64), np.zeros(0, np.int64)))
        if rng.random() < 0.7:
            wm = max(wm, now - int(rng.integers(0, 80)))
            calls.append(("w", wm))
            if rng.random() < 0.4:
                calls.append(("w", wm))                  # repeated equal watermark
            if rng.random() < 0.2:
                calls.append(("w", wm - 50))             # a watermark never goes back
        now += int(rng.integers(5, 60))
    return calls


def _rows(chunks) -> list:
    """advance_watermark's chunks as (key, count, last, deadline) tuples in output order."""
    out = []
    for cols in chunks:
        out.extend(zip(*(c.cpu().tolist() for c in cols)))
    return out


def _check_invariant(op) -> None:
    dl = op.deadline.cpu().numpy()
    tm = op.tile_min.cpu().numpy()
    assert tm.size == -(-dl.size // TILE)
    pad = np.full(tm.size * TILE, NONE, dtype=np.int64)
    pad[:dl.size] = dl
    assert (tm <= pad.reshape(tm.size, TILE).min(axis=1)).all()


def _run(calls, timeout, dev="cpu", snapshot_at=None, check=True):
    """The operator against the model over `calls`, then two INT64_MAX watermarks. Returns every
    advance's rows (sorted) and the final entries."""
    op, model, fired = KeyedTimeoutOperator(timeout, device=dev), Model(timeout), []
    for i, call in enumerate(calls):
        if snapshot_at == i:
            snap = op.snapshot_state()
            op = KeyedTimeoutOperator(timeout, device=dev)
            op.restore_state(snap.columns, snap.meta)
            if check:
                _check_invariant(op)
        if call[0] == "p":
            assert op.process(T(call[1], dev), T(call[2], dev)) == []
            model.process(call[1], call[2])
        else:
            got, want = _rows(op.advance_watermark(call[1])), model.advance(call[1])
            assert sorted(got) == sorted(want)
            assert all(a[3] <= b[3] for a, b in zip(got, got[1:]))
            fired.append(sorted(got))
        if check:
            _check_invariant(op)
    armed = model.armed()
    got, want = _rows(op.advance_watermark(K.I64_MAX)), model.advance(K.I64_MAX)
    assert sorted(got) == sorted(want) and sorted(r[0] for r in got) == sorted(armed)
    assert all(a[3] <= b[3] for a, b in zip(got, got[1:]))
    fired.append(sorted(got))
    assert op.advance_watermark(K.I64_MAX) == [] and model.advance(K.I64_MAX) == []
    _check_invariant(op)
    ids, count, last, dl = op.entries()
    assert ids.tolist() == sorted(model.state)
    assert list(zip(count.tolist(), last.tolist())) == [model.state[k] for k in ids.tolist()]
    assert (dl == NONE).all()
    return fired, (ids.tolist(), count.tolist(), last.tolist())


# ---- twins and engine against the per-record model ---------------------------------------------
@pytest.mark.parametrize("nkeys", KEY_SPACES)
def test_engine_equals_the_per_record_model(nkeys):
    calls = _stream(3, nkeys)
    assert sum(c[0] == "p" for c in calls) + sum(c[0] == "w" for c in calls) >= 20
    fired, _ = _run(calls, timeout=90)
    assert sum(len(f) for f in fired) >= 1
    if nkeys > TILE:
        op = KeyedTimeoutOperator(90)
        assert op.cap < TILE                       # the stream grows it across a tile boundary


def test_rearm_after_firing_late_deadline_and_repeated_watermark():
    op = KeyedTimeoutOperator(10)
    op.process(T([5, 5, 6]), T([100, 90, 95]))     # last arrival, not the largest timestamp
    assert _rows(op.advance_watermark(99)) == []
    assert _rows(op.advance_watermark(100)) == [(5, 2, 90, 100)]
    assert _rows(op.advance_watermark(100)) == []
    assert _rows(op.advance_watermark(105)) == [(6, 1, 95, 105)]
    op.process(T([5]), T([20]))                    # late: the deadline 30 lies behind 105
    assert _rows(op.advance_watermark(50)) == [(5, 3, 20, 30)]   # w = max(50, 105)
    assert op.wm == 105 and _rows(op.advance_watermark(105)) == []
    op.process(T([6, 5]), T([200, 200]))           # both arm again; ties leave in key order
    assert _rows(op.advance_watermark(K.I64_MAX)) == [(5, 4, 200, 210), (6, 2, 200, 210)]
    assert _rows(op.advance_watermark(K.I64_MAX)) == []
    ids, count, last, dl = op.entries()
    assert (ids.tolist(), count.tolist(), last.tolist()) == ([5, 6], [4, 2], [200, 200])


def _sort_spans(dev="cpu"):
    T = lambda a: globals()["T"](a, dev)  # noqa: E731
    op = KeyedTimeoutOperator(10, device=dev)
    big = 1 << 62
    op.process(T([1, 2, 3, 4]), T([big, -big - 5, 0, -7]))       # a span beyond 62 bits
    assert _rows(op.advance_watermark(K.I64_MAX)) == [
        (2, 1, -big - 5, -big + 5), (4, 1, -7, 3), (3, 1, 0, 10), (1, 1, big, big + 10)]
    op.process(T([9, 8, 7]), T([5, 5, 4]))                       # a narrow span, and a tie
    assert _rows(op.advance_watermark(20)) == [(7, 1, 4, 14), (8, 1, 5, 15), (9, 1, 5, 15)]
    op.process(T([6, 5]), T([1, 1]))                             # one deadline for every row
    assert _rows(op.advance_watermark(20)) == [(5, 1, 1, 11), (6, 1, 1, 11)]


def test_deadlines_sort_signed_over_any_span():
    _sort_spans()


def test_growth_keeps_state_and_new_entries_are_unarmed():
    op = KeyedTimeoutOperator(10, capacity=4)
    op.process(T([3]), T([7]))
    op.process(T([2 * TILE + 5]), T([1]))
    assert op.cap >= 2 * TILE + 6 and op.tile_min.numel() == -(-op.cap // TILE)
    _check_invariant(op)
    assert (op.deadline == NONE).sum().item() == op.cap - 2
    assert _rows(op.advance_watermark(17)) == [(2 * TILE + 5, 1, 1, 11), (3, 1, 7, 17)]


def test_unsupported_batches_are_refused():
    op = KeyedTimeoutOperator(10, dense_limit=100)
    for keys, ts in (([100], [1]), ([-1], [1]), ([1], [K.I64_MAX - 10]), ([1], [K.I64_MAX])):
        with pytest.raises(TypeError):
            op.process(T(keys), T(ts))
    op.process(T([99]), T([K.I64_MAX - 11]))       # the largest deadline below the sentinel
    assert _rows(op.advance_watermark(K.I64_MAX - 2)) == []
    assert _rows(op.advance_watermark(K.I64_MAX)) == [(99, 1, K.I64_MAX - 11, K.I64_MAX - 1)]
    for bad in (0, -5, True, 1.5, None):
        with pytest.raises(ValueError):
            KeyedTimeoutOperator(bad)
    with pytest.raises(TypeError):
        op.process(T([1]).to(torch.int32), T([1]))
    m = K.load()
    assert (m.TIMEOUT_TILE, m.TIMEOUT_WORDS, m.TIMEOUT_NONE) == (TILE, TILE // 64, NONE)
    st, dl, tm = K.timeout_tables(8, "cpu")
    with pytest.raises(ValueError):
        K.timeout_update(st, dl, tm, T([8]), T([1]), 10)
    with pytest.raises(ValueError):
        K.timeout_update(st, dl, tm[:0], T([1]), T([1]), 10)
    with pytest.raises(ValueError):
        K.timeout_update(st, dl, tm, T([1]), T([1]), 0)
    with pytest.raises(ValueError):
        K.timeout_mask(dl[1:], tm, 5)              # not 16-byte aligned


# ---- invariants --------------------------------------------------------------------------------
@pytest.mark.parametrize("nkeys", [300, TILE + 1, 2 * TILE + 1])
def test_tile_skipping_changes_no_row_and_no_state(monkeypatch, nkeys):
    res = {}
    for skip in ("1", "0"):
        monkeypatch.setenv("MXS_TIMEOUT_TILESKIP", skip)
        res[skip] = _run(_stream(9, nkeys), timeout=60)   # checks the invariant after every call
    assert res["0"] == res["1"]


def test_a_skipped_tile_keeps_its_bound_and_a_scanned_tile_gets_the_exact_minimum(monkeypatch):
    for skip in ("1", "0"):
        monkeypatch.setenv("MXS_TIMEOUT_TILESKIP", skip)
        op = KeyedTimeoutOperator(100, capacity=2 * TILE + 5)
        op.process(T([7, TILE + 1, 2 * TILE + 4]), T([200, 50, 10]))
        op.process(T([7]), T([400]))               # tile 0: bound 300, true minimum 500
        assert op.tile_min.tolist() == [300, 150, 110]
        assert _rows(op.advance_watermark(120)) == [(2 * TILE + 4, 1, 10, 110)]
        # only the last, partial tile was due: tile 0 keeps its stale bound when it is skipped
        assert op.tile_min.tolist() == [300 if skip == "1" else 500, 150, NONE]
        tm = K.timeout_mask(op.deadline, op.tile_min, 120)        # nothing due: every tile skipped
        assert tm.total == 0 and tm.counts.tolist() == [0, 0, 0]
        assert _rows(op.advance_watermark(300)) == [(TILE + 1, 1, 50, 150)]
        assert op.tile_min.tolist() == [500, NONE, NONE]          # tile 0 scanned: exact now
        _check_invariant(op)


# ---- checkpoints -------------------------------------------------------------------------------
def test_snapshot_in_mid_stream_restores_into_a_fresh_operator():
    calls = _stream(5, TILE + 1)
    want = _run(calls, timeout=90)
    for at in (len(calls) // 3, len(calls) // 2):
        assert _run(calls, timeout=90, snapshot_at=at) == want
    op = KeyedTimeoutOperator(90)
    op.process(T([1, 2, 2]), T([5, 6, 7]))
    op.advance_watermark(95)
    snap = op.snapshot_state()
    assert snap.meta["kind"] == "count_timeout" and snap.meta["timeout"] == 90
    assert snap.meta["wm"] == 95 and snap.meta["metrics"]["num_records_in"] == 3
    assert {k: v.tolist() for k, v in snap.columns.items()} == {
        "key": [1, 2], "count": [1, 2], "last": [5, 7], "deadline": [NONE, 97]}
    with pytest.raises(ValueError, match="different timeout"):
        KeyedTimeoutOperator(91).restore_state(snap.columns, snap.meta)
    with pytest.raises(ValueError, match="different timeout"):
        KeyedTimeoutOperator(90).restore_state(snap.columns, {"kind": "lookup"})
    fresh = KeyedTimeoutOperator(90)
    fresh.restore_state(snap.columns, snap.meta)
    assert fresh.wm == 95 and fresh.metrics.num_records_out == 1
    assert _rows(fresh.advance_watermark(97)) == [(2, 2, 7, 97)]


# ---- NativeTimeoutOp against the host operator ---------------------------------------------------
def _ctx():
    from mxstream.runtime.operators import OpContext

    return OpContext("timeout", 4, 128, lambda: 0, "EventTime")


def _host(timeout, key_pos=0):
    from mxstream.runtime.operators import KeyedProcessOp

    op = KeyedProcessOp(lambda v: v[key_pos], F.CountWithTimeout(timeout))
    op.open(_ctx())
    return op


def _native(timeout, key_pos=0, **kw):
    from mxstream.runtime.native_ops import NativeTimeoutOp

    op = NativeTimeoutOp(fn=F.CountWithTimeout(timeout), key_pos=key_pos,
                         device=kw.pop("device", "cpu"),
                         fallback_factory=lambda: _host(timeout, key_pos), **kw)
    op.open(_ctx())
    return op


def _segments(items) -> list:
    """Output as the watermarks and, between them, the sorted (text, ts, subtask) rows."""
    from mxstream.runtime.columnar import expand_columns
    from mxstream.runtime.operators import WM

    out, rows = [], []
    for it in expand_columns(list(items)):
        if isinstance(it, WM):
            out.extend([sorted(rows), it])
            rows = []
        else:
            rows.append((str(it.value), it.ts, it.subtask))
    return out + [sorted(rows)]


def _passes(seed, mode, passes=12):
    """Passes of records ("recs"), column batches ("str" / "int" keys) or both, with watermarks."""
    from mxstream.ops.native import load
    from mxstream.ops.text import FK_DOUBLE, FK_LONG, FK_STR
    from mxstream.runtime.columnar import ColumnBatch
    from mxstream.runtime.operators import WM, Rec

    rng = np.random.default_rng(seed)
    sd = load().StringDict()
    str_keys = mode in ("recs", "str")
    key = (lambda i: f"host{i}") if str_keys else (lambda i: int(i) * 3)
    now = 1_000
    for _ in range(passes):
        items = []
        for _ in range(int(rng.integers(1, 5))):
            n = int(rng.integers(1, 40))
            ks = rng.integers(0, 25, n)
            tsa = (now + rng.integers(-20, 20, n)).astype(np.int64)
            now += int(rng.integers(5, 50))
            if mode != "recs" and rng.integers(0, 3):
                kcol = (np.array([sd.intern(key(k)) for k in ks]) if str_keys
                        else np.array([key(k) for k in ks], dtype=np.int64))
                items.append(ColumnBatch(n, [kcol, np.arange(n, dtype=np.float64)],
                                         (FK_STR if str_keys else FK_LONG, FK_DOUBLE),
                                         sd if str_keys else None, tsa, np.zeros(n, np.int32)))
            else:
                items.extend(Rec(Tuple2(key(k), 0.5), int(t), 0) for k, t in zip(ks, tsa))
            if rng.integers(0, 2):
                items.append(WM(now - int(rng.integers(0, 60))))
        yield items


@pytest.mark.parametrize("mode", ["recs", "str", "int"])
def test_native_operator_equals_the_host_operator(mode):
    from mxstream.runtime.columnar import ColumnBatch, expand_columns
    from mxstream.runtime.operators import WM

    native, host = _native(70), _host(70)
    rows = 0
    for items in list(_passes(17, mode)) + [[WM(K.I64_MAX)], [WM(K.I64_MAX)]]:
        got, want = native.process(list(items)), host.process(expand_columns(list(items)))
        assert all(isinstance(it, (ColumnBatch, WM)) for it in got)
        assert _segments(got) == _segments(want)
        for cb in got:
            if isinstance(cb, ColumnBatch):
                assert (np.diff(cb.ts) >= 0).all()
                rows += cb.n
    assert native.fallback is None and native.op is not None and rows > 25
    assert native.finish() == host.finish() == []


def _rec(value, ts=5):
    from mxstream.runtime.operators import Rec

    return Rec(value, ts, 0)


def _double_key_batch():
    from mxstream.ops.text import FK_DOUBLE
    from mxstream.runtime.columnar import ColumnBatch

    return [ColumnBatch(2, [np.array([1.5, 2.5])], (FK_DOUBLE,), None,
                        np.array([5, 6], dtype=np.int64), np.zeros(2, np.int32))]


FALLBACKS = {
    "non_tuple": (lambda: [_rec(["a", 1])], 0, None),
    "arity": (lambda: [_rec(Tuple1("a"))], 1, IndexError),
    "double_key": (lambda: [_rec(Tuple2(1.5, "x"))], 0, None),
    "double_key_column": (_double_key_batch, 0, None),
    "mixed_keys": (lambda: [_rec(Tuple2("a", 1)), _rec(Tuple2(3, 1))], 0, None),
    "negative_key": (lambda: [_rec(Tuple2(-1, 1))], 0, None),
    "key_at_dense_limit": (lambda: [_rec(Tuple2(100, 1))], 0, None),
    "no_timestamp": (lambda: [_rec(Tuple2("a", 1), K.I64_MIN)], 0, ValueError),
    "overflow": (lambda: [_rec(Tuple2("a", 1), K.I64_MAX - 70)], 0, None),
}


@pytest.mark.parametrize("case", sorted(FALLBACKS))
def test_unsupported_data_falls_back_before_state_exists_and_raises_after(case):
    from mxstream.runtime.columnar import expand_columns
    from mxstream.runtime.operators import WM

    make, key_pos, host_error = FALLBACKS[case]
    good_key = 3 if case in ("negative_key", "key_at_dense_limit", "double_key_column") else "b"
    good = [_rec(Tuple2(good_key, good_key), 1)]
    tail = [WM(50), WM(K.I64_MAX)]
    # before native state exists: the host operator, told the watermark that was pending
    op = _native(70, key_pos, dense_limit=100)
    assert op.process([WM(40)]) == [WM(40)] and op.op is None
    if host_error is not None:
        with pytest.raises(host_error):
            op.process(make() + tail)
        assert op.fallback is not None and op.op is None and op.fallback.wm == 40
    else:
        host = _host(70, key_pos)
        host.process([WM(40)])
        got = op.process(make() + tail)
        assert op.fallback is not None and op.op is None
        assert _segments(got) == _segments(host.process(expand_columns(make()) + tail))
        assert sum(len(s) for s in _segments(got) if isinstance(s, list)) >= 1
    # afterwards: an error
    op = _native(70, key_pos, dense_limit=100)
    op.process(good + [WM(2)])
    assert op.op is not None and op.fallback is None
    with pytest.raises(ValueError if case == "no_timestamp" else TypeError):
        op.process(make() + tail)
    assert op.fallback is None


def test_native_operator_snapshot_restore_and_foreign_function():
    passes = list(_passes(23, "str", passes=10))
    ref, op = _native(70), _native(70)
    want = [_segments(ref.process(list(p))) for p in passes]
    for i, p in enumerate(passes):
        if i == 5:
            snap = op.snapshot()
            assert snap["count_timeout"] == ("count_timeout", 70)
            assert snap["engine"]["meta"]["kind"] == "count_timeout"
            op = _native(70)
            op.restore(snap)
        assert _segments(op.process(list(p))) == want[i]
    with pytest.raises(ValueError, match="different timeout"):
        _native(71).restore(snap)
    with pytest.raises(RuntimeError, match="pending"):
        op.pending.append(_rec(Tuple2("a", 1)))
        op.snapshot()


def test_several_ranks_fall_back_in_open():
    from mxstream.runtime.native_ops import NativeTimeoutOp

    class Comm:
        world = 2

    ctx = _ctx()
    ctx.comm = Comm()
    op = NativeTimeoutOp(fn=F.CountWithTimeout(70), key_pos=0, device="cpu",
                         fallback_factory=lambda: _host(70))
    op.open(ctx)
    assert op.fallback is not None and op.op is None


# ---- sanitizer -----------------------------------------------------------------------------
def test_sanitizer_harness_runs_clean():
    from mxstream.build import build_sanitize_timeout

    res = subprocess.run([str(build_sanitize_timeout())], capture_output=True, text=True,
                         timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.strip().splitlines()[-1] == "timeout sanitize ok"


# ---- GPU ---------------------------------------------------------------------------------------
def _both(dev, cap, steps):
    """The same updates and firings on the twin and on the device from fresh tables of `cap` key
    ids: state, deadline, tile_min, the scanned tiles' words, counts, offsets and the emitted
    columns are equal after every step. Returns the totals of the firings."""
    tabs = {d: K.timeout_tables(cap, d) for d in ("cpu", dev)}
    totals = []

    def same_tables():
        for a, b in zip(tabs["cpu"], tabs[dev]):
            assert torch.equal(a, b.cpu())

    for step in steps:
        if step[0] == "p":
            for d, (st, dl, tm) in tabs.items():
                K.timeout_update(st, dl, tm, T(step[1], d), T(step[2], d), step[3])
            same_tables()
            continue
        res = []
        for d, (st, dl, tm) in tabs.items():
            scanned = (tm.cpu() <= step[1]) | (not K.load().timeout_tileskip())
            m = K.timeout_mask(dl, tm, step[1])
            out = K.timeout_emit(st, dl, m)
            res.append((scanned, m.words.cpu().view(-1, 64), m.counts.cpu(), m.offsets.cpu(),
                        m.total, [c.cpu() for c in out]))
        (s0, w0, c0, o0, t0, out0), (s1, w1, c1, o1, t1, out1) = res
        assert torch.equal(s0, s1) and torch.equal(w0[s0], w1[s1])
        assert torch.equal(c0, c1) and torch.equal(o0, o1) and t0 == t1
        assert all(torch.equal(a, b) for a, b in zip(out0, out1))
        assert (c0[~s0] == 0).all() and int(c0.sum()) == t0 == out0[0].numel()
        same_tables()
        totals.append(t0)
    return totals


BATCHES = [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]


def _tile_ends(cap: int) -> np.ndarray:
    ends = np.concatenate([np.arange(0, cap, TILE), np.arange(TILE - 1, cap, TILE), [cap - 1]])
    return np.unique(ends)


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [1, TILE, TILE + 1, 3 * TILE])
def test_gpu_kernels_equal_the_twins(gpu_device, cap):
    rng = np.random.default_rng(cap)
    ends = _tile_ends(cap)
    for n in BATCHES:
        ts = rng.integers(0, 1_000, n).astype(np.int64)
        patterns = {
            "hot": np.full(n, cap - 1),                          # one run: the whole batch
            "distinct": rng.permutation(max(n, cap))[:n] % cap,  # distinct while n <= cap
            "tile_ends": ends[rng.integers(0, ends.size, n)],
        }
        for keys in patterns.values():
            again = rng.integers(0, cap, 50)
            totals = _both(gpu_device, cap, [
                ("p", keys, ts, 100), ("w", 600),
                ("p", again, rng.integers(400, 2_000, 50), 100),   # some keys arm again, some late
                ("w", 600), ("w", 1_500), ("w", K.I64_MAX), ("w", K.I64_MAX)])
            assert totals[-1] == 0 and (n == 0 or sum(totals) >= 1)


@pytest.mark.gpu
def test_gpu_one_due_key_in_each_of_1025_tiles_then_skipped_and_partial_firings(gpu_device,
                                                                                monkeypatch):
    """1025 tiles with one due key each (the scan's carry round), a firing where every tile is
    skipped, and one where only the last, partial tile is scanned."""
    ntiles = 1025
    cap = (ntiles - 1) * TILE + 77
    due = np.arange(ntiles) * TILE + (np.arange(ntiles) * 37) % 77
    later = (due + 1) % cap
    totals = _both(gpu_device, cap, [
        ("p", np.concatenate([due, later]), np.concatenate([np.zeros(ntiles), np.full(ntiles, 900)]),
         100),
        ("w", 100),                  # one key of every tile
        ("w", 100), ("w", 999),      # every tile's bound is 1000: all skipped
        ("p", np.array([cap - 1]), np.array([5]), 100),
        ("w", 999),                  # only the last, partial tile is scanned
        ("w", 1_000)])
    assert totals == [ntiles, 0, 0, 1, ntiles]
    monkeypatch.setenv("MXS_TIMEOUT_TILESKIP", "0")
    assert _both(gpu_device, 2 * TILE + 5, [
        ("p", np.array([7, TILE + 1, 2 * TILE + 4]), np.array([200, 50, 10]), 100),
        ("w", 120), ("w", 120), ("w", 300), ("w", K.I64_MAX)]) == [1, 0, 2, 0]


@pytest.mark.gpu
def test_gpu_operator_equals_the_model_with_and_without_tile_skipping(gpu_device, monkeypatch):
    calls = _stream(7, 2 * TILE + 1, steps=20)
    res = {}
    for skip in ("1", "0"):
        monkeypatch.setenv("MXS_TIMEOUT_TILESKIP", skip)
        res[skip] = _run(calls, timeout=90, dev=gpu_device, snapshot_at=len(calls) // 2)
    assert res["0"] == res["1"] == _run(calls, timeout=90, check=False)


@pytest.mark.gpu
def test_gpu_deadlines_sort_signed_over_any_span(gpu_device):
    _sort_spans(gpu_device)


@pytest.mark.gpu
def test_gpu_native_operator_takes_device_batches(gpu_device):
    from mxstream.ops.text import FK_DOUBLE, FK_LONG
    from mxstream.runtime.columnar import DeviceColumnBatch, expand_columns
    from mxstream.runtime.operators import WM

    native, host = _native(70, device=gpu_device), _host(70)
    rng = np.random.default_rng(4)
    for step in range(6):
        n = 500
        keys = rng.integers(0, 60, n).astype(np.int64)
        ts = (1_000 + 40 * step + rng.integers(-20, 20, n)).astype(np.int64)
        cb = DeviceColumnBatch(n, [T(keys, gpu_device), torch.zeros(n, dtype=torch.float64,
                                                                    device=gpu_device)],
                               (FK_LONG, FK_DOUBLE), None, T(ts, gpu_device), parallelism=4)
        items = [cb, WM(1_000 + 40 * step)] + ([WM(K.I64_MAX)] if step == 5 else [])
        assert _segments(native.process(list(items))) == \
            _segments(host.process(expand_columns(list(items))))
    assert native.fallback is None and native.op.device.type == "cuda"
