"""Counter rates (csrc/mxs_rate.h): the C++ twin and the engine operator
(runtime/rate_operator.py) against a per-record model of CounterRate (a dict per key), and the
gfx950 kernels against the twin array for array. Everything is an integer or a bit pattern and
compares exactly, row for row and in order: the rate's bits included, which is the check that
the device's f64 multiply and divide round as the host's do."""
from __future__ import annotations

import functools
import operator
import struct
import subprocess

import numpy as np
import pytest
import torch

from mxstream.ops import kernels as K
from mxstream.runtime.rate_operator import KeyedRateOperator

NONE = K.RATE_NONE
KEY_SPACES = [1, 7, 300, 4095, 4096, 4097, 8193]
SEEDS = [0, 1]
NAN, INF = float("nan"), float("inf")
LIM = K.SUSTAIN_TS_LIMIT
CMP = {">": operator.gt, ">=": operator.ge, "<": operator.lt, "<=": operator.le,
       "==": operator.eq, "!=": operator.ne}

# name -> the rule. "lt": the threshold lies near the median rate of the streams below, which
# falls with the key space (LT_THRESHOLD: the fewer keys, the more increments and the fewer
# milliseconds lie between two accepted samples of a key); "ne": the
# double streams of this configuration hold infinite and NaN readings, whose rates are NaN, and
# every stream holds increments of 0, whose rate 0.0 is the one that fails ``!= 0.0``.
CONFIGS = {
    "plain": dict(per_ms=1000),
    "gap": dict(per_ms=1000, max_gap=40),
    "lt": dict(per_ms=1000, when="<"),
    "ne": dict(per_ms=7, when="!=", threshold=0.0),
}
LT_THRESHOLD = {1: 8e5, 7: 2.5e5, 300: 7.5e3}   # wider key spaces: 2e3


def _rule(config: str, nkeys: int) -> dict:
    if config == "lt":
        return dict(CONFIGS[config], threshold=LT_THRESHOLD.get(nkeys, 2e3))
    return CONFIGS[config]


def T(a, dev="cpu") -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev)


def fbits(x: float) -> int:
    return struct.unpack("<q", struct.pack("<d", x))[0]


def bits(vals, is_float) -> np.ndarray:
    """The value column as the engine takes it: doubles' bit patterns, or the longs."""
    if is_float:
        return np.ascontiguousarray(vals, dtype=np.float64).view(np.int64)
    return np.ascontiguousarray(vals, dtype=np.int64)


def wrap64(x: int) -> int:
    return (x + (1 << 63)) % (1 << 64) - (1 << 63)


class Model:
    """CounterRate.process_element record by record: key -> (last_ts, last value, the batch
    that stored it, stragglers ignored since)."""

    def __init__(self, per_ms=1000, when=None, threshold=None, max_gap=None):
        self.per_ms, self.when, self.threshold, self.max_gap = per_ms, when, threshold, max_gap
        self.state, self.batch, self.out_of_order = {}, 0, 0
        # what the streams are meant to hold
        self.resets = self.stragglers = self.equal_ts = self.gap_suppressed = 0
        # based elements whose baseline stems from an earlier batch / lies behind a straggler
        self.carried = self.past_a_straggler = self.ignored_runs = self.nan_rates = 0
        self.kept = self.failed_rule = 0

    def process(self, keys, vals, ts, is_float) -> list:
        """Rows (key, rate bits, inc bits, dt, ts) in arrival order."""
        out, seen, accepted = [], set(), set()
        vals = np.asarray(vals, dtype=np.float64 if is_float else np.int64).tolist()
        for k, v, t in zip(np.asarray(keys).tolist(), vals, np.asarray(ts).tolist()):
            seen.add(k)
            cur = self.state.get(k)
            if cur is None:
                self.state[k] = (t, v, self.batch, 0)
                accepted.add(k)
                continue
            last_ts, last, born, ignored = cur
            if t <= last_ts:
                self.out_of_order += 1
                self.stragglers += t < last_ts
                self.equal_ts += t == last_ts
                self.state[k] = (last_ts, last, born, ignored + 1)
                continue
            accepted.add(k)
            dt = t - last_ts
            if v >= last:
                inc = v - last if is_float else wrap64(v - last)
            else:
                inc = v
                self.resets += 1
            self.state[k] = (t, v, self.batch, 0)
            self.carried += born < self.batch
            self.past_a_straggler += ignored > 0
            if self.max_gap is not None and dt > self.max_gap:
                self.gap_suppressed += 1
                continue
            rate = float(inc) * float(self.per_ms) / float(dt)
            if self.when is None or CMP[self.when](rate, float(self.threshold)):
                out.append((k, fbits(rate), fbits(inc) if is_float else inc, dt, t))
                self.kept += 1
                self.nan_rates += rate != rate
            else:
                self.failed_rule += 1
        self.ignored_runs += len(seen - accepted)
        self.batch += 1
        return out

    def table_rows(self, cap: int, is_float) -> np.ndarray:
        st = np.zeros((cap, 2), dtype=np.int64)
        st[:, 0] = NONE
        for k, (last_ts, last, _, _) in self.state.items():
            st[k] = (last_ts, fbits(last) if is_float else last)
        return st


@functools.lru_cache(maxsize=None)
def _stream(seed: int, nkeys: int, steps: int = 24):
    """The sustained-alert tests' call generator -- ("p", keys, ts, counter, special) and
    ("w", wm) calls: 0 to 399 rows per step, +-30 ms of disorder, 10 % of the rows 500 ms late,
    equal timestamps forced on one key, empty batches, a key range that grows with the steps and
    a quarter of the rows on key 0 -- with a value column that is a running counter per key in
    arrival order: increments U[0, 1000), 5 % of them 0, about 2 % resets to a small reading.
    `special` marks 20 % of the rows (1: an infinite reading, 2: a NaN) for the configuration
    that wants them. Step 10 is followed by a pause of 200 ms (a gap for every key, one key
    included) and every row of step 13 is late (a batch whose runs are all ignored)."""
    rng = np.random.default_rng(seed)
    calls, now, wm = [], 1_000, 0
    counter = np.zeros(nkeys, dtype=np.int64)
    for s in range(steps):
        hi = max(1, min(nkeys, 1 + nkeys * (s + 2) // 12))
        n = 0 if s % 7 == 3 else int(rng.integers(1, 400))
        keys = rng.integers(0, hi, n).astype(np.int64)
        keys[rng.random(n) < 0.25] = 0
        ts = now + rng.integers(-30, 30, n)
        late = rng.random(n) < 0.1
        if s == 13:
            late[:] = True
        ts = np.where(late, ts - 500, ts).astype(np.int64)
        if n > 2:
            ts[1] = ts[0]
            keys[1] = keys[0]
        incs = np.where(rng.random(n) < 0.05, 0, rng.integers(0, 1000, n))
        reset = rng.random(n) < 0.02
        small = rng.integers(0, 10, n)
        vals = np.empty(n, dtype=np.int64)
        for i, k in enumerate(keys.tolist()):
            counter[k] = small[i] if reset[i] else counter[k] + incs[i]
            vals[i] = counter[k]
        special = np.where(rng.random(n) < 0.2, rng.integers(1, 3, n), 0)
        calls.append(("p", keys, ts, vals, special))
        if s % 5 == 4:
            z = np.zeros(0, np.int64)
            calls.append(("p", z, z, z, z))
        if rng.random() < 0.7:
            wm = max(wm, now - int(rng.integers(0, 80)))
            calls.append(("w", wm))
        now += int(rng.integers(5, 60)) + (200 if s == 10 else 0)
    return calls


def _values(call, config: str, is_float: bool) -> np.ndarray:
    """The value column of a "p" call: the counter as longs, or as doubles a tenth of it (so
    that the subtraction rounds), with the special readings where the configuration has them."""
    if not is_float:
        return call[3]
    vals = call[3].astype(np.float64) * 0.1
    if config == "ne":
        vals = np.where(call[4] == 1, INF, np.where(call[4] == 2, NAN, vals))
    return vals


@functools.lru_cache(maxsize=None)
def _expected(config: str, is_float: bool, seed: int, nkeys: int):
    """The model over a stream, computed once: every "p" call's rows, the final table, and the
    model itself for what it has seen."""
    model = Model(**_rule(config, nkeys))
    rows = [model.process(c[1], _values(c, config, is_float), c[2], is_float)
            for c in _stream(seed, nkeys) if c[0] == "p"]
    return rows, model.table_rows(nkeys, is_float), model


CASES = [(c, f, s, k) for c in CONFIGS for f in (False, True) for s in SEEDS for k in KEY_SPACES]


def _rows(chunks) -> list:
    out = []
    for cols in chunks:
        out.extend(zip(*(c.cpu().tolist() for c in cols)))
    return out


# ---- the streams hold what they are meant to test ---------------------------------------------
@pytest.mark.parametrize("config,is_float,seed,nkeys", CASES)
def test_streams_hold_what_they_test(config, is_float, seed, nkeys):
    rows, _, m = _expected(config, is_float, seed, nkeys)
    assert m.resets > 0 and m.stragglers > 0 and m.equal_ts > 0
    assert m.carried > 0 and m.past_a_straggler > 0 and m.ignored_runs > 0 and m.kept > 0
    assert (m.gap_suppressed > 0) == (config == "gap")
    # (one key's accepted samples lie stragglers apart, whose increments they carry: no 0.0)
    assert (m.failed_rule > 0) == (config == "lt" or (config == "ne" and nkeys > 1))
    assert (m.nan_rates > 0) == (config == "ne" and is_float)
    calls = [c for c in _stream(seed, nkeys) if c[0] == "p"]
    if nkeys <= 7:
        # a quarter of at most 399 rows stays below 128 in a wide key space: there the directed
        # 200-row cases are the long runs
        assert max(np.bincount(c[1]).max() for c in calls if len(c[1])) > 128
    assert sum(len(c[1]) == 0 for c in calls) >= 1
    assert sum(len(r) for r in rows) == m.kept


# ---- the twin and the engine against the per-record model -------------------------------------
def _kw(config, nkeys):
    c = _rule(config, nkeys)
    thr = c.get("threshold")
    return dict(per_ms=c["per_ms"], when=c.get("when"), max_gap=c.get("max_gap"),
                threshold_bits=0 if thr is None else fbits(float(thr)))


def _update(state, call, config, is_float, dev="cpu"):
    nkeys = state.shape[0]
    return K.rate_update(state, T(call[1], dev), T(bits(_values(call, config, is_float), is_float),
                                                   dev), T(call[2], dev),
                         kind=K.SUSTAIN_DOUBLE if is_float else K.SUSTAIN_LONG, **_kw(config, nkeys))


@pytest.mark.parametrize("config,is_float,seed,nkeys", CASES)
def test_twin_equals_the_per_record_model(config, is_float, seed, nkeys):
    want, table, model = _expected(config, is_float, seed, nkeys)
    state = K.rate_table(nkeys, "cpu")
    got, ignored = [], 0
    for c in _stream(seed, nkeys):
        if c[0] == "p":
            cols, ooo = _update(state, c, config, is_float)
            got.append(_rows([cols]))
            ignored += ooo
    assert got == want
    assert ignored == model.out_of_order
    assert np.array_equal(state.numpy(), table)


def _make(config, nkeys, dev="cpu", **kw):
    c = _rule(config, nkeys)
    return KeyedRateOperator(c["per_ms"], c.get("when"), c.get("threshold"), c.get("max_gap"),
                             device=dev, **kw)


def _run_engine(config, is_float, seed, nkeys, dev="cpu"):
    calls = _stream(seed, nkeys)
    op, got = _make(config, nkeys, dev), []
    for i, c in enumerate(calls):
        if i == len(calls) // 2:
            snap = op.snapshot_state()
            assert snap.meta["kind"] == "counter_rate"
            assert snap.meta["per_ms"] == CONFIGS[config]["per_ms"]
            assert snap.meta["out_of_order"] == op.out_of_order > 0
            assert snap.meta["value_kind"] == (K.SUSTAIN_DOUBLE if is_float else K.SUSTAIN_LONG)
            assert sorted(snap.columns) == ["key", "last_ts", "last_value"]
            op = _make(config, nkeys, dev, capacity=2)   # a smaller table: the restore grows it
            op.restore_state(snap.columns, snap.meta)
        if c[0] == "w":
            assert op.advance_watermark(c[1]) == []
            continue
        chunks = op.process(T(c[1], dev), T(bits(_values(c, config, is_float), is_float), dev),
                            T(c[2], dev), is_float=is_float)
        assert len(chunks) <= 1 and all(len(cols) == 5 for cols in chunks)
        got.append(_rows(chunks))
    want, table, model = _expected(config, is_float, seed, nkeys)
    assert got == want
    assert op.out_of_order == model.out_of_order
    st = op.state.cpu().numpy()     # the capacity covers the largest key seen, not nkeys
    full = Model().table_rows(max(op.cap, nkeys), is_float)
    full[:nkeys] = table
    assert np.array_equal(st, full[:op.cap]) and (full[op.cap:, 0] == NONE).all()
    ids, last_ts, last = op.entries()
    seen = np.nonzero(table[:, 0] != NONE)[0]
    assert ids.tolist() == seen.tolist()
    assert last_ts.tolist() == table[seen, 0].tolist() and last.tolist() == table[seen, 1].tolist()
    return op


@pytest.mark.parametrize("config,is_float,seed,nkeys", CASES)
def test_engine_equals_the_per_record_model_across_a_snapshot(config, is_float, seed, nkeys):
    op = _run_engine(config, is_float, seed, nkeys)
    if nkeys > 4096:
        assert op.cap >= 4096  # it grew from 2


# ---- hand-built batches: the smallest shapes where the scan can go wrong ----------------------
def _one_key(vals, ts=None, key=0):
    n = len(vals)
    return (np.full(n, key), vals, np.arange(n) if ts is None else ts)


def _hand_cases():
    """name -> (rule, [batches (keys, vals, ts)], is_float, capacity)."""
    c = {}
    rng = np.random.default_rng(3)
    plain = dict(per_ms=1000)
    count = lambda n: np.cumsum(rng.integers(0, 1000, n))  # noqa: E731
    c["one_row"] = (plain, [_one_key([5], [4], key=9), _one_key([9], [5], key=9),
                            _one_key([9], [5], key=9)], False, 1024)
    c["empty"] = (plain, [_one_key([]), _one_key([1]), _one_key([])], False, 1024)
    # key 1's run begins at sorted row 63 of the first chunk; the arrival order interleaves and
    # the random timestamps make most rows stragglers
    keys = np.array([0] * 63 + [1] * 70 + [2] * 3)
    order = rng.permutation(keys.size)
    c["run_begins_at_row_63"] = (plain, [(keys[order], count(keys.size),
                                          rng.integers(0, 50, keys.size)),
                                         (keys[order], count(keys.size),
                                          rng.integers(40, 90, keys.size))], False, 1024)
    for L in (64, 65):   # key 0's run ends at sorted row 63 / row 64
        keys = np.array([0] * L + [1] * 5)
        order = rng.permutation(keys.size)
        c[f"run_ends_at_row_{L - 1}"] = (plain, [(keys[order], count(keys.size),
                                                  np.sort(rng.integers(0, 300, keys.size)))] * 2,
                                         False, 1024)
    for f in (False, True):
        c[f"a_200_row_key_{'double' if f else 'long'}"] = (
            plain, [_one_key(count(200) * (0.1 if f else 1), np.arange(200) * 3),
                    _one_key(count(200) * (0.1 if f else 1), np.arange(200) * 3 + 400)], f, 1024)
    # the record high sits in the first chunk: every later chunk is all stragglers and the carry
    # must survive the walk untouched
    ts = rng.integers(0, 1000, 200)
    ts[10] = 5000
    c["a_200_row_key_with_its_high_in_the_first_chunk"] = (
        plain, [_one_key(count(200), ts), _one_key([7, 8], [5000, 5001])], False, 1024)
    ts = np.concatenate([np.arange(60), rng.integers(0, 60, 140)])
    c["a_200_row_key_whose_later_chunks_are_stragglers"] = (
        dict(per_ms=1000, max_gap=1), [_one_key(count(200), ts)], False, 1024)
    keys = np.concatenate([np.full(1000, 77), np.arange(200)])
    rng.shuffle(keys)
    c["a_1000_row_key_among_200"] = (plain, [(keys, count(1200), rng.integers(0, 5000, 1200)),
                                             (keys, count(1200), rng.integers(4000, 9000, 1200))],
                                     False, 1024)
    c["a_state_row_newer_than_the_batch"] = (
        plain, [(np.array([0, 1, 2]), [1, 2, 3], [1000, 1000, 10]),
                (np.array([0, 1, 0, 2, 1, 0]), [5, 6, 7, 8, 9, 10], [5, 999, 1000, 11, 7, 8]),
                (np.array([0, 1]), [20, 30], [1001, 1001])], False, 1024)
    c["long_values_across_the_wrap"] = (
        plain, [_one_key([K.I64_MAX, K.I64_MIN + 5, K.I64_MAX, K.I64_MIN, -1, 0, K.I64_MAX])],
        False, 1024)
    c["minus_zero_inf_and_nan_counters"] = (
        dict(per_ms=7), [_one_key([1.0, NAN, 0.1, 0.0, -0.0, INF, INF, NAN, NAN, -INF, 3.0, -0.0,
                                   0.0])], True, 1024)
    c["nan_first"] = (plain, [_one_key([NAN, 1.0, 2.0])], True, 1024)
    for per in (1, 1000, 60000, 7):   # 7: the product is inexact, the quotient rounds again
        c[f"per_{per}"] = (dict(per_ms=per), [_one_key(np.cumsum(rng.uniform(0, 9, 90)),
                                                       np.cumsum(rng.integers(1, 30, 90)))],
                           True, 1024)
        c[f"per_{per}_long"] = (dict(per_ms=per), [_one_key(count(90),
                                                            np.cumsum(rng.integers(1, 30, 90)))],
                                False, 1024)
    c["per_7_beyond_2_53"] = (dict(per_ms=7), [_one_key([0, (1 << 53) + 1, (1 << 62) + 3,
                                                         K.I64_MAX])], False, 1024)
    c["dt_near_2_62"] = (plain, [_one_key([0, 3, 9, 10], [-LIM + 1, 0, LIM - 2, LIM - 1])],
                         False, 1024)
    c["dt_near_2_62_with_a_gap"] = (
        dict(per_ms=1000, max_gap=LIM - 1),
        [_one_key([0.0, 3.0, 9.0, 10.0, 11.0], [-LIM + 1, 1, 2, LIM - 3, LIM - 2])],
        True, 1024)
    c["a_subnormal_rate"] = (dict(per_ms=1), [_one_key([0.0, 1e-300, 3e-300, 3.5e-300],
                                                       [-LIM + 1, LIM - 3, LIM - 2, LIM - 1])],
                             True, 1024)
    c["equal_timestamps"] = (plain, [_one_key(count(90), [7] * 90), _one_key(count(90), [8] * 90)],
                             False, 1024)
    c["decreasing_timestamps"] = (plain, [_one_key(count(100), np.arange(100, 0, -1))], False,
                                  1024)
    c["key_at_cap_minus_1_then_growth"] = (
        plain, [(np.array([3, 3]), [1, 5], [0, 1]), (np.array([13, 3, 13]), [1, 9, 4], [2, 3, 4])],
        False, 4)
    keys = np.sort(rng.choice(9, 700, p=np.array([40, 20, 10, 10, 5, 5, 5, 3, 2]) / 100))
    rng.shuffle(keys[300:])      # runs of many lengths that cross the 64-row chunks
    c["runs_across_chunk_boundaries"] = (
        plain, [(keys, count(700), rng.integers(0, 40, 700)),
                (keys, count(700), rng.integers(20, 80, 700))], False, 1024)
    # the compaction's tile edges: every row kept, then no row kept (all stragglers), then no
    # row kept by the rule
    for n in (4095, 4096, 4097, 8193):
        ids = np.arange(n)
        for name, rule in (("", plain), ("_by_the_rule", dict(per_ms=1000, when=">",
                                                                threshold=INF))):
            c[f"{n}_rows_all_kept_then_none{name}"] = (
                rule, [(ids, np.zeros(n, np.int64), np.zeros(n, np.int64)),
                       (rng.permutation(ids), count(n), np.full(n, 10)),
                       (rng.permutation(ids), count(n), np.full(n, 5))], False, 1024)
    return c


HAND = _hand_cases()


def _hand(name, dev):
    rule, batches, is_float, capacity = HAND[name]
    op = KeyedRateOperator(rule["per_ms"], rule.get("when"), rule.get("threshold"),
                           rule.get("max_gap"), device=dev, capacity=capacity)
    model, rows = Model(**rule), []
    for keys, vals, ts in batches:
        vals = np.asarray(vals, dtype=np.float64 if is_float else np.int64)
        got = _rows(op.process(T(keys, dev), T(bits(vals, is_float), dev), T(ts, dev),
                               is_float=is_float))
        assert got == model.process(keys, vals, ts, is_float)
        rows.append(got)
    assert np.array_equal(op.state.cpu().numpy(), model.table_rows(op.cap, is_float))
    assert op.out_of_order == model.out_of_order
    return op, rows


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_built_batches(name):
    op, rows = _hand(name, "cpu")
    flat = [r for b in rows for r in b]
    if name == "one_row":
        assert flat == [(9, fbits(4000.0), 4, 1, 5)] and op.out_of_order == 1
    if name == "key_at_cap_minus_1_then_growth":
        assert op.cap == 16
    if name == "a_200_row_key_with_its_high_in_the_first_chunk":
        assert [r[3:] for r in rows[1]] == [(1, 5001)] and op.out_of_order >= 189
    if name == "a_state_row_newer_than_the_batch":
        assert rows[1] == [(2, fbits(5000.0), 5, 1, 11)] and len(rows[2]) == 2
    if name == "long_values_across_the_wrap":
        # a smaller reading is a reset, whatever its sign; MAX - (MIN + 5) wraps to -6
        assert [r[2] for r in flat] == [K.I64_MIN + 5, -6, K.I64_MIN, K.I64_MAX, 1, K.I64_MAX]
    if name == "minus_zero_inf_and_nan_counters":
        incs = [struct.unpack("<d", struct.pack("<q", r[2]))[0] for r in flat]
        assert str(incs) == str([NAN, 0.1, 0.0, -0.0, INF, NAN, NAN, NAN, -INF, INF, -0.0, 0.0])
    if name == "a_subnormal_rate":
        rate = struct.unpack("<d", struct.pack("<q", flat[0][1]))[0]
        assert 0.0 < rate < 2.2250738585072014e-308 and flat[0][3] == 2 * LIM - 4
    if name == "dt_near_2_62":
        assert [r[3] for r in flat] == [LIM - 1, LIM - 2, 1]
    if name == "dt_near_2_62_with_a_gap":
        assert [r[3] for r in flat] == [1, LIM - 5, 1]   # the first, LIM, is beyond the gap
    if name == "equal_timestamps":
        assert [r[3:] for r in flat] == [(1, 8)] and op.out_of_order == 89 + 89
    if name == "decreasing_timestamps":
        assert flat == [] and op.out_of_order == 99
    if name.endswith("_rows_all_kept_then_none"):
        n = int(name.split("_")[0])
        assert [len(b) for b in rows] == [0, n, 0] and op.out_of_order == n
    if name.endswith("_by_the_rule"):
        assert not flat


def test_exact_rows_of_a_small_example():
    op = KeyedRateOperator(1000)
    keys = [1, 2, 1, 1, 1, 2, 1]
    vals = [100, 7, 350, 999, 360, 3, 7]
    ts = [10, 10, 20, 15, 20, 30, 24]
    got = _rows(op.process(T(keys), T(vals), T(ts), is_float=False))
    assert got == [(1, fbits(25000.0), 250, 10, 20), (2, fbits(150.0), 3, 20, 30),
                   (1, fbits(1750.0), 7, 4, 24)]
    assert op.out_of_order == 2
    assert op.metrics.num_records_in == 7 and op.metrics.num_records_out == 3
    assert [a.tolist() for a in op.entries()] == [[1, 2], [24, 30], [7, 3]]
    with pytest.raises(TypeError, match="all longs or all doubles"):
        op.process(T([1]), T(bits([1.0], True)), T([99]), is_float=True)
    assert op.process(T([]), T([]), T([]), is_float=True) == []


# ---- refusals ---------------------------------------------------------------------------------
def test_unsupported_batches_and_parameters_are_refused():
    op = KeyedRateOperator(dense_limit=100)
    for keys, ts in (([100], [1]), ([-1], [1]), ([1], [LIM]), ([1], [-LIM]), ([1], [K.I64_MIN])):
        with pytest.raises(TypeError):
            op.process(T(keys), T([0]), T(ts), is_float=False)
    assert op.entries()[0].size == 0 and op.metrics.num_records_in == 0
    with pytest.raises(TypeError):
        op.process(T([1]).to(torch.int32), T([0]), T([1]))
    for bad in (dict(per_ms=0), dict(per_ms=True), dict(per_ms=1.0), dict(max_gap=0),
                dict(max_gap=LIM), dict(max_gap=2.0), dict(when="<"), dict(threshold=1.0),
                dict(when="=", threshold=1.0)):
        with pytest.raises(ValueError):
            KeyedRateOperator(**bad)
    with pytest.raises(TypeError):
        KeyedRateOperator(when="<", threshold="1")
    m = K.load()
    assert m.RATE_NONE == NONE
    st = K.rate_table(8, "cpu")
    kw = dict(kind=K.SUSTAIN_LONG, per_ms=1000, when=None, threshold_bits=0, max_gap=None)
    with pytest.raises(ValueError):
        K.rate_update(st, T([8]), T([0]), T([1]), **kw)                  # key out of range
    with pytest.raises(ValueError):
        K.rate_update(st, T([-1]), T([0]), T([1]), **kw)
    for t in (LIM, -LIM):
        with pytest.raises(TypeError):
            K.rate_update(st, T([1]), T([0]), T([t]), **kw)
    with pytest.raises(ValueError):
        K.rate_update(st, T([1]), T([0]), T([1, 2]), **kw)
    with pytest.raises(ValueError, match="aligned"):
        K.rate_update(st.view(-1)[1:15].view(7, 2), T([1]), T([0]), T([1]), **kw)
    for bad in (dict(kind=2), dict(per_ms=0), dict(per_ms=1.5), dict(per_ms=True),
                dict(max_gap=0), dict(max_gap=LIM), dict(when="=~"), dict(threshold_bits=1 << 64)):
        with pytest.raises(ValueError):
            K.rate_update(st, T([1]), T([0]), T([1]), **{**kw, **bad})
    # the native side checks the rule too, whoever calls it
    for args in ((2, 0, 0, 1, 0), (0, 7, 0, 1, 0), (0, 0, 0, 0, 0), (0, 0, 0, 1, -1),
                 (0, 0, 0, 1, LIM)):
        with pytest.raises(ValueError):
            m.cpu_rate_update(0, 0, 0, 0, *args, st.data_ptr(), 8, 0, 0, 0, 0, 0)
    assert np.array_equal(st.numpy(), Model().table_rows(8, False))
    assert K.rate_update(st, T([]), T([]), T([]), **kw)[1] == 0
    for cap in (0, -1):
        with pytest.raises(ValueError):
            K.rate_table(cap, "cpu")


def test_snapshot_rows_and_a_foreign_checkpoint():
    rule = dict(per_ms=1000, when="<", threshold=100.0, max_gap=50)
    op = KeyedRateOperator(**rule)
    op.process(T([1, 2, 2, 4, 4, 2]), T([5, 6, 7, 8, 9, 1]), T([5, 6, 20, 7, 8, 19]),
               is_float=False)
    op.advance_watermark(95)
    snap = op.snapshot_state()
    assert snap.meta["kind"] == "counter_rate" and snap.meta["per_ms"] == 1000
    assert snap.meta["when"] == "<" and snap.meta["threshold_bits"] == fbits(100.0)
    assert snap.meta["max_gap"] == 50 and snap.meta["out_of_order"] == 1
    assert snap.meta["value_kind"] == K.SUSTAIN_LONG
    assert snap.meta["wm"] == 95 and snap.meta["metrics"]["num_records_in"] == 6
    assert {k: v.tolist() for k, v in snap.columns.items()} == {
        "key": [1, 2, 4], "last_ts": [5, 20, 8], "last_value": [5, 7, 9]}
    for other in (dict(rule, per_ms=1), dict(rule, when="<="), dict(rule, threshold=101.0),
                  dict(rule, max_gap=None), dict(per_ms=1000)):
        with pytest.raises(ValueError, match="different counter-rate"):
            KeyedRateOperator(**other).restore_state(snap.columns, snap.meta)
    with pytest.raises(ValueError, match="different counter-rate"):
        KeyedRateOperator(**rule).restore_state(snap.columns, {"kind": "sustained"})
    # the same rule written with an int threshold is the same function
    fresh = KeyedRateOperator(**dict(rule, threshold=100), capacity=2)
    fresh.restore_state(snap.columns, snap.meta)
    assert fresh.wm == 95 and fresh.metrics.num_records_out == 1 and fresh.out_of_order == 1
    assert _rows(fresh.process(T([2, 1, 3, 4]), T([8, 9, 1, 10]), T([40, 5, 11, 9]),
                               is_float=False)) == [(2, fbits(50.0), 1, 20, 40)]
    assert fresh.out_of_order == 2
    with pytest.raises(TypeError, match="all longs or all doubles"):
        fresh.process(T([2]), T(bits([1.0], True)), T([50]), is_float=True)
    bad = dict(snap.columns, last_ts=np.array([5, NONE, 8]))
    with pytest.raises(ValueError, match="never seen"):
        KeyedRateOperator(**rule).restore_state(bad, snap.meta)
    with pytest.raises(ValueError, match="counter kind"):
        KeyedRateOperator(**rule).restore_state(snap.columns, dict(snap.meta, value_kind=5))


# ---- sanitizer --------------------------------------------------------------------------------
def test_sanitizer_harness_runs_clean():
    from mxstream.build import build_sanitize_rate

    res = subprocess.run([str(build_sanitize_rate())], capture_output=True, text=True,
                         timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.strip().splitlines()[-1] == "rate sanitize ok"


# ---- GPU --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("config,is_float,seed,nkeys", CASES)
def test_gpu_engine_equals_the_per_record_model_across_a_snapshot(gpu_device, config, is_float,
                                                                  seed, nkeys):
    op = _run_engine(config, is_float, seed, nkeys, dev=gpu_device)
    assert op.device.type == "cuda"


@pytest.mark.gpu
@pytest.mark.parametrize("config,is_float,seed,nkeys", CASES)
def test_gpu_kernels_equal_the_twin(gpu_device, config, is_float, seed, nkeys):
    tabs = {d: K.rate_table(nkeys, d) for d in ("cpu", gpu_device)}
    for c in _stream(seed, nkeys):
        if c[0] != "p":
            continue
        (a, ia), (b, ib) = (_update(tabs[d], c, config, is_float, d) for d in ("cpu", gpu_device))
        assert len(a) == len(b) == 5 and ia == ib
        assert all(torch.equal(x, y.cpu()) for x, y in zip(a, b))
        assert torch.equal(tabs["cpu"], tabs[gpu_device].cpu())


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(HAND))
def test_gpu_hand_built_batches(gpu_device, name):
    _, rows = _hand(name, gpu_device)
    assert rows == _hand(name, "cpu")[1]
