"""Burst alerts (csrc/mxs_burst.h): the C++ twin and the engine operator
(runtime/burst_operator.py) against a per-record model of BurstAlert (a dict per key), and the
gfx950 kernel against the twin array for array. Everything is an integer or a bit pattern and
compares exactly, row for row and in order; a ring is compared oldest first, which does not
depend on its rotation."""
from __future__ import annotations

import functools
import subprocess

import numpy as np
import pytest
import torch

from mxstream.api import functions as F
from mxstream.ops import kernels as K
from mxstream.runtime.burst_operator import KeyedBurstOperator, unpack
from mxstream.runtime.sustain_operator import threshold_bits

KEY_SPACES = [1, 7, 300, 4095, 4096, 4097, 8193]
RULES = [(2, 0), (2, 40), (3, 120), (5, 400)]   # (times, within)
SEEDS = [0, 1]
NAN = float("nan")


def T(a, dev="cpu") -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev)


def bits(vals, is_float=True) -> np.ndarray:
    """The value column as the engine takes it: doubles' bit patterns, or the longs."""
    if is_float:
        return np.ascontiguousarray(vals, dtype=np.float64).view(np.int64)
    return np.ascontiguousarray(vals, dtype=np.int64)


class Model:
    """BurstAlert record by record: key -> [recent, since, firing], and per entry of `recent`
    the batch it came in."""

    def __init__(self, when, threshold, times, within):
        self.cmp = F._LOOKUP_WHENS[when]
        self.thr, self.times, self.within = float(threshold), times, within
        self.state, self.batch = {}, 0
        self.spread = 0  # code-1 rows whose `times` breaches came in at least two batches

    def process(self, keys, vals, ts, is_float=True) -> list:
        """Rows (key, code, since, value bits, ts) in arrival order."""
        out = []
        vb = bits(vals, is_float).tolist()
        for k, v, b, t in zip(np.asarray(keys).tolist(), np.asarray(vals).tolist(), vb,
                              np.asarray(ts).tolist()):
            breach = self.cmp(float(v), self.thr)
            if not breach and k not in self.state:
                continue
            s = self.state.setdefault(k, [[], 0, False])
            if breach:
                s[0] = (s[0] + [(t, self.batch)])[-self.times:]
            dense = len(s[0]) == self.times and t - s[0][0][0] <= self.within
            if breach and dense and not s[2]:
                s[1], s[2] = s[0][0][0], True
                out.append((k, 1, s[1], b, t))
                self.spread += s[0][0][1] < self.batch
            elif not dense and s[2]:
                out.append((k, 0, s[1], b, t))
                s[1], s[2] = 0, False
        self.batch += 1
        return out

    def table(self, cap: int):
        """(since, firing, held, recent oldest first) as unpack() gives them."""
        since, firing, held = (np.zeros(cap, dtype=np.int64) for _ in range(3))
        recent = np.zeros((cap, self.times), dtype=np.int64)
        for k, (rec, s, f) in self.state.items():
            since[k], firing[k], held[k] = s, int(f), len(rec)
            recent[k, :len(rec)] = [t for t, _ in rec]
        return since, firing, held, recent


def _same_state(got, want) -> bool:
    return all(np.array_equal(a, b) for a, b in zip(got, want))


@functools.lru_cache(maxsize=None)
def _stream(seed: int, nkeys: int, steps: int = 24):
    """The sustained-alert tests' call generator -- ("p", keys, ts, vals) and ("w", wm) calls: 0
    to 399 rows per step, +-30 ms of disorder, late elements, equal timestamps for one key, empty
    batches and a key range that grows with the steps -- with a value column
    round(base[key] + N(0, 8), 1), base ~ U(40, 100) per key."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(40, 100, nkeys)
    calls, now, wm = [], 1_000, 0
    for s in range(steps):
        hi = max(1, min(nkeys, 1 + nkeys * (s + 2) // 12))
        n = 0 if s % 7 == 3 else int(rng.integers(1, 400))
        keys = rng.integers(0, hi, n).astype(np.int64)
        ts = now + rng.integers(-30, 30, n)
        late = rng.random(n) < 0.1
        ts = np.where(late, ts - 500, ts).astype(np.int64)
        if n > 2:
            ts[1] = ts[0]
            keys[1] = keys[0]
        vals = np.round(base[keys] + rng.normal(0, 8, n), 1)
        calls.append(("p", keys, ts, vals))
        if s % 5 == 4:
            calls.append(("p", np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0)))
        if rng.random() < 0.7:
            wm = max(wm, now - int(rng.integers(0, 80)))
            calls.append(("w", wm))
            if rng.random() < 0.4:
                calls.append(("w", wm))
            if rng.random() < 0.2:
                calls.append(("w", wm - 50))
        now += int(rng.integers(5, 60))
    return calls


@functools.lru_cache(maxsize=None)
def _expected(seed: int, nkeys: int, times: int, within: int):
    """The model over a stream, computed once: every "p" call's rows, the final state, and the
    number of code-1 rows whose breaches came in at least two batches."""
    model = Model(">", 70.0, times, within)
    rows = [model.process(c[1], c[3], c[2]) for c in _stream(seed, nkeys) if c[0] == "p"]
    return rows, model.table(nkeys), model.spread


CASES = [(s, k, t, w) for s in SEEDS for k in KEY_SPACES for t, w in RULES]


def _rows(chunks) -> list:
    out = []
    for cols in chunks:
        out.extend(zip(*(c.cpu().tolist() for c in cols)))
    return out


# ---- the streams hold what they are meant to test ---------------------------------------------
@pytest.mark.parametrize("nkeys", KEY_SPACES)
@pytest.mark.parametrize("times,within", RULES)
def test_streams_hold_fires_resolves_and_bursts_across_batches(nkeys, times, within):
    asserted = nkeys <= 300 or (times, within) in ((2, 40), (3, 120))
    spread = 0
    for seed in SEEDS:
        rows, _, s = _expected(seed, nkeys, times, within)
        flat = [r for b in rows for r in b]
        if asserted:
            assert sum(r[1] == 1 for r in flat) >= 1 and sum(r[1] == 0 for r in flat) >= 1
        spread += s
        assert sum(c[0] == "p" and len(c[1]) == 0 for c in _stream(seed, nkeys)) >= 1
    if asserted:
        assert spread >= 1   # some fire comes from breaches spread over two batches at least


# ---- the twin and the engine against the per-record model -------------------------------------
def _update(state, call, within, dev="cpu"):
    return K.burst_update(state[0], state[1], T(call[1], dev), T(bits(call[3]), dev),
                          T(call[2], dev), kind=K.SUSTAIN_DOUBLE, when=">",
                          threshold_bits=threshold_bits(70.0), within=within)


@pytest.mark.parametrize("seed,nkeys,times,within", CASES)
def test_twin_equals_the_per_record_model(seed, nkeys, times, within):
    want, table, _ = _expected(seed, nkeys, times, within)
    state = K.burst_table(nkeys, times, "cpu")
    got = [_rows([_update(state, c, within)]) for c in _stream(seed, nkeys) if c[0] == "p"]
    assert got == want
    assert _same_state(unpack(*state), table)


def _run_engine(seed, nkeys, times, within, dev="cpu", snapshot=True):
    calls = _stream(seed, nkeys)
    make = lambda: KeyedBurstOperator(">", 70.0, times, within, device=dev)  # noqa: E731
    op, got = make(), []
    for i, c in enumerate(calls):
        if snapshot and i == len(calls) // 2:
            snap = op.snapshot_state()
            assert snap.meta["kind"] == "burst" and snap.meta["times"] == times
            assert snap.meta["within_ms"] == within
            assert set(snap.columns) == {"key", "since", "firing", "held"} | {
                f"r{j}" for j in range(times)}
            op = make()
            op.restore_state(snap.columns, snap.meta)
        if c[0] == "w":
            assert op.advance_watermark(c[1]) == []
            continue
        chunks = op.process(T(c[1], dev), T(bits(c[3]), dev), T(c[2], dev))
        assert len(chunks) <= 1 and all(len(cols) == 5 for cols in chunks)
        got.append(_rows(chunks))
    want, table, _ = _expected(seed, nkeys, times, within)
    assert got == want
    # the capacity covers the largest key seen, not nkeys
    full = Model(">", 70.0, times, within).table(max(op.cap, nkeys))
    for f, t in zip(full, table):
        f[:nkeys] = t
    state = unpack(op.ring, op.row)
    assert _same_state(state, [f[:op.cap] for f in full]) and not full[2][op.cap:].any()
    ids, since, firing, held, recent = op.entries()
    assert ids.tolist() == np.nonzero(table[2])[0].tolist()
    assert np.array_equal(recent, table[3][ids]) and np.array_equal(firing, table[1][ids])
    return op


@pytest.mark.parametrize("seed,nkeys,times,within", CASES)
def test_engine_equals_the_per_record_model_across_a_snapshot(seed, nkeys, times, within):
    op = _run_engine(seed, nkeys, times, within)
    if nkeys > 4096:
        assert KeyedBurstOperator(">", 70.0, times, within).cap < 4096 <= op.cap  # it grew


# ---- hand-built batches: the smallest shapes where the look-back and the scan can go wrong ----
B, Q = 80.0, 10.0   # a breaching and a quiet value under "> 70"


def _one_key(vals, ts=None, key=0):
    n = len(vals)
    return (np.full(n, key), vals, np.arange(n) if ts is None else ts)


def _at(n, breaches, quiet=Q):
    vals = [quiet] * n
    for p in breaches:
        vals[p] = B
    return vals


def _hand_cases():
    """name -> (rule (when, threshold, times, within), [batches (keys, vals, ts)], is_float,
    capacity)."""
    c = {}
    # one key, 130 rows: the look-back of the breaches at rows 64.. and 128.. reaches over the
    # chunk ends at rows 63 / 64 and 127 / 128
    for times in (2, 3, 16):
        near = [63 - 2 * j for j in range(times - 1)][::-1] + [64, 66] \
            + [127 - 2 * j for j in range(times - 1)][::-1] + [128, 129]
        c[f"straddle_130_times_{times}"] = (
            (">", 70.0, times, 2 * times), [_one_key(_at(130, near))], True, 1024)
        c[f"straddle_130_all_breach_times_{times}"] = (
            (">", 70.0, times, times - 1), [_one_key([B] * 130)], True, 1024)
        c[f"straddle_130_all_breach_one_short_times_{times}"] = (
            (">", 70.0, times, times - 2), [_one_key([B] * 130)], True, 1024)
        c[f"straddle_130_stored_ring_times_{times}"] = (
            (">", 70.0, times, 70), [_one_key([B] * (times - 1), np.arange(times - 1) - 50),
                                      _one_key(_at(130, [0, 62, 63, 64, 100, 127, 128]))],
            True, 1024)
    # a 64-row run that ends exactly at a chunk end, behind a 64-row run of another key
    keys = np.repeat([4, 9], 64)
    c["64_row_runs_end_at_chunk_ends"] = (
        (">", 70.0, 3, 4), [(keys, _at(128, [1, 2, 3, 60, 62, 63, 64, 65, 66, 120, 126, 127]),
                             np.arange(128))] * 2, True, 1024)
    c["64_row_run_walked_to_a_chunk_end"] = (
        (">", 70.0, 3, 4), [(np.repeat([4, 9], [10, 118]), _at(128, [70, 72, 73, 125, 126, 127]),
                             np.arange(128)), _one_key([B, Q], [128, 140], key=9)], True, 1024)
    # two short runs sharing a wave; the second one's look-back reads the stored ring
    c["two_short_runs_second_reads_the_ring"] = (
        (">", 70.0, 3, 10), [(np.array([7, 7]), [B, B], [1, 2]),
                             (np.array([5, 7, 5, 7, 5]), [B, B, B, Q, B], [3, 4, 5, 6, 7]),
                             (np.array([5, 7]), [Q, Q], [30, 30])], True, 1024)
    # the ring wraps: more than `times` breaches over four batches
    c["ring_wraps_over_four_batches"] = (
        (">", 70.0, 3, 25), [_one_key([B, B], [0, 10]), _one_key([B, Q, B], [20, 21, 50]),
                             _one_key([B, B, B, B], [60, 61, 62, 63]),
                             _one_key([Q, B, Q], [64, 200, 201])], True, 1024)
    c["resolve_by_a_quiet_element_in_a_later_batch"] = (
        (">", 70.0, 2, 10), [_one_key([B, B], [0, 5]), _one_key([Q], [9]), _one_key([Q], [11]),
                             _one_key([Q], [12])], True, 1024)
    c["a_breach_that_resolves"] = (
        (">", 70.0, 2, 10), [_one_key([B, B, B, B], [0, 5, 30, 32])], True, 1024)
    c["within_0_equal_timestamps"] = (
        (">", 70.0, 2, 0), [_one_key([B, B, Q, B, B, B], [7, 7, 7, 8, 9, 9])], True, 1024)
    c["within_0_equal_timestamps_long_run"] = (
        (">", 70.0, 16, 0), [_one_key([B] * 70 + [Q, B], [7] * 70 + [8, 8])], True, 1024)
    c["disorder_breach_below_recent_0"] = (
        (">", 70.0, 2, 5), [_one_key([B, B, B, Q, B], [100, 40, 200, 20, 30])], True, 1024)
    c["times_16_fire_and_resolve"] = (
        (">", 70.0, 16, 100), [_one_key([B] * 10, np.arange(10) * 5),
                               _one_key([B] * 6 + [Q, Q], list(50 + np.arange(6) * 5) + [90, 180])],
        True, 1024)
    c["empty"] = ((">", 70.0, 2, 0), [_one_key([]), _one_key([B]), _one_key([])], True, 1024)
    c["one_row"] = ((">", 70.0, 2, 9), [_one_key([B], [4], key=9), _one_key([B], [5], key=9),
                                        _one_key([Q], [50], key=9)], True, 1024)
    k64 = np.arange(64)[::-1].copy()
    c["64_keys_of_one_row"] = (
        (">", 70.0, 2, 4), [(k64, [B] * 64, np.zeros(64)), (k64, [B, Q] * 32, np.full(64, 4)),
                            (k64, [Q] * 64, np.full(64, 9))], True, 1024)
    for when in (">", ">=", "<", "<=", "==", "!="):
        c[f"nan_values_{when}"] = ((when, 70.0, 2, 3), [_one_key([NAN, B, NAN, 70.0, NAN, NAN, Q,
                                                                  Q, Q, Q])], True, 1024)
        c[f"nan_threshold_{when}"] = ((when, NAN, 2, 1), [_one_key([NAN, B, B, 70.0])], True, 1024)
    big = 1 << 53
    c["int_column"] = ((">", 70, 2, 1), [_one_key([80, 90, 70, 71, 72, 3, 3])], False, 1024)
    c["int_column_beyond_2_53"] = (  # float(2**53 + 1) == 2.0**53: no breach, as the doubles say
        (">", float(big), 2, 2), [_one_key([big + 1, big + 2, big + 1, K.I64_MAX, K.I64_MIN, 0])],
        False, 1024)
    c["two_capacity_doublings"] = (
        (">", 70.0, 2, 5), [(np.array([3, 3]), [B, B], [0, 1]),
                            (np.array([13, 3, 13]), [B, Q, B], [2, 30, 4])], True, 4)
    rng = np.random.default_rng(11)   # runs of many lengths that cross the 64-row chunks
    keys = np.sort(rng.choice(9, 700, p=np.array([40, 20, 10, 10, 5, 5, 5, 3, 2]) / 100))
    rng.shuffle(keys[300:])
    for times, p in ((2, 0.3), (5, 0.5), (16, 0.8)):
        c[f"runs_across_chunk_boundaries_times_{times}"] = (
            (">", 70.0, times, 12),
            [(keys, np.where(rng.random(700) < p, B, Q), np.sort(rng.integers(0, 400, 700)))] * 2,
            True, 1024)
    return c


HAND = _hand_cases()


def _hand(name, dev):
    (when, thr, times, within), batches, is_float, capacity = HAND[name]
    op = KeyedBurstOperator(when, thr, times, within, device=dev, capacity=capacity)
    model, fires, resolves = Model(when, thr, times, within), 0, 0
    for keys, vals, ts in batches:
        vals = np.asarray(vals, dtype=np.float64 if is_float else np.int64)
        got = _rows(op.process(T(keys, dev), T(bits(vals, is_float), dev), T(ts, dev),
                               is_float=is_float))
        assert got == model.process(keys, vals, ts, is_float)
        fires += sum(r[1] == 1 for r in got)
        resolves += sum(r[1] == 0 for r in got)
    assert _same_state(unpack(op.ring, op.row), model.table(op.cap))
    return op, fires, resolves


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_built_batches(name):
    op, fires, resolves = _hand(name, "cpu")
    if name == "two_capacity_doublings":
        assert op.cap == 16
    if name.startswith("straddle_130_times_"):
        assert (fires, resolves) == (2, 1)   # a burst around each chunk end; the last stays open
    if name.startswith("straddle_130_all_breach_times_"):
        assert (fires, resolves) == (1, 0)
    if name.startswith("straddle_130_all_breach_one_short"):
        assert (fires, resolves) == (0, 0)
    if name.startswith("straddle_130_stored_ring"):
        assert fires >= 1 and resolves >= 1
    if name in ("64_row_runs_end_at_chunk_ends", "64_row_run_walked_to_a_chunk_end",
                "two_short_runs_second_reads_the_ring", "ring_wraps_over_four_batches",
                "within_0_equal_timestamps", "within_0_equal_timestamps_long_run",
                "disorder_breach_below_recent_0", "times_16_fire_and_resolve", "int_column",
                "64_keys_of_one_row", "one_row"):
        assert fires >= 1 and resolves >= 1
    if name == "resolve_by_a_quiet_element_in_a_later_batch":
        assert (fires, resolves) == (1, 1)
    if name == "a_breach_that_resolves":
        assert (fires, resolves) == (2, 1)
    if name == "nan_values_!=":
        assert fires == 1
    if name in ("nan_threshold_>", "nan_values_==", "empty"):
        assert fires == 0
    if name == "int_column_beyond_2_53":
        assert (fires, resolves) == (1, 1)  # 2**53 + 2 and INT64_MAX breach, 2**53 + 1 does not


def test_exact_rows_of_a_small_example():
    op = KeyedBurstOperator(">=", 500, 3, 100)
    keys = [1, 2, 1, 1, 2, 1, 1, 1]
    vals = [500, 503, 200, 502, 500, 500, 200, 200]
    ts = [0, 10, 20, 30, 40, 90, 100, 131]
    got = _rows(op.process(T(keys), T(vals), T(ts), is_float=False))
    assert got == [(1, 1, 0, 500, 90), (1, 0, 0, 200, 131)]
    assert op.metrics.num_records_in == 8 and op.metrics.num_records_out == 2
    ids, since, firing, held, recent = op.entries()
    assert (ids.tolist(), firing.tolist(), held.tolist()) == ([1, 2], [0, 0], [3, 2])
    assert recent.tolist() == [[0, 30, 90], [10, 40, 0]]


# ---- refusals ---------------------------------------------------------------------------------
def test_unsupported_batches_and_parameters_are_refused():
    op = KeyedBurstOperator(">", 70.0, 2, 10, dense_limit=100)
    lim = K.SUSTAIN_TS_LIMIT
    for keys, ts in (([100], [1]), ([-1], [1]), ([1], [lim]), ([1], [-lim]), ([1], [K.I64_MIN])):
        with pytest.raises(TypeError):
            op.process(T(keys), T(bits([B])), T(ts))
    assert op.entries()[0].size == 0 and op.metrics.num_records_in == 0
    assert _rows(op.process(T([99, 99]), T(bits([B, B])), T([lim - 1, -lim + 1]))) == \
        [(99, 1, lim - 1, int(bits([B])[0]), -lim + 1)]
    with pytest.raises(TypeError):
        op.process(T([1]).to(torch.int32), T(bits([B])), T([1]))
    for bad in (1, 0, -1, 17, True, 2.0, None):
        with pytest.raises(ValueError):
            KeyedBurstOperator(">", 70.0, bad, 10)
    for bad in (-1, True, 1.5, None, lim):
        with pytest.raises(ValueError):
            KeyedBurstOperator(">", 70.0, 2, bad)
    for bad in (None, "=>", 3):
        with pytest.raises(ValueError):
            KeyedBurstOperator(bad, 70.0, 2, 1)
    for bad in (True, "70", None):
        with pytest.raises(TypeError):
            KeyedBurstOperator(">", bad, 2, 1)
    m = K.load()
    assert (m.BURST_MAX_TIMES, m.BURST_HELD_SHIFT, m.BURST_POS_SHIFT) == \
        (K.BURST_MAX_TIMES, K.BURST_HELD_SHIFT, K.BURST_POS_SHIFT)
    for bad in (1, 17, True):
        with pytest.raises(ValueError):
            K.burst_table(8, bad, "cpu")
    ring, row = K.burst_table(8, 2, "cpu")
    kw = dict(kind=K.SUSTAIN_DOUBLE, when=">", threshold_bits=0, within=1)
    with pytest.raises(ValueError):
        K.burst_update(ring, row, T([8]), T([0]), T([1]), **kw)
    with pytest.raises(TypeError):
        K.burst_update(ring, row, T([1]), T([0]), T([lim]), **kw)
    with pytest.raises(ValueError):
        K.burst_update(ring, row, T([1]), T([0]), T([1, 2]), **kw)
    with pytest.raises(ValueError):
        K.burst_update(ring, row.view(-1)[1:15].view(7, 2), T([1]), T([0]), T([1]), **kw)
    with pytest.raises(ValueError):   # a ring of another capacity
        K.burst_update(ring[:7], row, T([1]), T([0]), T([1]), **kw)
    for bad in (dict(when=None), dict(within=-1), dict(within=lim), dict(kind=2)):
        with pytest.raises(ValueError):
            K.burst_update(ring, row, T([1]), T([0]), T([1]), **{**kw, **bad})
    assert not ring.any() and not row.any()


def test_snapshot_rows_and_a_foreign_checkpoint():
    op = KeyedBurstOperator(">", 70.0, 3, 50)
    op.process(T([1, 2, 2, 2, 2, 4, 4]), T(bits([B, B, B, B, B, B, Q])),
               T([5, 6, 20, 21, 22, 7, 8]))
    op.advance_watermark(95)
    snap = op.snapshot_state()
    assert snap.meta["kind"] == "burst" and snap.meta["when"] == ">"
    assert snap.meta["wm"] == 95 and snap.meta["metrics"]["num_records_in"] == 7
    # key 2's ring has wrapped: its rows are oldest first all the same
    assert {k: v.tolist() for k, v in snap.columns.items()} == {
        "key": [1, 2, 4], "since": [0, 6, 0], "firing": [0, 1, 0], "held": [1, 3, 1],
        "r0": [5, 20, 7], "r1": [0, 21, 0], "r2": [0, 22, 0]}
    for other in ((">", 70.0, 3, 51), (">=", 70.0, 3, 50), (">", 71.0, 3, 50), (">", 70.0, 4, 50)):
        with pytest.raises(ValueError, match="different burst"):
            KeyedBurstOperator(*other).restore_state(snap.columns, snap.meta)
    with pytest.raises(ValueError, match="different burst"):
        KeyedBurstOperator(">", 70.0, 3, 50).restore_state(snap.columns, {"kind": "sustained"})
    fresh = KeyedBurstOperator(">", 70.0, 3, 50, capacity=2)
    fresh.restore_state(snap.columns, snap.meta)
    assert fresh.wm == 95 and fresh.metrics.num_records_out == 1
    assert _same_state(unpack(fresh.ring, fresh.row)[:4], [x[:8] for x in unpack(op.ring, op.row)])
    assert _rows(fresh.process(T([2, 1, 1]), T(bits([Q, B, B])), T([71, 10, 11]))) == [
        (2, 0, 6, int(bits([Q])[0]), 71), (1, 1, 5, int(bits([B])[0]), 11)]


# ---- sanitizer --------------------------------------------------------------------------------
def test_sanitizer_harness_runs_clean():
    from mxstream.build import build_sanitize_burst

    res = subprocess.run([str(build_sanitize_burst())], capture_output=True, text=True,
                         timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.strip().splitlines()[-1] == "burst sanitize ok"


# ---- GPU --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("seed,nkeys,times,within", CASES)
def test_gpu_engine_equals_the_per_record_model_across_a_snapshot(gpu_device, seed, nkeys, times,
                                                                  within):
    op = _run_engine(seed, nkeys, times, within, dev=gpu_device)
    assert op.device.type == "cuda"


@pytest.mark.gpu
@pytest.mark.parametrize("seed,nkeys,times,within", CASES)
def test_gpu_kernels_equal_the_twin(gpu_device, seed, nkeys, times, within):
    tabs = {d: K.burst_table(nkeys, times, d) for d in ("cpu", gpu_device)}
    for c in _stream(seed, nkeys):
        if c[0] != "p":
            continue
        a, b = (_update(tabs[d], c, within, d) for d in ("cpu", gpu_device))
        assert len(a) == len(b) == 5
        assert all(torch.equal(x, y.cpu()) for x, y in zip(a, b))
        assert torch.equal(tabs["cpu"][1], tabs[gpu_device][1].cpu())      # row, bit for bit
        assert _same_state(unpack(*tabs["cpu"]), unpack(*tabs[gpu_device]))  # ring, oldest first


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(HAND))
def test_gpu_hand_built_batches(gpu_device, name):
    _, fires, resolves = _hand(name, gpu_device)
    assert (fires, resolves) == _hand(name, "cpu")[1:]
