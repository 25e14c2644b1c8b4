"""Keyed state machines (csrc/mxs_fsm.h): the C++ twin and the engine operator
(runtime/fsm_operator.py) against a per-record model of StateMachineAlert (a dict per key), and
the gfx950 kernels against the twin array for array. Everything is an integer or a bit pattern
and compares exactly, row for row and in order."""
from __future__ import annotations

import functools
import subprocess

import numpy as np
import pytest
import torch

from mxstream.ops import kernels as K
from mxstream.runtime.fsm_operator import KeyedStateMachineOperator

NONE = K.FSM_NONE
KEY_SPACES = [1, 7, 300, 4095, 4096, 4097, 8193]
SEEDS = [0, 1]
NAN, INF = float("nan"), float("inf")

# name -> (bounds, table, initial, report)
MACHINES = {
    # on at 90, off only below 80
    "hyst": ([80.0, 90.0], [[0, 0, 1], [0, 1, 1]], 0, "change"),
    # severity = class
    "sev": ([70.0, 85.0], [[0, 1, 2]] * 3, 0, "change"),
    # three breaches in a row; the two columns do not commute
    "consec": ([70.0], [[0, min(s + 1, 3)] for s in range(4)], 0, [(2, 3)]),
    # state 15 and the top nibble; a self-loop is reported
    "cycle16": ([70.0], [[s, (s + 1) % 16] for s in range(16)], 0, [(15, 0), (0, 0)]),
    "wide": ([43.75 + 3.75 * j for j in range(15)],
             np.random.default_rng(5).integers(0, 5, (5, 16)).tolist(), 2, "change"),
    "mute": ([70.0, 85.0], [[0, 1, 2]] * 3, 0, ()),
}


def T(a, dev="cpu") -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev)


def bits(vals, is_float=True) -> np.ndarray:
    """The value column as the engine takes it: doubles' bit patterns, or the longs."""
    if is_float:
        return np.ascontiguousarray(vals, dtype=np.float64).view(np.int64)
    return np.ascontiguousarray(vals, dtype=np.int64)


def _pairs(table, report) -> set:
    n = len(table)
    if isinstance(report, str):
        return {(a, b) for a in range(n) for b in range(n) if a != b}
    return {tuple(p) for p in report}


class Model:
    """StateMachineAlert record by record: key -> (since, state, the batch that set since)."""

    def __init__(self, bounds, table, initial=0, report="change"):
        self.bounds, self.table, self.initial = [float(b) for b in bounds], table, initial
        self.report = _pairs(table, report)
        self.state, self.batch = {}, 0
        self.carried = 0        # rows whose since stems from an earlier batch
        self.seen_states, self.seen_pairs = set(), set()

    def process(self, keys, vals, ts, is_float=True) -> list:
        """Rows (key, from << 4 | to, since, value bits, ts) in arrival order."""
        out = []
        vb = bits(vals, is_float).tolist()
        for k, v, b, t in zip(np.asarray(keys).tolist(), np.asarray(vals).tolist(), vb,
                              np.asarray(ts).tolist()):
            since, st, born = self.state.get(k) or (t, self.initial, self.batch)
            x = float(v)
            to = self.table[st][sum(x >= c for c in self.bounds)]
            self.seen_states.update((st, to))
            if (st, to) in self.report:
                out.append((k, st << 4 | to, since, b, t))
                self.carried += born < self.batch
                self.seen_pairs.add((st, to))
            if to != st:
                since, born = t, self.batch
            self.state[k] = (since, to, born)
        self.batch += 1
        return out

    def table_rows(self, cap: int) -> np.ndarray:
        st = np.zeros((cap, 2), dtype=np.int64)
        st[:, 0] = NONE
        for k, (since, state, _) in self.state.items():
            st[k] = (since, state)
        return st


@functools.lru_cache(maxsize=None)
def _stream(seed: int, nkeys: int, steps: int = 24):
    """The sustained-alert tests' call generator -- ("p", keys, ts, vals) and ("w", wm) calls: 0
    to 399 rows per step, +-30 ms of disorder, late elements, equal timestamps for one key,
    empty batches and a key range that grows with the steps -- with a quarter of the rows on key
    0, so that one key walks far through its machine whatever the key space, and a value column
    round(U(35, 105), 1) that reaches every class of every machine."""
    rng = np.random.default_rng(seed)
    calls, now, wm = [], 1_000, 0
    for s in range(steps):
        hi = max(1, min(nkeys, 1 + nkeys * (s + 2) // 12))
        n = 0 if s % 7 == 3 else int(rng.integers(1, 400))
        keys = rng.integers(0, hi, n).astype(np.int64)
        keys[rng.random(n) < 0.25] = 0
        ts = now + rng.integers(-30, 30, n)
        late = rng.random(n) < 0.1
        ts = np.where(late, ts - 500, ts).astype(np.int64)
        if n > 2:
            ts[1] = ts[0]
            keys[1] = keys[0]
        vals = np.round(rng.uniform(35, 105, n), 1)
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
def _expected(name: str, seed: int, nkeys: int):
    """The model over a stream, computed once: every "p" call's rows, the final table, and the
    model itself for what it has seen."""
    model = Model(*MACHINES[name])
    rows = [model.process(c[1], c[3], c[2]) for c in _stream(seed, nkeys) if c[0] == "p"]
    return rows, model.table_rows(nkeys), model


CASES = [(m, s, k) for m in MACHINES for s in SEEDS for k in KEY_SPACES]


def _rows(chunks) -> list:
    out = []
    for cols in chunks:
        out.extend(zip(*(c.cpu().tolist() for c in cols)))
    return out


# ---- the streams hold what they are meant to test ---------------------------------------------
@pytest.mark.parametrize("nkeys", KEY_SPACES)
@pytest.mark.parametrize("name", sorted(MACHINES))
def test_streams_hold_what_they_test(name, nkeys):
    bounds, table, initial, report = MACHINES[name]
    for seed in SEEDS:
        rows, _, model = _expected(name, seed, nkeys)
        assert model.seen_states == set(range(len(table)))
        if name == "mute":
            assert not any(rows)
        else:
            # every reported pair the table holds occurs
            held = {(s, to) for s, row in enumerate(table) for to in row}
            assert model.seen_pairs == _pairs(table, report) & held and model.seen_pairs
            assert model.carried >= 1
        calls = _stream(seed, nkeys)
        if nkeys <= 7:
            assert max(np.bincount(c[1]).max() for c in calls if c[0] == "p" and len(c[1])) > 64
        assert sum(c[0] == "p" and len(c[1]) == 0 for c in calls) >= 1


# ---- the twin and the engine against the per-record model -------------------------------------
def _packed(name):
    bounds, table, initial, report = MACHINES[name]
    cuts, cols, masks = K.fsm_pack(bounds, table, sorted(_pairs(table, report)))
    return dict(cuts=cuts, cols=cols, report=masks, states=len(masks), classes=len(cols),
                initial=initial)


def _update(state, call, name, dev="cpu"):
    return K.fsm_update(state, T(call[1], dev), T(bits(call[3]), dev), T(call[2], dev),
                        kind=K.SUSTAIN_DOUBLE, **_packed(name))


@pytest.mark.parametrize("name,seed,nkeys", CASES)
def test_twin_equals_the_per_record_model(name, seed, nkeys):
    want, table, _ = _expected(name, seed, nkeys)
    state = K.fsm_table(nkeys, "cpu")
    got = [_rows([_update(state, c, name)]) for c in _stream(seed, nkeys) if c[0] == "p"]
    assert got == want
    assert np.array_equal(state.numpy(), table)


def _run_engine(name, seed, nkeys, dev="cpu"):
    calls = _stream(seed, nkeys)
    make = lambda **kw: KeyedStateMachineOperator(*MACHINES[name], device=dev, **kw)  # noqa: E731
    op, got = make(), []
    for i, c in enumerate(calls):
        if i == len(calls) // 2:
            snap = op.snapshot_state()
            assert snap.meta["kind"] == "state_machine"
            assert snap.meta["initial"] == MACHINES[name][2]
            assert sorted(snap.columns) == ["key", "since", "state"]
            op = make(capacity=2)   # a smaller table: the restore grows it
            op.restore_state(snap.columns, snap.meta)
        if c[0] == "w":
            assert op.advance_watermark(c[1]) == []
            continue
        chunks = op.process(T(c[1], dev), T(bits(c[3]), dev), T(c[2], dev))
        assert len(chunks) <= 1 and all(len(cols) == 5 for cols in chunks)
        got.append(_rows(chunks))
    want, table, _ = _expected(name, seed, nkeys)
    assert got == want
    st = op.state.cpu().numpy()     # the capacity covers the largest key seen, not nkeys
    full = Model(*MACHINES[name]).table_rows(max(op.cap, nkeys))
    full[:nkeys] = table
    assert np.array_equal(st, full[:op.cap]) and (full[op.cap:, 0] == NONE).all()
    ids, since, state = op.entries()
    seen = np.nonzero(table[:, 0] != NONE)[0]
    assert ids.tolist() == seen.tolist()
    assert since.tolist() == table[seen, 0].tolist() and state.tolist() == table[seen, 1].tolist()
    return op


@pytest.mark.parametrize("name,seed,nkeys", CASES)
def test_engine_equals_the_per_record_model_across_a_snapshot(name, seed, nkeys):
    op = _run_engine(name, seed, nkeys)
    if nkeys > 4096:
        assert op.cap >= 4096  # it grew from 2


# ---- hand-built batches: the smallest shapes where the scan can go wrong ----------------------
B, Q = 95.0, 10.0   # the highest and the lowest class of every machine here


def _one_key(vals, ts=None, key=0):
    n = len(vals)
    return (np.full(n, key), vals, np.arange(n) if ts is None else ts)


def _hand_cases():
    """name -> (machine (bounds, table, initial, report), [batches (keys, vals, ts)], is_float,
    capacity)."""
    c = {}
    rng = np.random.default_rng(3)
    c["one_row"] = (MACHINES["sev"], [_one_key([B], [4], key=9), _one_key([Q], [5], key=9)],
                    True, 1024)
    c["empty"] = (MACHINES["sev"], [_one_key([]), _one_key([B]), _one_key([])], True, 1024)
    for L in (63, 64, 65, 128, 129):
        for m in ("hyst", "consec", "cycle16", "wide"):
            # the walk and its carry: a second batch goes on from the first one's state
            c[f"run_{L}_{m}"] = (MACHINES[m], [_one_key(np.round(rng.uniform(35, 105, L), 1)),
                                               _one_key(np.round(rng.uniform(35, 105, L), 1),
                                                        np.arange(L) + 1000)], True, 1024)
        c[f"run_{L}_every_row_steps"] = (MACHINES["cycle16"], [_one_key([B] * L)] * 2, True, 1024)
    # key 1's run begins at sorted row 63 of the first chunk; the arrival order interleaves
    keys = np.array([0] * 63 + [1] * 70 + [2] * 3)
    order = rng.permutation(keys.size)
    for m in ("consec", "cycle16"):
        c[f"run_begins_at_row_63_{m}"] = (
            MACHINES[m], [(keys[order], np.where(rng.random(keys.size) < 0.7, B, Q),
                           rng.integers(0, 50, keys.size))] * 2, True, 1024)
    k64 = np.arange(64)[::-1].copy()
    c["64_keys_of_one_row"] = (
        MACHINES["sev"], [(k64, [B] * 64, np.zeros(64)), (k64, [B, Q] * 32, np.full(64, 4)),
                          (k64, [80.0] * 64, np.full(64, 9))], True, 1024)
    keys = np.concatenate([np.full(1000, 77), np.arange(200)])
    rng.shuffle(keys)
    for m in ("hyst", "cycle16", "wide"):
        c[f"a_1000_row_key_among_200_{m}"] = (
            MACHINES[m], [(keys, np.round(rng.uniform(35, 105, 1200), 1),
                           rng.integers(0, 5000, 1200))] * 2, True, 1024)
    c["first_element_changes_state"] = (MACHINES["hyst"], [_one_key([B, 85.0, Q], [7, 8, 9])],
                                        True, 1024)
    c["first_element_of_a_long_run_changes_state"] = (
        MACHINES["hyst"], [_one_key([B] * 130 + [Q], np.arange(131) + 50)], True, 1024)
    c["values_on_a_bound"] = (
        MACHINES["hyst"], [_one_key([90.0, 80.0, np.nextafter(80.0, 0), 80.0,
                                     np.nextafter(90.0, 0), 90.0, np.nextafter(80.0, 0)])],
        True, 1024)
    zero = ([0.0], [[0, 1], [0, 1]], 0, "change")
    c["minus_zero_meets_a_bound_of_zero"] = (
        zero, [_one_key([-0.0, -1e-300, 0.0, -5.0, -0.0])], True, 1024)
    c["nan_and_infinities"] = (
        MACHINES["sev"], [_one_key([B, NAN, INF, NAN, -INF, INF, 75.0, NAN])], True, 1024)
    c["nan_first"] = (MACHINES["sev"], [_one_key([NAN, NAN, B])], True, 1024)
    big = 1 << 53
    c["int_column"] = (MACHINES["sev"], [_one_key([80, 90, 70, 69, 85, 84])], False, 1024)
    c["int_column_beyond_2_53"] = (  # float(2**53 + 1) == 2.0**53: the class the doubles say
        ([-float(big), float(big)], [[0, 1, 2]] * 3, 1, "change"),
        [_one_key([big - 1, big, big + 1, -big, -big - 1, -big - 2, big + 2, K.I64_MIN,
                   K.I64_MAX, 0])], False, 1024)
    c["equal_timestamps"] = (MACHINES["sev"], [_one_key([B, Q, 80.0] * 30, [7] * 90)], True, 1024)
    c["decreasing_timestamps"] = (
        MACHINES["consec"], [_one_key([B] * 4 + [Q] + [B] * 95, np.arange(100, 0, -1))],
        True, 1024)
    c["key_at_cap_minus_1_then_growth"] = (
        MACHINES["hyst"], [(np.array([3, 3]), [B, Q], [0, 1]),
                           (np.array([13, 3, 13]), [B, B, Q], [2, 3, 4])], True, 4)
    keys = np.sort(rng.choice(9, 700, p=np.array([40, 20, 10, 10, 5, 5, 5, 3, 2]) / 100))
    rng.shuffle(keys[300:])      # runs of many lengths that cross the 64-row chunks
    for m in ("consec", "wide"):
        c[f"runs_across_chunk_boundaries_{m}"] = (
            MACHINES[m], [(keys, np.round(rng.uniform(35, 105, 700), 1),
                           rng.integers(0, 40, 700))] * 2, True, 1024)
    return c


HAND = _hand_cases()


def _hand(name, dev):
    machine, batches, is_float, capacity = HAND[name]
    op = KeyedStateMachineOperator(*machine, device=dev, capacity=capacity)
    model, rows = Model(*machine), []
    for keys, vals, ts in batches:
        vals = np.asarray(vals, dtype=np.float64 if is_float else np.int64)
        got = _rows(op.process(T(keys, dev), T(bits(vals, is_float), dev), T(ts, dev),
                               is_float=is_float))
        assert got == model.process(keys, vals, ts, is_float)
        rows.append(got)
    assert np.array_equal(op.state.cpu().numpy(), model.table_rows(op.cap))
    return op, rows


def _code(a, b):
    return a << 4 | b


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_built_batches(name):
    op, rows = _hand(name, "cpu")
    flat = [r for b in rows for r in b]
    if name == "key_at_cap_minus_1_then_growth":
        assert op.cap == 16
    if name == "first_element_changes_state":
        # the key's first element ever: its row's since is its own timestamp
        assert flat == [(0, _code(0, 1), 7, int(bits([B])[0]), 7),
                        (0, _code(1, 0), 7, int(bits([Q])[0]), 9)]
    if name == "first_element_of_a_long_run_changes_state":
        assert [r[1:3] + r[4:] for r in flat] == [(_code(0, 1), 50, 50), (_code(1, 0), 50, 180)]
    if name == "values_on_a_bound":
        assert [(r[1], r[4]) for r in flat] == [(_code(0, 1), 0), (_code(1, 0), 2),
                                                (_code(0, 1), 5), (_code(1, 0), 6)]
    if name == "minus_zero_meets_a_bound_of_zero":
        assert [(r[1], r[4]) for r in flat] == [(_code(0, 1), 0), (_code(1, 0), 1),
                                                (_code(0, 1), 2), (_code(1, 0), 3),
                                                (_code(0, 1), 4)]
    if name == "nan_and_infinities":   # a NaN is class 0
        assert [r[1] for r in flat] == [_code(0, 2), _code(2, 0), _code(0, 2), _code(2, 0),
                                        _code(0, 2), _code(2, 1), _code(1, 0)]
    if name == "int_column_beyond_2_53":
        # 2**53 + 1 rounds to 2.0**53 and meets the bound; -2**53 - 1 rounds to -2.0**53 and
        # meets the lower one
        assert [(r[1], r[4]) for r in flat] == [(_code(1, 2), 1), (_code(2, 1), 3),
                                                (_code(1, 0), 5), (_code(0, 2), 6),
                                                (_code(2, 0), 7), (_code(0, 2), 8),
                                                (_code(2, 1), 9)]
    if name.startswith("run_") and name.endswith("every_row_steps"):
        L = int(name.split("_")[1])
        assert sum(r[1] == _code(15, 0) for r in flat) == (2 * L) // 16


def test_exact_rows_of_a_small_example():
    op = KeyedStateMachineOperator([80.0, 90.0], [[0, 0, 1], [0, 1, 1]])
    keys, vals = [1, 2, 1, 1, 2, 1, 1], [95.0, 99.0, 85.0, 91.0, 50.0, 79.0, 89.0]
    ts = [0, 10, 200, 300, 320, 400, 500]
    got = _rows(op.process(T(keys), T(bits(vals)), T(ts)))
    b = lambda v: int(bits([v])[0])  # noqa: E731
    assert got == [(1, 0x01, 0, b(95.0), 0), (2, 0x01, 10, b(99.0), 10),
                   (2, 0x10, 10, b(50.0), 320), (1, 0x10, 0, b(79.0), 400)]
    assert op.metrics.num_records_in == 7 and op.metrics.num_records_out == 4
    assert [a.tolist() for a in op.entries()] == [[1, 2], [400, 320], [0, 0]]


def test_pack_puts_the_table_in_columns_and_the_pairs_in_masks():
    cuts, cols, masks = K.fsm_pack([1, 2.5], [[0, 1, 2], [2, 2, 0], [1, 0, 0]], [(0, 2), (2, 0),
                                                                                  (1, 1)])
    assert cuts == (1.0, 2.5) and all(isinstance(c, float) for c in cuts)
    assert cols == (0x120, 0x021, 0x002) and masks == (0b100, 0b010, 0b001)
    _, cols, masks = K.fsm_pack(*MACHINES["cycle16"][:2], MACHINES["cycle16"][3])
    assert cols == (0xFEDCBA9876543210, 0x0FEDCBA987654321) and masks[15] == 1 and masks[0] == 1


# ---- refusals ---------------------------------------------------------------------------------
def test_unsupported_batches_and_parameters_are_refused():
    op = KeyedStateMachineOperator(*MACHINES["hyst"], dense_limit=100)
    lim = K.SUSTAIN_TS_LIMIT
    for keys, ts in (([100], [1]), ([-1], [1]), ([1], [lim]), ([1], [-lim]), ([1], [K.I64_MIN])):
        with pytest.raises(TypeError):
            op.process(T(keys), T(bits([B])), T(ts))
    assert op.entries()[0].size == 0 and op.metrics.num_records_in == 0
    assert _rows(op.process(T([99, 99]), T(bits([B, Q])), T([-lim + 1, lim - 1]))) == \
        [(99, 0x01, -lim + 1, int(bits([B])[0]), -lim + 1),
         (99, 0x10, -lim + 1, int(bits([Q])[0]), lim - 1)]
    with pytest.raises(TypeError):
        op.process(T([1]).to(torch.int32), T(bits([B])), T([1]))
    bounds, table = MACHINES["hyst"][:2]
    bad_machines = (
        ([1.0], [[0]]), ([1.0] * 2, [[0, 0, 0]]), ([2.0, 1.0], [[0, 0, 0]]), ([NAN], [[0, 0]]),
        ([INF], [[0, 0]]), (list(range(16)), [[0] * 17]),            # C beyond 16
        ([1.0], [[0, 0]] * 17),                                        # S beyond 16
        ([1.0], [[0, 2], [0, 1]]), ([1.0], [[0, -1], [0, 1]]),         # an entry that is no state
        ([1.0], [[0, 1], [0]]), ([1.0], [[0, True], [0, 1]]), ([1.0], [[0, 1.0], [0, 1]]),
        ([1.0], []))
    for bad in bad_machines:
        with pytest.raises(ValueError):
            KeyedStateMachineOperator(*bad)
    with pytest.raises(TypeError):
        KeyedStateMachineOperator(["1"], [[0, 0]])
    for bad in (2, -1, True, 1.0, None):
        with pytest.raises(ValueError, match="initial"):
            KeyedStateMachineOperator(bounds, table, bad)
    for bad in ("changes", [(0, 2)], [(2, 0)], [(0, -1)], [(0, 1.0)]):
        with pytest.raises(ValueError):
            KeyedStateMachineOperator(bounds, table, 0, bad)
    m = K.load()
    assert (m.FSM_NONE, m.FSM_MAX_STATES, m.FSM_MAX_CLASSES, m.FSM_TAG_BITS) == \
        (NONE, K.FSM_MAX_STATES, K.FSM_MAX_CLASSES, K.FSM_TAG_BITS) and K.FSM_MAX_STATES == 16
    st = K.fsm_table(8, "cpu")
    kw = dict(kind=K.SUSTAIN_DOUBLE, **_packed("hyst"))
    with pytest.raises(ValueError):
        K.fsm_update(st, T([8]), T([0]), T([1]), **kw)                  # key out of range
    with pytest.raises(ValueError):
        K.fsm_update(st, T([-1]), T([0]), T([1]), **kw)
    for t in (lim, -lim):
        with pytest.raises(TypeError):
            K.fsm_update(st, T([1]), T([0]), T([t]), **kw)
    with pytest.raises(ValueError):
        K.fsm_update(st, T([1]), T([0]), T([1, 2]), **kw)
    with pytest.raises(ValueError, match="aligned"):
        K.fsm_update(st.view(-1)[1:15].view(7, 2), T([1]), T([0]), T([1]), **kw)  # alignment
    wide16 = [[0] * 16] * 16
    assert len(K.fsm_pack(list(range(15)), wide16, ())[1]) == 16
    bads = (dict(kind=2), dict(states=17, report=(0,) * 17), dict(states=0, report=()),
            dict(classes=17, cols=(0,) * 17, cuts=tuple(float(i) for i in range(16))),
            dict(classes=2), dict(initial=2), dict(initial=-1), dict(initial=True),
            dict(cols=(0x00, 0x10, 0x12)),              # a table entry >= S
            dict(cols=(0x100, 0x10, 0x11)),             # an entry above the last state
            dict(cols=(0x00, 0x10, 1 << 64)), dict(report=(2, 4)), dict(report=(2, -1)),
            dict(cuts=(90.0, 80.0)), dict(cuts=(80.0, NAN)), dict(cuts=(80, 90)))
    for bad in bads:
        with pytest.raises(ValueError):
            K.fsm_update(st, T([1]), T(bits([B])), T([1]), **{**kw, **bad})
    # the native side checks the rule too, whoever calls it
    for args in (((80.0, 90.0), (0x00, 0x10, 0x12), (2, 1), 0, 1),
                 ((90.0, 80.0), (0x00, 0x10, 0x11), (2, 1), 0, 1),
                 ((80.0, 90.0), (0x00, 0x10, 0x11), (2, 1), 2, 1),
                 ((80.0,), (0x00, 0x10, 0x11), (2, 1), 0, 1),
                 ((80.0, 90.0), (0x00, 0x10, 0x11), (2, 1) + (0,) * 15, 0, 1)):
        with pytest.raises(ValueError):
            m.cpu_fsm_update(0, 0, 0, 0, *args, st.data_ptr(), 8, 0, 0, 0, 0, 0)
    assert np.array_equal(st.numpy(), Model(*MACHINES["hyst"]).table_rows(8))
    for cap in (0, -1):
        with pytest.raises(ValueError):
            K.fsm_table(cap, "cpu")


def test_snapshot_rows_and_a_foreign_checkpoint():
    hyst = MACHINES["hyst"]
    op = KeyedStateMachineOperator(*hyst)
    op.process(T([1, 2, 2, 4, 4]), T(bits([B, B, 85.0, Q, B])), T([5, 6, 20, 7, 8]))
    op.advance_watermark(95)
    snap = op.snapshot_state()
    assert snap.meta["kind"] == "state_machine" and snap.meta["bounds"] == [80.0, 90.0]
    assert snap.meta["cols"] == [0x00, 0x10, 0x11] and snap.meta["report"] == [2, 1]
    assert snap.meta["wm"] == 95 and snap.meta["metrics"]["num_records_in"] == 5
    assert {k: v.tolist() for k, v in snap.columns.items()} == {
        "key": [1, 2, 4], "since": [5, 6, 8], "state": [1, 1, 1]}
    others = (([80.0, 91.0],) + hyst[1:], (hyst[0], [[0, 0, 1], [0, 0, 1]]) + hyst[2:],
              hyst[:2] + (1, "change"), hyst[:3] + ([(0, 1)],), MACHINES["sev"])
    for other in others:
        with pytest.raises(ValueError, match="different state-machine"):
            KeyedStateMachineOperator(*other).restore_state(snap.columns, snap.meta)
    with pytest.raises(ValueError, match="different state-machine"):
        KeyedStateMachineOperator(*hyst).restore_state(snap.columns, {"kind": "sustained"})
    # the same machine written with int bounds and explicit pairs is the same function
    fresh = KeyedStateMachineOperator([80, 90], hyst[1], 0, [(1, 0), (0, 1)], capacity=2)
    fresh.restore_state(snap.columns, snap.meta)
    assert fresh.wm == 95 and fresh.metrics.num_records_out == 3
    assert _rows(fresh.process(T([2, 1, 3]), T(bits([Q, B, Q])), T([30, 10, 11]))) == [
        (2, 0x10, 6, int(bits([Q])[0]), 30)]
    bad = dict(snap.columns, state=np.array([1, 2, 1]))
    with pytest.raises(ValueError, match="state the machine does not have"):
        KeyedStateMachineOperator(*hyst).restore_state(bad, snap.meta)


# ---- sanitizer --------------------------------------------------------------------------------
def test_sanitizer_harness_runs_clean():
    from mxstream.build import build_sanitize_fsm

    res = subprocess.run([str(build_sanitize_fsm())], capture_output=True, text=True,
                         timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.strip().splitlines()[-1] == "fsm sanitize ok"


# ---- GPU --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,seed,nkeys", CASES)
def test_gpu_engine_equals_the_per_record_model_across_a_snapshot(gpu_device, name, seed, nkeys):
    op = _run_engine(name, seed, nkeys, dev=gpu_device)
    assert op.device.type == "cuda"


@pytest.mark.gpu
@pytest.mark.parametrize("name,seed,nkeys", CASES)
def test_gpu_kernels_equal_the_twin(gpu_device, name, seed, nkeys):
    tabs = {d: K.fsm_table(nkeys, d) for d in ("cpu", gpu_device)}
    for c in _stream(seed, nkeys):
        if c[0] != "p":
            continue
        a, b = (_update(tabs[d], c, name, d) for d in ("cpu", gpu_device))
        assert len(a) == len(b) == 5
        assert all(torch.equal(x, y.cpu()) for x, y in zip(a, b))
        assert torch.equal(tabs["cpu"], tabs[gpu_device].cpu())


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(HAND))
def test_gpu_hand_built_batches(gpu_device, name):
    _, rows = _hand(name, gpu_device)
    assert rows == _hand(name, "cpu")[1]
