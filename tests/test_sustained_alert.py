"""Sustained-condition alerts (csrc/mxs_sustain.h): the C++ twin and the engine operator
(runtime/sustain_operator.py) against a per-record model of SustainedAlert (a dict per key), and
the gfx950 kernels against the twin array for array. Everything is an integer or a bit pattern
and compares exactly, row for row and in order."""
from __future__ import annotations

import functools
import subprocess

import numpy as np
import pytest
import torch

from mxstream.api import functions as F
from mxstream.ops import kernels as K
from mxstream.runtime.sustain_operator import KeyedSustainOperator, threshold_bits

NONE = K.SUSTAIN_NONE
KEY_SPACES = [1, 7, 300, 4095, 4096, 4097, 8193]
FORS = [0, 40]
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
    """SustainedAlert record by record: key -> (since, firing, the batch that opened the run)."""

    def __init__(self, when, threshold, for_ms):
        self.cmp = F._LOOKUP_WHENS[when]
        self.thr, self.for_ms, self.state, self.batch = float(threshold), for_ms, {}, 0
        self.carried = 0  # code-1 rows whose run began in an earlier batch

    def process(self, keys, vals, ts, is_float=True) -> list:
        """Rows (key, code, since, value bits, ts) in arrival order."""
        out = []
        vb = bits(vals, is_float).tolist()
        for k, v, b, t in zip(np.asarray(keys).tolist(), np.asarray(vals).tolist(), vb,
                              np.asarray(ts).tolist()):
            cur = self.state.get(k)
            if self.cmp(float(v), self.thr):
                since, firing, born = cur if cur is not None else (t, False, self.batch)
                if not firing and t - since >= self.for_ms:
                    firing = True
                    out.append((k, 1, since, b, t))
                    self.carried += born < self.batch
                self.state[k] = (since, firing, born)
            else:
                if cur is not None and cur[1]:
                    out.append((k, 0, cur[0], b, t))
                self.state.pop(k, None)
        self.batch += 1
        return out

    def table(self, cap: int) -> np.ndarray:
        st = np.zeros((cap, 2), dtype=np.int64)
        st[:, 0] = NONE
        for k, (since, firing, _) in self.state.items():
            st[k] = (since, int(firing))
        return st


@functools.lru_cache(maxsize=None)
def _stream(seed: int, nkeys: int, steps: int = 24):
    """The keyed-timer tests' call generator -- ("p", keys, ts, vals) and ("w", wm) calls: 0 to
    399 rows per step, +-30 ms of disorder, late elements, equal timestamps for one key, empty
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
def _expected(seed: int, nkeys: int, for_ms: int):
    """The model over a stream, computed once: every "p" call's rows, the final table, and the
    number of code-1 rows from a run begun in an earlier batch."""
    model = Model(">", 70.0, for_ms)
    rows = [model.process(c[1], c[3], c[2]) for c in _stream(seed, nkeys) if c[0] == "p"]
    return rows, model.table(nkeys), model.carried


CASES = [(s, k, f) for s in SEEDS for k in KEY_SPACES for f in FORS]


def _rows(chunks) -> list:
    out = []
    for cols in chunks:
        out.extend(zip(*(c.cpu().tolist() for c in cols)))
    return out


# ---- the streams hold what they are meant to test ---------------------------------------------
@pytest.mark.parametrize("nkeys", KEY_SPACES)
@pytest.mark.parametrize("for_ms", FORS)
def test_streams_hold_fires_resolves_and_runs_across_batches(nkeys, for_ms):
    for seed in SEEDS:
        rows, _, carried = _expected(seed, nkeys, for_ms)
        flat = [r for b in rows for r in b]
        assert sum(r[1] == 1 for r in flat) >= 1 and sum(r[1] == 0 for r in flat) >= 1
        if for_ms:
            assert carried >= 1
        assert sum(c[0] == "p" and len(c[1]) == 0 for c in _stream(seed, nkeys)) >= 1


# ---- the twin and the engine against the per-record model -------------------------------------
def _update(state, call, for_ms, dev="cpu"):
    return K.sustain_update(state, T(call[1], dev), T(bits(call[3]), dev), T(call[2], dev),
                            kind=K.SUSTAIN_DOUBLE, when=">", threshold_bits=threshold_bits(70.0),
                            for_ms=for_ms)


@pytest.mark.parametrize("seed,nkeys,for_ms", CASES)
def test_twin_equals_the_per_record_model(seed, nkeys, for_ms):
    want, table, _ = _expected(seed, nkeys, for_ms)
    state = K.sustain_table(nkeys, "cpu")
    got = [_rows([_update(state, c, for_ms)]) for c in _stream(seed, nkeys) if c[0] == "p"]
    assert got == want
    assert np.array_equal(state.numpy(), table)


def _run_engine(seed, nkeys, for_ms, dev="cpu", snapshot=True):
    calls = _stream(seed, nkeys)
    make = lambda: KeyedSustainOperator(">", 70.0, for_ms, device=dev)  # noqa: E731
    op, got = make(), []
    for i, c in enumerate(calls):
        if snapshot and i == len(calls) // 2:
            snap = op.snapshot_state()
            assert snap.meta["kind"] == "sustained" and snap.meta["for_ms"] == for_ms
            op = make()
            op.restore_state(snap.columns, snap.meta)
        if c[0] == "w":
            assert op.advance_watermark(c[1]) == []
            continue
        chunks = op.process(T(c[1], dev), T(bits(c[3]), dev), T(c[2], dev))
        assert len(chunks) <= 1 and all(len(cols) == 5 for cols in chunks)
        got.append(_rows(chunks))
    want, table, _ = _expected(seed, nkeys, for_ms)
    assert got == want
    st = op.state.cpu().numpy()     # the capacity covers the largest key seen, not nkeys
    full = Model(">", 70.0, for_ms).table(max(op.cap, nkeys))
    full[:nkeys] = table
    assert np.array_equal(st, full[:op.cap]) and (full[op.cap:, 0] == NONE).all()
    ids, since, firing = op.entries()
    assert ids.tolist() == np.nonzero(table[:, 0] != NONE)[0].tolist()
    return op


@pytest.mark.parametrize("seed,nkeys,for_ms", CASES)
def test_engine_equals_the_per_record_model_across_a_snapshot(seed, nkeys, for_ms):
    op = _run_engine(seed, nkeys, for_ms)
    if nkeys > 4096:
        assert KeyedSustainOperator(">", 70.0, for_ms).cap < 4096 <= op.cap  # it grew


# ---- hand-built batches: the smallest shapes where the scan can go wrong ----------------------
B, Q = 80.0, 10.0   # a breaching and a quiet value under "> 70"


def _one_key(vals, ts=None, key=0):
    n = len(vals)
    return (np.full(n, key), vals, np.arange(n) if ts is None else ts)


def _hand_cases():
    """name -> (rule (when, threshold, for_ms), [batches (keys, vals, ts)], is_float, capacity)."""
    c = {}
    for L in (1, 63, 64, 65, 128, 129):
        for for_ms in (0, L - 1, L):
            c[f"run_{L}_for_{for_ms}"] = ((">", 70.0, for_ms),
                                          [_one_key([Q] + [B] * L + [Q] + [B] * 3)], True, 1024)
    for p in (0, 63, 64, 129):
        vals = [B] * 130
        vals[p] = Q
        c[f"quiet_only_at_{p}"] = ((">", 70.0, 3), [_one_key([B] * 5), _one_key(vals)], True, 1024)
    c["for_exact"] = ((">", 70.0, 50), [_one_key([B, B, B], [0, 49, 50])], True, 1024)
    c["for_one_below"] = ((">", 70.0, 50), [_one_key([B, B, B, Q], [0, 49, 49, 60])], True, 1024)
    c["open_fire_resolve_in_three_batches"] = (
        (">", 70.0, 10), [_one_key([Q, B], [0, 1], key=3), _one_key([B, B], [5, 11], key=3),
                          _one_key([B, Q, Q], [12, 13, 14], key=3)], True, 1024)
    c["resolve_then_fire_in_one_chunk_for_0"] = (
        (">", 70.0, 0), [_one_key([B, B]), _one_key([B, Q, B, Q, Q, B])], True, 1024)
    c["resolve_then_fire_in_one_chunk_for_2"] = (
        (">", 70.0, 2), [_one_key([B, B, B]), _one_key([B, Q, B, B, B, B, Q, B], np.arange(8) + 3)],
        True, 1024)
    c["equal_timestamps_for_0"] = ((">", 70.0, 0), [_one_key([B] * 70 + [Q], [7] * 71)], True, 1024)
    c["equal_timestamps_for_1"] = ((">", 70.0, 1), [_one_key([B] * 70 + [Q], [7] * 71)], True, 1024)
    c["decreasing_timestamps"] = (
        (">", 70.0, 5), [_one_key([B] * 100 + [Q], np.arange(100, -1, -1))], True, 1024)
    c["decreasing_then_a_jump"] = (
        (">", 70.0, 5), [_one_key([B] * 67 + [Q], list(range(66, 0, -1)) + [71, 72])], True, 1024)
    c["an_early_maximum_fires_later_lanes_do_not"] = (
        (">", 70.0, 5), [_one_key([B] * 6 + [Q], [10, 20, 3, 4, 30, 5, 6])], True, 1024)
    c["empty"] = ((">", 70.0, 0), [_one_key([]), _one_key([B]), _one_key([])], True, 1024)
    c["one_row"] = ((">", 70.0, 0), [_one_key([B], [4], key=9), _one_key([Q], [5], key=9)],
                    True, 1024)
    k64 = np.arange(64)[::-1].copy()
    c["64_keys_of_one_row"] = (
        (">", 70.0, 4), [(k64, [B] * 64, np.zeros(64)), (k64, [B, Q] * 32, np.full(64, 4)),
                         (k64, [Q] * 64, np.full(64, 9))], True, 1024)
    for when in (">", ">=", "<", "<=", "==", "!="):
        c[f"nan_values_{when}"] = ((when, 70.0, 1), [_one_key([NAN, B, NAN, 70.0, NAN, NAN, Q])],
                                   True, 1024)
        c[f"nan_threshold_{when}"] = ((when, NAN, 1), [_one_key([NAN, B, B, 70.0])], True, 1024)
    big = 1 << 53
    c["int_column"] = ((">", 70, 1), [_one_key([80, 90, 70, 71, 72])], False, 1024)
    c["int_column_beyond_2_53"] = (  # float(2**53 + 1) == 2.0**53: no breach, as the doubles say
        (">", float(big), 0), [_one_key([big + 1, big + 2, big + 1, K.I64_MAX, K.I64_MIN])],
        False, 1024)
    c["double_column_int_threshold"] = ((">=", 70, 2), [_one_key([70.0, 69.9, 70.5, 71.0, 72.0])],
                                        True, 1024)
    c["two_capacity_doublings"] = (
        (">", 70.0, 1), [(np.array([3, 3]), [B, B], [0, 1]), (np.array([13, 3, 13]), [B, Q, B],
                                                               [2, 3, 4])], True, 4)
    rng = np.random.default_rng(11)   # runs of many lengths that cross the 64-row chunks
    keys = np.sort(rng.choice(9, 700, p=np.array([40, 20, 10, 10, 5, 5, 5, 3, 2]) / 100))
    rng.shuffle(keys[300:])
    c["runs_across_chunk_boundaries"] = (
        (">", 70.0, 6), [(keys, np.where(rng.random(700) < 0.8, B, Q), rng.integers(0, 40, 700))] * 2,
        True, 1024)
    return c


HAND = _hand_cases()


def _hand(name, dev):
    (when, thr, for_ms), batches, is_float, capacity = HAND[name]
    op = KeyedSustainOperator(when, thr, for_ms, device=dev, capacity=capacity)
    model, total = Model(when, thr, for_ms), 0
    for keys, vals, ts in batches:
        vals = np.asarray(vals, dtype=np.float64 if is_float else np.int64)
        got = _rows(op.process(T(keys, dev), T(bits(vals, is_float), dev), T(ts, dev),
                               is_float=is_float))
        assert got == model.process(keys, vals, ts, is_float)
        total += len(got)
    assert np.array_equal(op.state.cpu().numpy(), model.table(op.cap))
    return op, total


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_built_batches(name):
    op, total = _hand(name, "cpu")
    if name == "two_capacity_doublings":
        assert op.cap == 16
    if name in ("for_exact", "open_fire_resolve_in_three_batches", "64_keys_of_one_row",
                "int_column", "nan_values_!=", "nan_threshold_!=", "run_129_for_128"):
        assert total >= 1
    if name in ("for_one_below", "decreasing_timestamps", "nan_threshold_>", "nan_values_==",
                "run_64_for_64"):
        assert total == 0
    if name == "int_column_beyond_2_53":
        assert total == 4   # 2**53 + 2 and INT64_MAX breach as doubles, 2**53 + 1 does not


def test_exact_rows_of_a_small_example():
    op = KeyedSustainOperator(">", 90.0, 300)
    keys, vals = [1, 2, 1, 1, 2, 1, 1], [95.0, 99.0, 96.0, 97.0, 50.0, 91.0, 10.0]
    ts = [0, 10, 200, 300, 320, 400, 500]
    got = _rows(op.process(T(keys), T(bits(vals)), T(ts)))
    assert got == [(1, 1, 0, int(bits([97.0])[0]), 300), (1, 0, 0, int(bits([10.0])[0]), 500)]
    assert op.metrics.num_records_in == 7 and op.metrics.num_records_out == 2
    assert op.entries()[0].size == 0


# ---- refusals ---------------------------------------------------------------------------------
def test_unsupported_batches_and_parameters_are_refused():
    op = KeyedSustainOperator(">", 70.0, 10, dense_limit=100)
    lim = K.SUSTAIN_TS_LIMIT
    for keys, ts in (([100], [1]), ([-1], [1]), ([1], [lim]), ([1], [-lim]), ([1], [K.I64_MIN])):
        with pytest.raises(TypeError):
            op.process(T(keys), T(bits([B])), T(ts))
    assert op.entries()[0].size == 0 and op.metrics.num_records_in == 0
    assert _rows(op.process(T([99, 99]), T(bits([B, B])), T([-lim + 1, lim - 1]))) == \
        [(99, 1, -lim + 1, int(bits([B])[0]), lim - 1)]
    with pytest.raises(TypeError):
        op.process(T([1]).to(torch.int32), T(bits([B])), T([1]))
    for bad in (-1, True, 1.5, None):
        with pytest.raises(ValueError):
            KeyedSustainOperator(">", 70.0, bad)
    for bad in (None, "=>", 3):
        with pytest.raises(ValueError):
            KeyedSustainOperator(bad, 70.0, 1)
    for bad in (True, "70", None):
        with pytest.raises(TypeError):
            KeyedSustainOperator(">", bad, 1)
    m = K.load()
    assert (m.SUSTAIN_NONE, m.SUSTAIN_TS_LIMIT, m.SUSTAIN_LONG, m.SUSTAIN_DOUBLE) == \
        (NONE, lim, K.SUSTAIN_LONG, K.SUSTAIN_DOUBLE)
    st = K.sustain_table(8, "cpu")
    kw = dict(kind=K.SUSTAIN_DOUBLE, when=">", threshold_bits=0, for_ms=1)
    with pytest.raises(ValueError):
        K.sustain_update(st, T([8]), T([0]), T([1]), **kw)
    with pytest.raises(TypeError):
        K.sustain_update(st, T([1]), T([0]), T([lim]), **kw)
    with pytest.raises(ValueError):
        K.sustain_update(st, T([1]), T([0]), T([1, 2]), **kw)
    with pytest.raises(ValueError):
        K.sustain_update(st.view(-1)[1:15].view(7, 2), T([1]), T([0]), T([1]), **kw)  # alignment
    for bad in (dict(when=None), dict(for_ms=-1), dict(kind=2)):
        with pytest.raises(ValueError):
            K.sustain_update(st, T([1]), T([0]), T([1]), **{**kw, **bad})
    assert np.array_equal(st.numpy(), Model(">", 0, 0).table(8))


def test_snapshot_rows_and_a_foreign_checkpoint():
    op = KeyedSustainOperator(">", 70.0, 5)
    op.process(T([1, 2, 2, 4, 4]), T(bits([B, B, B, B, Q])), T([5, 6, 20, 7, 8]))
    op.advance_watermark(95)
    snap = op.snapshot_state()
    assert snap.meta["kind"] == "sustained" and snap.meta["when"] == ">"
    assert snap.meta["wm"] == 95 and snap.meta["metrics"]["num_records_in"] == 5
    assert {k: v.tolist() for k, v in snap.columns.items()} == {
        "key": [1, 2], "since": [5, 6], "firing": [0, 1]}
    for other in ((">", 70.0, 6), (">=", 70.0, 5), (">", 71.0, 5)):
        with pytest.raises(ValueError, match="different sustained"):
            KeyedSustainOperator(*other).restore_state(snap.columns, snap.meta)
    with pytest.raises(ValueError, match="different sustained"):
        KeyedSustainOperator(">", 70.0, 5).restore_state(snap.columns, {"kind": "count_timeout"})
    fresh = KeyedSustainOperator(">", 70.0, 5, capacity=2)
    fresh.restore_state(snap.columns, snap.meta)
    assert fresh.wm == 95 and fresh.metrics.num_records_out == 1
    assert _rows(fresh.process(T([2, 1]), T(bits([Q, B])), T([30, 10]))) == [
        (2, 0, 6, int(bits([Q])[0]), 30), (1, 1, 5, int(bits([B])[0]), 10)]


# ---- sanitizer --------------------------------------------------------------------------------
def test_sanitizer_harness_runs_clean():
    from mxstream.build import build_sanitize_sustain

    res = subprocess.run([str(build_sanitize_sustain())], capture_output=True, text=True,
                         timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.strip().splitlines()[-1] == "sustain sanitize ok"


# ---- GPU --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("seed,nkeys,for_ms", CASES)
def test_gpu_engine_equals_the_per_record_model_across_a_snapshot(gpu_device, seed, nkeys, for_ms):
    op = _run_engine(seed, nkeys, for_ms, dev=gpu_device)
    assert op.device.type == "cuda"


@pytest.mark.gpu
@pytest.mark.parametrize("seed,nkeys,for_ms", CASES)
def test_gpu_kernels_equal_the_twin(gpu_device, seed, nkeys, for_ms):
    tabs = {d: K.sustain_table(nkeys, d) for d in ("cpu", gpu_device)}
    for c in _stream(seed, nkeys):
        if c[0] != "p":
            continue
        a, b = (_update(tabs[d], c, for_ms, d) for d in ("cpu", gpu_device))
        assert len(a) == len(b) == 5
        assert all(torch.equal(x, y.cpu()) for x, y in zip(a, b))
        assert torch.equal(tabs["cpu"], tabs[gpu_device].cpu())


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(HAND))
def test_gpu_hand_built_batches(gpu_device, name):
    _, total = _hand(name, gpu_device)
    assert total == _hand(name, "cpu")[1]
