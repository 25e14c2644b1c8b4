"""The plain session model (tests/session_model.py) against the CPU session engine.

The GPU kernel tests (tests/test_session_kernels.py) compare the kernels with the model, so the
model itself is checked here, without a GPU: the same random batches go through the model and
through KeyedSessionOperator(device="cpu") (the host SessionStore), and the fired rows must be
identical. The inputs never hold more than K_SESS live sessions per key (asserted), the regime in
which the slot table and the store are the same function.
"""
from collections import Counter

import numpy as np
import pytest
import torch

import session_model as M
from mxstream.ops import kernels as K
from mxstream.runtime.session_operator import KeyedSessionOperator


def test_model_constants_match_the_package(native):
    names = ("AGG_SUM_I64", "AGG_SUM_F64", "AGG_MIN_I64", "AGG_MAX_I64", "AGG_MIN_F64",
             "AGG_MAX_F64", "AGG_COUNT", "AGG_AVG_F64", "AGG_AVG_I64", "I64_MIN", "I64_MAX")
    for n in names:
        assert getattr(M, n) == getattr(K, n), n
    for x in (0, 1, 5, 0xABCDEF01, (1 << 63) + 12345, M.U64 - 2):
        assert M.mix64(x) == native.mix64(x)


def test_model_table_and_set_checks():
    keys = [M.EMPTY_KEY] * 16
    slots = [M.table_insert(keys, 1, 3, k) for k in range(100, 106)]
    assert len(set(slots)) == 6 and all(8 <= s < 16 for s in slots)
    assert M.check_table(keys, 2, 3) == {(1, k): s for k, s in zip(range(100, 106), slots)}
    # a key behind an empty slot of its own chain is not reachable
    k, s = 100, slots[0] % 8
    bad = [M.EMPTY_KEY] * 8
    bad[(s + 2) % 8] = k
    with pytest.raises(AssertionError):
        M.check_table(bad, 1, 3)
    bad[s] = bad[(s + 1) % 8] = M.TOMB_KEY
    M.check_table(bad, 1, 3)
    with pytest.raises(AssertionError):
        M.check_table([7, 7], 1, 1)
    st = [M.EMPTY_KEY] * 16
    for k in (3, 4, 5, 3):
        M.set_insert(st, k)
    M.check_set(st, {3, 4, 5})
    assert M.set_contains(st, 4) and not M.set_contains(st, 6)


def test_model_fold_of_one_key():
    # gap 10, sessions [0,15) (fired) and [40,52): the run 14..20 re-opens the first (flags 3),
    # 31 joins the second, 100 is new; then a run that is late at wm 200; then overflow.
    pre = [(0, 15, 7, 2, 1), (40, 52, 5, 1, 0)]
    recs = [(14, 1), (20, 2), (31, 4), (100, 8)]
    r = M.fold_key(pre, 42, recs, 10, 1000, 20, M.AGG_SUM_I64)
    assert sorted(r["sessions"]) == [(0, 30, 10, 4, 3), (31, 52, 9, 2, 0), (100, 110, 8, 1, 0)]
    assert r["last"] == 100 and r["late"] == 0 and r["ovf"] == []
    assert r["due"] == 29
    r = M.fold_key(pre, 42, [(60, 1), (61, 1)], 10, 100, 200, M.AGG_SUM_I64)
    assert r["late"] == 2 and sorted(r["sessions"]) == sorted(pre)
    full = [(0, 5, 1, 1, 0), (10, 15, 1, 1, 0), (20, 25, 1, 1, 0), (30, 35, 1, 1, 0)]
    r = M.fold_key(full, 0, [(50, 9), (70, 9), (71, 3)], 1, 0, M.I64_MIN, M.AGG_SUM_I64)
    # 50 overflows, and so does every later run
    assert r["ovf"] == [(50, 51, 9, 1), (70, 72, 12, 2)] and sorted(r["sessions"]) == full
    r = M.fold_key(full, 0, [(12, 3), (50, 9)], 1, 0, M.I64_MIN, M.AGG_SUM_I64)
    assert r["ovf"] == [(50, 51, 9, 1)]
    assert (10, 15, 4, 2, 0) in r["sessions"] and len(r["sessions"]) == 4


def _events(seed, n, nkeys, span, disorder, straggle):
    """Roughly time-ordered events; every 40th one arrives `straggle` ms behind (late data)."""
    rng = np.random.default_rng(seed)
    ts = np.sort(rng.integers(0, span, n)) + rng.integers(-disorder, disorder + 1, n)
    ts[39::40] -= straggle
    return [(int(k), int(max(t, 0)), int(v)) for k, t, v in
            zip(rng.integers(0, nkeys, n), ts, rng.integers(-50, 100, n))]


@pytest.mark.parametrize("agg", [K.AGG_SUM_I64, K.AGG_MIN_I64, K.AGG_MAX_I64, K.AGG_COUNT])
@pytest.mark.parametrize("seed,gap,lateness,batch", [(1, 5, 0, 64), (2, 100, 300, 50),
                                                     (3, 400, 300, 97), (4, 100, 2000, 1)])
def test_model_equals_cpu_engine(seed, gap, lateness, batch, agg):
    n = 3000 if batch > 1 else 400
    events = _events(seed, n, 300, 10 * n, 400, gap + lateness + 600)
    op = KeyedSessionOperator(gap=gap, lateness=lateness, agg=agg, device="cpu", max_keys=1 << 10,
                              batch_capacity=max(batch, 64), ooo_bound=100)
    model = M.SessionTable(gap, lateness, agg)
    got, want = Counter(), Counter()
    wm = M.I64_MIN
    most, refired = 0, 0

    def take(rows):
        for k, s, e, r, c in zip(rows.keys, rows.start, rows.end, rows.raw, rows.counts):
            got[(int(k), int(s), int(e), int(r), int(c))] += 1

    for i in range(0, n, batch):
        chunk = events[i:i + batch]
        k, t, v = (torch.tensor([e[j] for e in chunk], dtype=torch.int64) for j in range(3))
        take(op.process(k, t, v))
        assert model.fold(chunk, wm) == {}          # no overflow: the slot table's regime
        touched = [model.rows[k][0] for k in {e[0] for e in chunk}]
        most = max(most, max(len(r) for r in touched))
        refired += sum(s[4] == 3 for r in touched for s in r)
        wm = op.wm                                   # the watermark is an input of the model
        want.update(model.fire(wm))
    take(op.finish())
    want.update(model.fire(M.I64_MAX))
    assert most <= M.K_SESS
    assert got == want
    assert model.late == op.metrics.num_late_records_dropped
    if lateness:
        assert refired > 0 and model.late > 0       # the interesting branches were taken
