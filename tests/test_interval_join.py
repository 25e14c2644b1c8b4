"""Interval-join kernels (csrc/ijoin_hip.hip, twins csrc/ijoin_cpu.cpp) and the engine operator
(runtime/interval_join_operator.py) against a per-record Python model of Flink 1.8's
IntervalJoinOperator. Every comparison is exact: arrays and multisets."""
from __future__ import annotations

import functools
import subprocess
from collections import Counter

import numpy as np
import pytest
import torch

from mxstream.ops import kernels as K
from mxstream.runtime.interval_join_operator import KeyedIntervalJoinOperator

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
BOUNDS = [(-3, 5), (0, 0), (2, 7), (-7, -2), (-3 + 1, 5), (-3, 5 - 1), (2 + 1, 7 - 1), (0, 1 - 1)]


def sat(a: int, b: int) -> int:
    return max(I64_MIN, min(I64_MAX, a + b))


class Model:
    """Flink's rules, record by record: buffers in arrival order per side."""

    def __init__(self, lo: int, hi: int):
        if lo > hi:
            raise ValueError("lowerBound <= upperBound must be fulfilled")
        self.lo, self.hi, self.wm, self.late = lo, hi, I64_MIN, 0
        self.buf = ([], [])  # (key, ts, val)

    def element(self, side: int, k: int, t: int, v: int) -> list:
        if t == I64_MIN:
            raise ValueError("no timestamp")
        if self.wm != I64_MIN and t < self.wm:
            self.late += 1
            return []
        rlo, rhi = (self.lo, self.hi) if side == 0 else (-self.hi, -self.lo)
        out = []
        for ok, ot, ov in self.buf[1 - side]:
            if ok == k and sat(t, rlo) <= ot <= sat(t, rhi):
                out.append((k, v, ov, max(t, ot)) if side == 0 else (k, ov, v, max(t, ot)))
        self.buf[side].append((k, t, v))
        return out

    def batch(self, side: int, keys, ts, vals) -> list:
        """A batch sees only the other side's elements of earlier calls."""
        out = []
        for k, t, v in zip(keys, ts, vals):
            out += self.element(side, int(k), int(t), int(v))
        return out

    def watermark(self, wm: int) -> None:
        if wm <= self.wm:
            return
        self.wm = wm
        for s, keep in ((0, max(self.hi, 0)), (1, max(-self.lo, 0))):
            self.buf[s][:] = [e for e in self.buf[s] if not wm >= sat(e[1], keep)]

    def sorted_buf(self, side: int):
        rows = sorted(self.buf[side], key=lambda e: (e[0], e[1]))  # stable: arrival order on ties
        return np.array(rows, dtype=np.int64).reshape(-1, 3).T


def T(x, dev="cpu"):
    return torch.tensor(np.asarray(x, dtype=np.int64), dtype=torch.int64, device=dev)


def cols(rows, dev="cpu"):
    """(key, ts, val) rows, sorted by (key, ts) -> three columns."""
    rows = sorted(rows, key=lambda e: (e[0], e[1]))
    a = np.array(rows, dtype=np.int64).reshape(-1, 3)
    return tuple(T(a[:, i].copy(), dev) for i in range(3))


def brute(side, batch, other, lo, hi, cutoff=I64_MIN):
    """The nested loop over sorted columns, in the kernels' order."""
    rlo, rhi = (lo, hi) if side == 0 else (-hi, -lo)
    bk, bt, bv = (c.tolist() for c in batch)
    ok, ot, ov = (c.tolist() for c in other)
    out = []
    for i in range(len(bk)):
        for o in range(len(ok)):
            if ok[o] == bk[i] and ot[o] > cutoff and sat(bt[i], rlo) <= ot[o] <= sat(bt[i], rhi):
                l, r = (bv[i], ov[o]) if side == 0 else (ov[o], bv[i])
                out.append((bk[i], l, r, max(bt[i], ot[o])))
    return np.array(out, dtype=np.int64).reshape(-1, 4).T


def expand(jp, p0=0, p1=None) -> np.ndarray:
    p1 = jp.pairs if p1 is None else p1
    return np.stack([c.cpu().numpy() for c in K.ijoin_expand(jp, p0, p1)])


def random_rows(rng, n, nkeys=5, tspan=12, base=0):
    return [(int(k), int(t), base + i) for i, (k, t) in
            enumerate(zip(rng.integers(0, nkeys, n), rng.integers(0, tspan, n)))]


# ---- twins against the model ---------------------------------------------------------------
@pytest.mark.parametrize("lo,hi", BOUNDS)
def test_twin_equals_the_nested_loop(lo, hi):
    rng = np.random.default_rng(1000 + lo * 31 + hi)
    for side in (0, 1):
        batch, other = cols(random_rows(rng, 90)), cols(random_rows(rng, 120, base=1000))
        for cutoff in (I64_MIN, 4, I64_MAX):
            jp = K.ijoin_plan(side, batch, other, lo, hi, cutoff)
            want = brute(side, batch, other, lo, hi, cutoff)
            assert jp.pairs == want.shape[1]
            np.testing.assert_array_equal(expand(jp), want)
            first = jp.plan[:jp.rows + 1].numpy()
            assert (np.diff(first) > 0).all() and first[-1] == jp.pairs


def _engine_vs_model(lo, hi, dev="cpu", steps=30, seed=0, chunk=1 << 24, snapshot_at=None):
    rng = np.random.default_rng(seed)
    op = KeyedIntervalJoinOperator(lo=lo, hi=hi, device=dev, pair_chunk=chunk, capacity=4)
    mo = Model(lo, hi)
    wm = 0
    for step in range(steps):
        if snapshot_at == step:
            sn = op.snapshot_state()
            op = KeyedIntervalJoinOperator(lo=lo, hi=hi, device=dev, pair_chunk=chunk)
            # key groups come back in another order, each in the snapshot's
            perm = np.argsort(-sn.kg.astype(np.int64), kind="stable")
            op.restore_state({k: v[perm] for k, v in sn.columns.items()}, sn.meta)
        side = int(rng.integers(0, 2))
        n = int(rng.integers(0, 40))
        rows = random_rows(rng, n, nkeys=4, tspan=14, base=step * 1000)
        rows = [(k, t + wm - 3, v) for k, t, v in rows]  # some late, many duplicates
        k, t, v = (T([r[i] for r in rows], dev) for i in range(3))
        got = op.process(side, k, t, v)
        want = mo.batch(side, *zip(*rows)) if rows else []
        got_rows = np.concatenate([np.stack([c.cpu().numpy() for c in ch]) for ch in got], axis=1) \
            if got else np.zeros((4, 0), np.int64)
        assert all(ch[0].numel() <= chunk for ch in got)
        assert Counter(map(tuple, got_rows.T.tolist())) == Counter(want), step
        assert op.metrics.num_late_records_dropped == mo.late
        if rng.random() < 0.5:
            wm += int(rng.integers(0, 5))
            assert op.advance_watermark(wm) == []
            mo.watermark(wm)
        for s in (0, 1):
            np.testing.assert_array_equal(np.stack(op.buffered(s)), mo.sorted_buf(s))
    return op


@pytest.mark.parametrize("lo,hi", BOUNDS)
def test_engine_equals_model(lo, hi):
    op = _engine_vs_model(lo, hi, seed=100 + hi + lo)
    assert op.pairs_out == op.metrics.num_records_out > 0


@pytest.mark.parametrize("snapshot_at", [5, 10, 15, 20])
@pytest.mark.parametrize("lo,hi", BOUNDS + [(0, 3), (-3, 0)])
def test_engine_chunked_and_snapshot_restore_continue_identically(lo, hi, snapshot_at):
    """Also bounds that keep a side for 0 ms: its rows at ts == wm live until the next watermark,
    in a restored operator as in an uninterrupted one."""
    for seed in (5, 6, 7):
        _engine_vs_model(lo, hi, chunk=7 if seed == 5 else 1 << 24, snapshot_at=snapshot_at,
                         seed=seed * 100 + snapshot_at)


def test_restored_operator_keeps_rows_at_the_watermark():
    for lo, hi in [(0, 3), (-3, 0), (0, 0)]:
        got = []
        for restore in (False, True):
            op = KeyedIntervalJoinOperator(lo=lo, hi=hi)
            op.advance_watermark(10)
            op.process(1, T([1]), T([10]), T([7]))
            op.process(0, T([2]), T([10]), T([5]))
            if restore:
                sn = op.snapshot_state()
                op = KeyedIntervalJoinOperator(lo=lo, hi=hi)
                op.restore_state(sn.columns, sn.meta)
            got.append(sum(c[0].numel() for c in op.process(0, T([1]), T([10]), T([8])))
                       + sum(c[0].numel() for c in op.process(1, T([2]), T([10]), T([9]))))
            op.advance_watermark(11)
            assert all(op.buffered(s)[0].size == (0 if op.keep[s] == 0 else 2) for s in (0, 1))
        assert got == [2, 2]


def test_foreign_checkpoint_is_refused():
    sn = KeyedIntervalJoinOperator(lo=-3, hi=5).snapshot_state()
    with pytest.raises(ValueError, match="different interval join"):
        KeyedIntervalJoinOperator(lo=-3, hi=4).restore_state(sn.columns, sn.meta)
    with pytest.raises(ValueError, match="different interval join"):
        KeyedIntervalJoinOperator(lo=-3, hi=5).restore_state({}, {"kind": "join_window"})


def test_lazy_purge_never_leaks_an_expired_row():
    op = KeyedIntervalJoinOperator(lo=-2, hi=5)
    op.process(0, T([1, 1, 2]), T([10, 20, 10]), T([1, 2, 3]))
    op.advance_watermark(15)  # l(1, 10) and l(2, 10) expire: 15 >= 10 + 5
    assert op.n[0] == 3  # not compacted yet
    got = op.process(1, T([1, 1, 2]), T([15, 20, 15]), T([7, 8, 9]))
    assert sorted(map(tuple, np.stack([c.numpy() for c in got[0]]).T.tolist())) == [(1, 2, 8, 20)]
    sn = op.snapshot_state()
    left = sn.columns["side"] == 0
    assert sn.columns["ts"][left].tolist() == [20] and op.n[0] == 1
    # The right rows (ts 15, 20; kept for max(-lo, 0) = 2) are all alive at watermark 15.
    assert sorted(sn.columns["ts"][~left].tolist()) == [15, 15, 20]


# ---- edges ---------------------------------------------------------------------------------
def test_edges_empty_sides_neighbour_key_gap_and_ties():
    empty = cols([])
    other = cols([(1, 10, 100), (1, 12, 101), (2, 10, 200), (2, 10, 201), (3, 11, 300)])
    assert K.ijoin_plan(0, cols([(2, 10, 1)]), empty, -3, 5).pairs == 0
    assert K.ijoin_plan(0, empty, other, -3, 5).pairs == 0
    assert expand(K.ijoin_plan(0, empty, other, -3, 5)).shape == (4, 0)
    # key 2 at ts 30 has neighbours (1, 12) and (3, 11) in range of nothing it owns
    jp = K.ijoin_plan(0, cols([(2, 10, 1), (2, 30, 2), (4, 10, 3)]), other, 0, 0)
    np.testing.assert_array_equal(expand(jp), [[2, 2], [1, 1], [200, 201], [10, 10]])
    # an element with no match between two that match: two plan rows, the idx column skips it
    batch = cols([(1, 11, 1), (1, 50, 2), (2, 11, 3)])
    jp = K.ijoin_plan(1, batch, other, -1, 2)
    assert jp.cnt.tolist() == [2, 0, 2] and jp.rows == 2
    assert jp.plan[4:6].tolist() == [0, 2]  # the idx column (stride n + 1 = 4)
    np.testing.assert_array_equal(expand(jp), brute(1, batch, other, -1, 2))
    # a key of the neighbour whose ts is in range must not match
    jp = K.ijoin_plan(0, cols([(2, 11, 1)]), cols([(1, 11, 5), (3, 11, 6)]), -5, 5)
    assert jp.pairs == 0


def test_merge_ties_keep_old_rows_first_and_batches_outside():
    old = cols([(1, 10, 100), (2, 10, 200), (2, 10, 201), (2, 15, 202), (3, 1, 300)])
    for batch, want in [
        (cols([(2, 10, 1), (2, 10, 2)]), [100, 200, 201, 1, 2, 202, 300]),
        (cols([(0, 99, 1), (1, 9, 2)]), [1, 2, 100, 200, 201, 202, 300]),     # entirely before
        (cols([(3, 1, 1), (3, 2, 2), (9, 0, 3)]), [100, 200, 201, 202, 300, 1, 2, 3]),  # after
        (cols([]), [100, 200, 201, 202, 300]),
    ]:
        out = torch.full((3, 9), -1, dtype=torch.int64)
        n = K.ijoin_merge(old, batch, out)
        assert out[2, :n].tolist() == want
        assert (out[:, n:] == -1).all()
        k, t = out[0, :n].tolist(), out[1, :n].tolist()
        assert sorted(zip(k, t)) == list(zip(k, t))
    out = torch.empty((3, 2), dtype=torch.int64)
    assert K.ijoin_merge(cols([]), cols([(5, 5, 5)]), out) == 1 and out[:, 0].tolist() == [5, 5, 5]
    with pytest.raises(ValueError):
        K.ijoin_merge(old, cols([(1, 1, 1)]), torch.empty((3, 5), dtype=torch.int64))


@pytest.mark.parametrize("wm,pairs", [(15, 0), (14, 1)])
def test_boundary_loss_left(wm, pairs):
    """l at ts 10 with hi = 5 is removed by watermark 15; r at ts 15 is not late then."""
    op = KeyedIntervalJoinOperator(lo=-2, hi=5)
    op.process(0, T([1]), T([10]), T([7]))
    op.advance_watermark(wm)
    got = op.process(1, T([1]), T([15]), T([8]))
    assert sum(c[0].numel() for c in got) == pairs
    assert op.metrics.num_late_records_dropped == 0
    if pairs:
        assert [c.tolist() for c in got[0]] == [[1], [7], [8], [15]]


@pytest.mark.parametrize("wm,pairs", [(12, 0), (11, 1)])
def test_boundary_loss_right(wm, pairs):
    """r at ts 10 with lo = -2 is removed by watermark 12."""
    op = KeyedIntervalJoinOperator(lo=-2, hi=5)
    op.process(1, T([1]), T([10]), T([8]))
    op.advance_watermark(wm)
    got = op.process(0, T([1]), T([12]), T([7]))
    assert sum(c[0].numel() for c in got) == pairs


def test_saturating_sums_at_the_int64_limits():
    far = cols([(7, I64_MIN + 1, 1), (7, -5, 2), (7, I64_MAX - 1, 3), (7, I64_MAX, 4)])
    batch = cols([(7, I64_MIN + 2, 9), (7, I64_MAX - 2, 10)])
    for lo, hi in [(-10, 10), (I64_MIN + 1, I64_MAX), (-(1 << 62), 1 << 62)]:
        for side in (0, 1):
            jp = K.ijoin_plan(side, batch, far, lo, hi)
            np.testing.assert_array_equal(expand(jp), brute(side, batch, far, lo, hi))
    assert K.ijoin_plan(0, batch, far, -10, 10).pairs == 3
    op = KeyedIntervalJoinOperator(lo=-5, hi=1 << 62)
    op.process(0, T([1]), T([I64_MAX - 3]), T([1]))
    op.advance_watermark(I64_MAX - 1)  # ts + hi saturates: only Long.MAX_VALUE removes the row
    assert op.buffered(0)[1].tolist() == [I64_MAX - 3]
    op.advance_watermark(I64_MAX)
    assert op.buffered(0)[1].size == 0


def test_bad_bounds_and_missing_timestamp_raise():
    with pytest.raises(ValueError, match="lowerBound <= upperBound must be fulfilled"):
        KeyedIntervalJoinOperator(lo=3 + 1, hi=4 - 1)
    op = KeyedIntervalJoinOperator(lo=0, hi=0)
    with pytest.raises(ValueError, match="timestamp"):
        op.process(0, T([1, 2]), T([5, I64_MIN]), T([0, 0]))
    with pytest.raises(ValueError):
        op.process(2, T([1]), T([5]), T([0]))
    with pytest.raises(TypeError):
        op.process(0, T([1]), T([5]).to(torch.int32), T([0]))


# ---- sizes ---------------------------------------------------------------------------------
_TILE_BOUNDS = (-1, 1)


@functools.lru_cache(maxsize=None)
def _tile_case():
    """P = 4096 + 1291 (odd): a first row of 4000 pairs, one of 200 that straddles the tile
    boundary, then 300 rows of 3 pairs and one of 287 (more than 256 rows in the second tile)."""
    other = [(0, 0, 10_000 + i) for i in range(4000)] + [(1, 0, 20_000 + i) for i in range(200)]
    other += [(2, t, 30_000 + t) for t in range(300)] + [(3, 0, 40_000 + i) for i in range(287)]
    batch = [(0, 0, 1), (1, 0, 2)] + [(2, 5, 100 + i) for i in range(300)] + [(3, 0, 3)]
    return cols(batch), cols(other)


def _plan_tiles(side=0, dev="cpu"):
    batch, other = (tuple(c.to(dev) for c in x) for x in _tile_case())
    return K.ijoin_plan(side, batch, other, *_TILE_BOUNDS)


def brute_fast(side, batch, other, lo, hi):
    """The nested loop per key with numpy (the sizes tests' reference)."""
    rlo, rhi = (lo, hi) if side == 0 else (-hi, -lo)
    bk, bt, bv = (c.numpy() for c in batch)
    ok, ot, ov = (c.numpy() for c in other)
    out = []
    for i in range(bk.size):
        sel = np.nonzero((ok == bk[i]) & (ot >= sat(int(bt[i]), rlo)) & (ot <= sat(int(bt[i]), rhi)))[0]
        l, r = (np.full(sel.size, bv[i]), ov[sel]) if side == 0 else (ov[sel], np.full(sel.size, bv[i]))
        out.append(np.stack([np.full(sel.size, bk[i]), l, r, np.maximum(bt[i], ot[sel])]))
    return np.concatenate(out, axis=1)


def test_tile_boundaries_and_chunked_expand_equal_one_launch():
    jp = _plan_tiles()
    assert jp.pairs == 4096 + 1291 and jp.pairs % 2 == 1 and jp.rows == 303
    assert jp.plan[:3].tolist() == [0, 4000, 4200]  # the second row straddles position 4096
    want = brute_fast(0, *_tile_case(), *_TILE_BOUNDS)
    np.testing.assert_array_equal(expand(jp), want)
    parts = [expand(jp, p0, min(jp.pairs, p0 + 4097)) for p0 in range(0, jp.pairs, 4097)]
    np.testing.assert_array_equal(np.concatenate(parts, axis=1), want)


@functools.lru_cache(maxsize=None)
def _hot_case():
    """One key, 70 000 buffered rows and 70 000 probing rows, all in range: P = 4.9e9."""
    n = 70_000
    z = np.zeros(n, np.int64)
    t = np.arange(n, dtype=np.int64) // 7
    batch = (T(z), T(t), T(np.arange(n) * 3 + 1))
    other = (T(z), T(t), T(np.arange(n) * 5 + 2))
    return batch, other


def _hot_range():
    return (1 << 32) - 5000, (1 << 32) + 5000


def _hot_expected(side, p0, p1):
    batch, other = _hot_case()
    n = 70_000
    p = np.arange(p0, p1, dtype=np.int64)
    i, o = p // n, p % n
    bv, ov = batch[2].numpy()[i], other[2].numpy()[o]
    ts = np.maximum(batch[1].numpy()[i], other[1].numpy()[o])
    return np.stack([np.zeros(p.size, np.int64), *((bv, ov) if side == 0 else (ov, bv)), ts])


def test_pairs_beyond_32_bits():
    batch, other = _hot_case()
    p0, p1 = _hot_range()
    for side in (0, 1):
        jp = K.ijoin_plan(side, batch, other, -20_000, 20_000)
        assert jp.pairs == 70_000 ** 2 > 1 << 32
        np.testing.assert_array_equal(expand(jp, p0, p1), _hot_expected(side, p0, p1))


@functools.lru_cache(maxsize=None)
def _carry_counts():
    """More than 4096 * 1024 elements: the tile scan's second round carries the first's total."""
    n = 4096 * 1024 + 4096 * 3 + 17
    rng = np.random.default_rng(3)
    cnt = rng.integers(0, 4, n).astype(np.int64)
    cnt[rng.random(n) < 0.5] = 0
    cnt[-1] = 1 << 40
    lb = rng.integers(0, 1 << 40, n).astype(np.int64)
    return cnt, lb


def _check_scan(cnt, lb, plan, pairs, rows):
    n = cnt.size
    ne = np.nonzero(cnt)[0]
    first = np.concatenate([[0], np.cumsum(cnt)])
    assert (pairs, rows) == (int(first[-1]), ne.size)
    plan = plan.cpu().numpy().reshape(3, n + 1)
    np.testing.assert_array_equal(plan[0, :rows + 1], np.concatenate([first[ne], first[-1:]]))
    np.testing.assert_array_equal(plan[1, :rows], ne)
    np.testing.assert_array_equal(plan[2, :rows], lb[ne])


def test_scan_carry_round_and_saturation_with_synthetic_counts():
    cnt, lb = _carry_counts()
    plan, pairs, rows, err = K.ijoin_scan(T(cnt), T(lb))
    assert err == 0
    _check_scan(cnt, lb, plan, pairs, rows)
    big = T([1 << 61, 0, 1 << 61, 5])
    plan, pairs, rows, err = K.ijoin_scan(big, T([0, 0, 0, 0]))
    assert (pairs, rows, err) == (1 << 62, 3, 1)


def test_2_62_pairs_are_refused_before_anything_is_expanded(monkeypatch):
    batch, other = cols([(1, 1, 1), (1, 2, 2)]), cols([(1, 1, 5)])
    real = K.ijoin_probe

    def probe(*a, **kw):
        lb, cnt = real(*a, **kw)
        return lb, torch.full_like(cnt, 1 << 61)

    monkeypatch.setattr(K, "ijoin_probe", probe)
    monkeypatch.setattr(K, "ijoin_expand", lambda *a, **kw: pytest.fail("expanded"))
    with pytest.raises(OverflowError, match="2\\*\\*62"):
        K.ijoin_plan(0, batch, other, 0, 0)
    op = KeyedIntervalJoinOperator(lo=0, hi=0)
    op.process(1, *other)
    with pytest.raises(OverflowError):
        op.process(0, *batch)


def test_purge_keeps_order():
    src = cols([(1, 10, 1), (1, 12, 2), (2, 5, 3), (2, 15, 4), (3, 11, 5)])
    out = torch.full((3, 6), -1, dtype=torch.int64)
    assert K.ijoin_purge(src, 10, out) == 3
    assert out[:, :3].tolist() == [[1, 2, 3], [12, 15, 11], [2, 4, 5]]
    assert K.ijoin_purge(src, I64_MAX, out) == 0 and K.ijoin_purge(src, I64_MIN, out) == 5


# ---- sanitizer -----------------------------------------------------------------------------
def test_sanitizer_harness_runs_clean():
    from mxstream.build import build_sanitize_ijoin

    res = subprocess.run([str(build_sanitize_ijoin())], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert res.stdout.strip().splitlines()[-1] == "ijoin sanitize ok"


# ---- GPU -----------------------------------------------------------------------------------
def _gpu_cols(c, dev):
    return tuple(x.to(dev) for x in c)


@pytest.mark.gpu
def test_gpu_kernels_equal_the_twin(gpu_device):
    dev = gpu_device
    rng = np.random.default_rng(11)
    cases = [(s, cols(random_rows(rng, 700, nkeys=9, tspan=40)),
              cols(random_rows(rng, 900, nkeys=9, tspan=40, base=5000)), lo, hi, cut)
             for s in (0, 1) for lo, hi in BOUNDS[:4] for cut in (I64_MIN, 7)]
    cases.append((0, *_tile_case(), *_TILE_BOUNDS, I64_MIN))
    cases.append((1, *_tile_case(), *_TILE_BOUNDS, I64_MIN))
    cases.append((0, cols([]), cols([(1, 1, 1)]), 0, 0, I64_MIN))
    cases.append((0, cols([(1, 1, 1)]), cols([]), 0, 0, I64_MIN))
    far = cols([(7, I64_MIN + 1, 1), (7, -5, 2), (7, I64_MAX - 1, 3), (7, I64_MAX, 4)])
    fb = cols([(7, I64_MIN + 2, 9), (7, I64_MAX - 2, 10)])
    cases += [(s, fb, far, I64_MIN + 1, I64_MAX, c) for s in (0, 1) for c in (I64_MIN, -6, I64_MAX)]
    for side, batch, other, lo, hi, cut in cases:
        cj = K.ijoin_plan(side, batch, other, lo, hi, cut)
        gj = K.ijoin_plan(side, _gpu_cols(batch, dev), _gpu_cols(other, dev), lo, hi, cut)
        assert (gj.pairs, gj.rows) == (cj.pairs, cj.rows)
        np.testing.assert_array_equal(gj.lb.cpu().numpy(), cj.lb.numpy())
        np.testing.assert_array_equal(gj.cnt.cpu().numpy(), cj.cnt.numpy())
        n = batch[0].numel()
        for c in range(3):
            w = cj.rows + (c == 0)
            np.testing.assert_array_equal(gj.plan[c * (n + 1):c * (n + 1) + w].cpu().numpy(),
                                          cj.plan[c * (n + 1):c * (n + 1) + w].numpy())
        want = expand(cj)
        np.testing.assert_array_equal(expand(gj), want)
        for chunk in (4097, 1000):
            if cj.pairs > chunk:
                parts = [expand(gj, p0, min(gj.pairs, p0 + chunk))
                         for p0 in range(0, gj.pairs, chunk)]
                np.testing.assert_array_equal(np.concatenate(parts, axis=1), want)
        # merge and purge on the same columns
        co = torch.empty((3, n + other[0].numel() + 1), dtype=torch.int64)
        go = torch.empty(co.shape, dtype=torch.int64, device=dev)
        rows = K.ijoin_merge(other, batch, co)
        assert K.ijoin_merge(_gpu_cols(other, dev), _gpu_cols(batch, dev), go) == rows
        np.testing.assert_array_equal(go[:, :rows].cpu().numpy(), co[:, :rows].numpy())
        for c in (cut, 3, I64_MAX):
            kept = K.ijoin_purge(other, c, co)
            assert K.ijoin_purge(_gpu_cols(other, dev), c, go) == kept
            np.testing.assert_array_equal(go[:, :kept].cpu().numpy(), co[:, :kept].numpy())


@pytest.mark.gpu
def test_gpu_pairs_beyond_32_bits_and_scan_carry(gpu_device):
    dev = gpu_device
    batch, other = (_gpu_cols(c, dev) for c in _hot_case())
    p0, p1 = _hot_range()
    for side in (0, 1):
        jp = K.ijoin_plan(side, batch, other, -20_000, 20_000)
        assert jp.pairs == 70_000 ** 2
        np.testing.assert_array_equal(expand(jp, p0, p1), _hot_expected(side, p0, p1))
    cnt, lb = _carry_counts()
    plan, pairs, rows, err = K.ijoin_scan(T(cnt, dev), T(lb, dev))
    assert err == 0
    _check_scan(cnt, lb, plan, pairs, rows)
    plan, pairs, rows, err = K.ijoin_scan(T([1 << 61, 0, 1 << 61, 5], dev), T([0] * 4, dev))
    assert (pairs, rows, err) == (1 << 62, 3, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("lo,hi", [(-3, 5), (2, 7), (0, 0), (0, 3), (-3, 0)])
def test_gpu_operator_equals_model(gpu_device, lo, hi):
    _engine_vs_model(lo, hi, dev=gpu_device, steps=20, seed=9, chunk=5, snapshot_at=11)


# ---- GPU: the scan's tile seams and the expand's ---------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ends", [0, 3], ids=["ends-empty", "ends-nonempty"])
@pytest.mark.parametrize("n", [1, 4095, 4096, 4097])
def test_gpu_scan_tile_seams_equal_the_twin(gpu_device, n, ends):
    rng = np.random.default_rng(n)
    cnt = rng.integers(0, 4, n).astype(np.int64) * (rng.random(n) < 0.5)
    cnt[0] = cnt[-1] = ends
    lb = rng.integers(0, 1 << 40, n).astype(np.int64)
    want = K.ijoin_scan(T(cnt), T(lb))
    got = K.ijoin_scan(T(cnt, gpu_device), T(lb, gpu_device))
    assert got[1:] == want[1:] and want[3] == 0
    _check_scan(cnt, lb, want[0], *want[1:3])
    _check_scan(cnt, lb, got[0], *got[1:3])


_SEAM_RANGES = [(0, 4097), (0, 1), (0, 2), (1, 2), (1, 3), (4095, 4096), (4095, 4097),
                (4096, 4097), (4097, 4098), (1, 4098), (4111, 8208), (4097, 8194), (0, 8208)]


@functools.lru_cache(maxsize=None)
def _seam_case():
    """A plan row of exactly one expand tile (4096 pairs), then one of 1 pair, three of 5 and
    another of 4096: P = 8208."""
    other = [(0, 0, 10_000 + i) for i in range(4096)] + [(1, 0, 20_000)]
    other += [(2, 0, 30_000 + i) for i in range(5)] + [(3, 0, 40_000 + i) for i in range(4096)]
    batch = [(0, 0, 1), (1, 0, 2)] + [(2, 0, 100 + i) for i in range(3)] + [(3, 0, 3)]
    return cols(batch), cols(other)


@pytest.mark.gpu
@pytest.mark.parametrize("side", [0, 1])
def test_gpu_expand_tile_seams_equal_the_twin(gpu_device, side):
    batch, other = _seam_case()
    cj = K.ijoin_plan(side, batch, other, 0, 0)
    assert cj.plan[:7].tolist() == [0, 4096, 4097, 4102, 4107, 4112, 8208]
    gj = K.ijoin_plan(side, _gpu_cols(batch, gpu_device), _gpu_cols(other, gpu_device), 0, 0)
    for p0, p1 in _SEAM_RANGES:  # lengths 1, 2 and 4097, even and odd starts, whole tiles
        np.testing.assert_array_equal(expand(gj, p0, p1), expand(cj, p0, p1), str((p0, p1)))
