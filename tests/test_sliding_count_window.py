"""Sliding count windows ``countWindow(size, slide)`` on the keyed rolling operator: the C++ twin
against a deque oracle, the gfx950 pane scan against the twin (exact equality), checkpoints and
the G-rank exchange."""
import functools
from collections import deque

import numpy as np
import pytest
import torch

from mxstream.ops import kernels as K
from mxstream.parallel.comm import run_loopback
from mxstream.runtime.rolling_operator import KeyedRollingOperator

# pane and window boundaries inside a 64-lane chunk, on its edge and across batches; more than
# ppw panes in one chunk ((64,1), (7,3)); a pane longer than a chunk ((130,65)); slide > size;
# slide == size; ppw = 64 twice ((64,1), (192,3)).
PAIRS = [(4, 2), (3, 5), (5, 5), (7, 3), (100, 10), (64, 1), (192, 3), (130, 65)]


def _gen(dev, n, nkeys, seed):
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    ts = torch.empty_like(keys)
    vals = torch.empty_like(keys)
    K.gen_events(keys, ts, vals, seed=seed, stream_id=0, idx0=0, nkeys=nkeys, ts_base=0,
                 ts_span=1000, disorder=0, val_lo=-500, val_span=1000)
    return keys, vals


def _per_key(rows, acc=None):
    """key -> [(value, element count)] in arrival order of the completing elements."""
    d = {} if acc is None else acc
    assert rows.counts is not None and len(rows.counts) == len(rows.keys)
    for i in np.argsort(rows.tags, kind="stable"):
        d.setdefault(int(rows.keys[i]), []).append((int(rows.values[i]), int(rows.counts[i])))
    return d


def _deque_oracle(batches, agg, size, slide):
    fn = {K.AGG_SUM_I64: sum, K.AGG_MIN_I64: min, K.AGG_MAX_I64: max, K.AGG_COUNT: len,
          K.AGG_AVG_I64: sum}[agg]  # avg rows carry (sum, count)
    win, seen, out = {}, {}, {}
    for keys, vals in batches:
        for k, v in zip(keys.tolist(), vals.tolist()):
            w = win.setdefault(k, deque(maxlen=size))
            w.append(v)
            seen[k] = seen.get(k, 0) + 1
            if seen[k] % slide == 0:
                out.setdefault(k, []).append((fn(w), len(w)))
    return out


# ---- 1. the twin against a pure-Python oracle -------------------------------------------------
@pytest.mark.parametrize("agg", [K.AGG_SUM_I64, K.AGG_MIN_I64, K.AGG_MAX_I64, K.AGG_COUNT,
                                 K.AGG_AVG_I64])
@pytest.mark.parametrize("size,slide", PAIRS)
def test_sliding_count_window_cpu_matches_oracle(agg, size, slide):
    batches = [_gen("cpu", 3000, 97, s) for s in range(4)]
    op = KeyedRollingOperator(agg=agg, device="cpu", max_keys=200, batch_capacity=3000,
                              cap_log2=8, count_window=size, count_slide=slide)
    got = {}
    for keys, vals in batches:
        _per_key(op.process(keys, vals), got)
    want = _deque_oracle(batches, agg, size, slide)
    assert got == want and len(want) > 0
    # the early windows of a key hold fewer than `size` elements
    assert all(c == min((i + 1) * slide, size) for seq in got.values()
               for i, (_, c) in enumerate(seq))
    if size == slide:  # the same rows as the tumbling countWindow(size)
        tum = KeyedRollingOperator(agg=agg, device="cpu", max_keys=200, batch_capacity=3000,
                                   cap_log2=8, count_window=size)
        ref = {}
        for keys, vals in batches:
            rows = tum.process(keys, vals)
            assert rows.counts is None
            for i in np.argsort(rows.tags, kind="stable"):
                ref.setdefault(int(rows.keys[i]), []).append(int(rows.values[i]))
        assert {k: [v for v, _ in seq] for k, seq in got.items()} == ref


def test_issue_examples_on_the_twin():
    keys = torch.zeros(11, dtype=torch.int64)
    vals = torch.arange(1, 12, dtype=torch.int64)
    for (size, slide), want in (((4, 2), [3, 10, 18, 26, 34]), ((3, 5), [12, 27])):
        op = KeyedRollingOperator(agg=K.AGG_SUM_I64, device="cpu", max_keys=8,
                                  count_window=size, count_slide=slide)
        assert [v for v, _ in _per_key(op.process(keys, vals))[0]] == want


# ---- 2. refusals ------------------------------------------------------------------------------
def test_sliding_count_window_refusals():
    mk = functools.partial(KeyedRollingOperator, agg=K.AGG_SUM_I64, device="cpu", max_keys=64)
    with pytest.raises(ValueError):
        mk(count_window=4, count_slide=2, spill=True)
    with pytest.raises(ValueError):
        mk(count_window=4, count_slide=2, dense_keys=True)
    with pytest.raises(ValueError):
        mk(count_window=65, count_slide=1)  # 65 panes per window
    with pytest.raises(ValueError):
        mk(count_slide=2)  # a slide without a window
    mk(count_window=64, count_slide=1)
    mk(count_window=192, count_slide=3)
    assert mk(count_window=4).count_slide == 0  # the default is the tumbling mode


# ---- 3. / 9. checkpoints -----------------------------------------------------------------------
def _checkpoint_case(dev_run, dev_restore, size, slide, agg=K.AGG_SUM_I64):
    def mk(d):
        return KeyedRollingOperator(agg=agg, device=d, max_keys=200, batch_capacity=3000,
                                    count_window=size, count_slide=slide)

    batches = [_gen("cpu", 3000, 97, s) for s in range(4)]
    def on(d, b):
        return b[0].to(d), b[1].to(d)

    whole = mk(dev_run)
    ref = [_per_key(whole.process(*on(dev_run, b))) for b in batches]
    first = mk(dev_run)
    for b in batches[:2]:
        first.process(*on(dev_run, b))
    snap = first.snapshot_state()
    assert snap.meta["count_slide"] == slide and "ord" in snap.columns
    # open panes (where a pane has more than one element) and partly filled rings
    pane = int(np.gcd(size, slide))
    assert pane == 1 or (snap.columns["ord"] % pane != 0).any()
    assert (snap.columns["ord"] // pane < size // pane).any()
    for d in dev_restore:
        op = mk(d)
        op.restore_state(snap.columns, snap.meta)
        for b, want in zip(batches[2:], ref[2:]):
            assert _per_key(op.process(*on(d, b))) == want
    return snap


@pytest.mark.parametrize("size,slide", [(100, 10), (192, 3), (64, 1)])
def test_sliding_count_window_checkpoint_cpu(size, slide):
    cpu = torch.device("cpu")
    _checkpoint_case(cpu, [cpu], size, slide)


def test_sliding_restore_refuses_other_shapes():
    keys, vals = _gen("cpu", 500, 20, 0)
    mk = functools.partial(KeyedRollingOperator, agg=K.AGG_SUM_I64, device="cpu", max_keys=64)
    tum = mk(count_window=4)
    tum.process(keys, vals)
    snap = tum.snapshot_state()
    assert "count_slide" not in snap.meta  # tumbling checkpoints keep their format
    with pytest.raises(ValueError):
        mk(count_window=4, count_slide=2).restore_state(snap.columns, snap.meta)
    sl = mk(count_window=4, count_slide=2)
    sl.process(keys, vals)
    s2 = sl.snapshot_state()
    for other in (mk(count_window=4), mk(count_window=4, count_slide=4),
                  mk(count_window=6, count_slide=2)):
        with pytest.raises(ValueError):
            other.restore_state(s2.columns, s2.meta)
    mk(count_window=4).restore_state(snap.columns, snap.meta)  # as before


@pytest.mark.gpu
@pytest.mark.parametrize("size,slide", [(100, 10), (64, 1)])
def test_sliding_count_window_checkpoint_gpu(gpu_device, size, slide):
    _checkpoint_case(gpu_device, [gpu_device, torch.device("cpu")], size, slide)


# ---- 4. / 10. G ranks through the exchange -----------------------------------------------------
def _rank_batch(dev, rank, step, per, nkeys):
    d = torch.device(dev)
    keys = torch.empty(per, dtype=torch.int64, device=d)
    ts = torch.empty_like(keys)
    vals = torch.empty_like(keys)
    K.gen_events(keys, ts, vals, seed=11, stream_id=rank, idx0=step * per, nkeys=nkeys,
                 ts_base=0, ts_span=1000, disorder=0, val_lo=0, val_span=1000)
    return keys, vals


def _loopback_case(dev, world, per, nkeys):
    size, slide = 6, 4

    def rank_fn(comm):
        op = KeyedRollingOperator(agg=K.AGG_SUM_I64, device=dev, comm=comm, max_keys=nkeys,
                                  parallelism=comm.world, batch_capacity=per,
                                  count_window=size, count_slide=slide)
        got = {}
        for step in range(4):
            _per_key(op.process(*_rank_batch(dev, comm.rank, step, per, nkeys)), got)
        return got

    merged = {}
    for g in run_loopback(world, rank_fn, device=torch.device(dev)):
        for k, seq in g.items():
            assert k not in merged  # one owner per key
            merged[k] = seq
    ref_op = KeyedRollingOperator(agg=K.AGG_SUM_I64, device=dev, max_keys=nkeys,
                                  batch_capacity=per * world, count_window=size,
                                  count_slide=slide)
    ref = {}
    for step in range(4):
        parts = [_rank_batch(dev, r, step, per, nkeys) for r in range(world)]
        _per_key(ref_op.process(torch.cat([p[0] for p in parts]),
                                torch.cat([p[1] for p in parts])), ref)
    assert merged == ref and len(ref) > 0


@pytest.mark.parametrize("world", [2, 4])
def test_sliding_count_window_invariant_to_world_cpu(world):
    _loopback_case("cpu", world, 4000, 700)


@pytest.mark.gpu
def test_sliding_count_window_invariant_to_world_gpu(gpu_device):
    _loopback_case("cuda", 2, 20_000, 5000)


# ---- 7. the gfx950 pane scan against the twin, exact -------------------------------------------
_FLOAT = (K.AGG_MAX_F64, K.AGG_SUM_F64)


@functools.lru_cache(maxsize=None)
def _gpu_case_batches(is_float):
    """3 batches of 2^15 records over 300 keys. Float values are k / 8 with |k| <= 2^20: every
    sum of at most 192 of them is exact in a double, so the comparison is bitwise whatever the
    association."""
    g = torch.Generator().manual_seed(1234)
    out = []
    for _ in range(3):
        keys = torch.randint(0, 300, (1 << 15,), generator=g, dtype=torch.int64)
        k = torch.randint(-(1 << 20), (1 << 20) + 1, (1 << 15,), generator=g, dtype=torch.int64)
        out.append((keys, (k.to(torch.float64) / 8).view(torch.int64) if is_float else k))
    return out


def _sorted_rows(rows):
    o = np.argsort(rows.tags, kind="stable")
    return rows.keys[o], rows.values[o], rows.tags[o], rows.counts[o]


@functools.lru_cache(maxsize=None)
def _twin_rows(agg, size, slide):
    op = KeyedRollingOperator(agg=agg, device="cpu", max_keys=300, batch_capacity=1 << 15,
                              count_window=size, count_slide=slide)
    return [_sorted_rows(op.process(k, v)) for k, v in _gpu_case_batches(agg in _FLOAT)]


@pytest.mark.gpu
@pytest.mark.parametrize("direct", [True, False])
@pytest.mark.parametrize("agg", [K.AGG_SUM_I64, K.AGG_MIN_I64, K.AGG_AVG_I64, K.AGG_COUNT,
                                 K.AGG_MAX_F64, K.AGG_SUM_F64])
@pytest.mark.parametrize("size,slide", PAIRS)
def test_sliding_count_window_gpu_equals_twin(gpu_device, size, slide, agg, direct):
    op = KeyedRollingOperator(agg=agg, device=gpu_device, max_keys=300, batch_capacity=1 << 15,
                              count_window=size, count_slide=slide)
    op.direct_single_rank = direct
    total = 0
    for (k, v), want in zip(_gpu_case_batches(agg in _FLOAT), _twin_rows(agg, size, slide)):
        got = _sorted_rows(op.process(k.to(gpu_device), v.to(gpu_device)))
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
        total += len(got[0])
    assert total > 0


# ---- 8. a hot key, then long-lived state -------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("size,slide", [(100, 10), (64, 1)])
def test_sliding_count_window_hot_key_and_long_lived_state(gpu_device, size, slide):
    g = torch.Generator().manual_seed(99)
    hot = torch.cat([torch.zeros(5000, dtype=torch.int64),
                     torch.randint(1, 201, (8192 - 5000,), generator=g, dtype=torch.int64)])
    hot = hot[torch.randperm(8192, generator=g)]
    batches = [(hot, torch.randint(-500, 500, (8192,), generator=g, dtype=torch.int64))]
    for _ in range(20):  # one element per key and batch
        batches.append((torch.randperm(256, generator=g),
                        torch.randint(-500, 500, (256,), generator=g, dtype=torch.int64)))
    res = {}
    for d in (gpu_device, torch.device("cpu")):
        op = KeyedRollingOperator(agg=K.AGG_SUM_I64, device=d, max_keys=300, batch_capacity=8192,
                                  count_window=size, count_slide=slide)
        res[d.type] = [_sorted_rows(op.process(k.to(d), v.to(d))) for k, v in batches]
    for got, want in zip(res["cuda"], res["cpu"]):
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
    assert sum(len(r[0]) for r in res["cpu"][1:]) > 0  # the small batches fire too
