"""The arg-select scan behind ``maxBy`` / ``minBy`` (KeyedRollingOperator with ``arg_select``):
the C++ twin ``rolling_arg_rows`` against a pure-Python left fold with the strict compare, and
the gfx950 kernel ``rolling_argscan_kernel`` against the twin, bit-equal on every output column
(rows sorted by tag, per-key winners sorted by key) and on the keyed state."""
import functools

import numpy as np
import pytest
import torch
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

from mxstream.ops import expr as E
from mxstream.ops import kernels as K
from mxstream.ops.native import load
from mxstream.runtime.rolling_operator import KeyedRollingOperator

AGGS = [K.AGG_MAX_I64, K.AGG_MIN_I64, K.AGG_MAX_F64, K.AGG_MIN_F64]
_FLOAT = (K.AGG_MAX_F64, K.AGG_MIN_F64)
_MAX = (K.AGG_MAX_I64, K.AGG_MAX_F64)
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def _bits(values, is_float):
    """Value words of a batch: int64, or the bit patterns of float64."""
    a = np.asarray(values, dtype=np.float64 if is_float else np.int64)
    return torch.from_numpy(a.view(np.int64).copy())


def _batch(keys, values, is_float):
    return torch.tensor(list(keys), dtype=torch.int64), _bits(list(values), is_float)


# ---- the definition: a left fold per key in arrival order, strict compare ---------------------
def _fold(batches, agg, cw):
    """Per batch: rows {tag: (key, value word, winner (batch, index))}, winners {key: (batch,
    index) or None (empty window)}; and the final state {key: (value word, count)}."""
    is_float, is_max = agg in _FLOAT, agg in _MAX
    state = {}  # key -> [value word, winner, count]
    out = []
    for b, (keys, vals) in enumerate(batches):
        rows, touched = {}, set()
        words = vals.tolist()
        nums = vals.numpy().view(np.float64).tolist() if is_float else words
        for i, k in enumerate(keys.tolist()):
            s = state.setdefault(k, [0, None, 0])
            touched.add(k)
            if s[2] == 0:
                s[0], s[1], s[3:] = words[i], (b, i), [nums[i]]
            elif (nums[i] > s[3]) if is_max else (nums[i] < s[3]):  # strictly better only
                s[0], s[1], s[3:] = words[i], (b, i), [nums[i]]
            s[2] += 1
            if not cw or s[2] == cw:
                rows[i] = (k, s[0], s[1])
            if cw and s[2] == cw:
                s[1], s[2] = None, 0
        out.append((rows, {k: state[k][1] for k in touched}))
    return out, {k: (s[0], s[2]) for k, s in state.items()}


def _mk(agg, dev, cw, direct=True):
    op = KeyedRollingOperator(agg=agg, device=dev, max_keys=300, batch_capacity=1024,
                              count_window=cw, arg_select=True)
    op.direct_single_rank = direct
    return op


def _state(op):
    keys = op.keys_g.cpu().numpy()
    live = np.nonzero(keys != -1)[0]
    acc, cnt = op.acc_g.cpu().numpy(), op.cnt_g.cpu().numpy()
    return {int(keys[i]): (int(acc[i]), int(cnt[i])) for i in live}


def _sorted(rows):
    o = np.argsort(rows.tags, kind="stable")
    w = np.argsort(rows.win_keys, kind="stable")
    assert rows.counts is None and len(rows.srcs) == len(rows.keys)
    return (rows.keys[o], rows.values[o], rows.tags[o], rows.srcs[o],
            rows.win_keys[w], rows.win_srcs[w])


def _run(op, batches):
    dev = op.device
    return [_sorted(op.process(k.to(dev), v.to(dev))) for k, v in batches], _state(op)


def _check_against_fold(batches, agg, cw, got, state):
    want, want_state = _fold(batches, agg, cw)
    stored = {}  # key -> (batch, index) of the row an operator would hold: resolves src == -1
    for b, ((keys, vals, tags, srcs, wkeys, wsrcs), (rows, wins)) in enumerate(zip(got, want)):
        assert tags.tolist() == sorted(rows)
        for k, v, t, s in zip(keys.tolist(), vals.tolist(), tags.tolist(), srcs.tolist()):
            wk, wv, wrec = rows[t]
            assert (k, v) == (wk, wv)
            assert s >= -1 and (s == -1) == (wrec[0] < b)  # -1: the record held in state
            assert (stored[k] if s == -1 else (b, s)) == wrec
        assert sorted(wkeys.tolist()) == sorted(wins)
        for k, s in zip(wkeys.tolist(), wsrcs.tolist()):
            if s >= 0:
                stored[k] = (b, s)
            elif s == -2:
                assert cw
                stored.pop(k, None)
            else:
                assert s == -1
            assert stored.get(k) == wins[k]
    # (a closed window leaves its last value in acc_g: only the count says it is empty)
    assert {k: c for k, (_, c) in state.items()} == {k: c for k, (_, c) in want_state.items()}
    assert all(state[k][0] == a for k, (a, c) in want_state.items() if c)


# ---- 1. the twin against the fold (Hypothesis: ties nearly everywhere) ------------------------
@settings(max_examples=120, deadline=None, suppress_health_check=list(HealthCheck))
@given(events=st.lists(st.tuples(st.integers(0, 3), st.integers(0, 3)), min_size=1, max_size=60),
       cuts=st.lists(st.integers(0, 60), min_size=0, max_size=2),
       cw=st.sampled_from([0, 1, 2, 3, 5]), agg=st.sampled_from(AGGS))
def test_arg_rows_twin_matches_left_fold(events, cuts, cw, agg):
    is_float = agg in _FLOAT
    edges = [0] + sorted(min(c, len(events)) for c in cuts) + [len(events)]
    batches = [_batch([k for k, _ in events[a:b]], [v for _, v in events[a:b]], is_float)
               for a, b in zip(edges, edges[1:])]
    got, state = _run(_mk(agg, "cpu", cw), batches)
    _check_against_fold(batches, agg, cw, got, state)


# ---- 2. the shapes that can break the wave scan ------------------------------------------------
def _segments_case(seed, is_float):
    """~200 keys with segment lengths 1..150 per batch, values in 0..3, three batches."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for b in range(3):
        lens = [1 + (j * 37 + b * 11) % 150 for j in range(200)]
        keys = torch.repeat_interleave(torch.arange(200, dtype=torch.int64) * 7 + 1,
                                       torch.tensor(lens))
        keys = keys[torch.randperm(keys.numel(), generator=g)]
        vals = torch.randint(0, 4, (keys.numel(),), generator=g, dtype=torch.int64)
        out.append((keys, _bits(vals.tolist(), is_float)))
    return out


def _window_case(cw, is_float):
    """Count windows straddling chunk and batch boundaries. Key 0 ends batch 1 exactly on a
    window end (win_src == -2), key 1 one past it, key 2 one short of it; key 3 sees a single
    record per batch; the rest are random."""
    g = torch.Generator().manual_seed(cw)
    out = []
    for b in range(3):
        lens = [2 * cw, cw + 1 + b, max(1, cw - 1), 1] + [1 + (j * 29 + b) % 140 for j in range(6)]
        keys = torch.repeat_interleave(torch.arange(len(lens), dtype=torch.int64),
                                       torch.tensor(lens))
        keys = keys[torch.randperm(keys.numel(), generator=g)]
        vals = torch.randint(0, 4, (keys.numel(),), generator=g, dtype=torch.int64)
        out.append((keys, _bits(vals.tolist(), is_float)))
    return out


_F_SPECIAL = [0.0, -0.0, float("inf"), -0.0, 0.0, float("-inf"), 1.5, float("inf"), -1.5,
              float("-inf"), 0.0]
_I_SPECIAL = [0, I64_MAX, I64_MIN, -1, I64_MAX, 1, I64_MIN, 0]


@functools.lru_cache(maxsize=None)
def _case(name, agg):
    """(count window, batches) of a named case."""
    f = agg in _FLOAT
    one = lambda vals: _batch([5] * len(vals), vals, f)  # noqa: E731
    if name == "all_equal_130":
        return 0, [one([2] * 130), one([2] * 130)]
    if name == "increasing_64_65":
        return 0, [one(range(64)), one(range(64, 129)), one(range(129, 194))]
    if name == "decreasing_64_65":
        return 0, [one(range(200, 136, -1)), one(range(136, 71, -1))]
    if name == "second_batch_worse":
        lo, hi = (0, 100) if agg in _MAX else (100, 0)
        return 0, [one([lo, hi, lo]), one([lo] * 70 + [hi])]  # (a tie with the state: still -1)
    if name == "segments":
        return 0, _segments_case(3, f)
    if name == "one_record":
        return 0, [one([7]), one([7]), one([8]), one([6])]
    if name == "one_record_window":
        return 3, [one([7]), one([7]), one([8]), one([6]), one([9])]
    if name == "specials":
        sp = _F_SPECIAL if f else _I_SPECIAL
        keys = [k for k in range(3) for _ in sp]
        return 0, [_batch(keys, sp * 3, f), _batch(keys[::-1], (sp * 3)[::-1], f)]
    if name == "specials_window":
        sp = _F_SPECIAL if f else _I_SPECIAL
        return 3, [_batch([1] * len(sp), sp, f), _batch([1] * len(sp), sp[::-1], f)]
    assert name.startswith("window_")
    cw = int(name[7:])
    return cw, _window_case(cw, f)


CASES = ["all_equal_130", "increasing_64_65", "decreasing_64_65", "second_batch_worse",
         "segments", "one_record", "one_record_window", "specials", "specials_window",
         "window_1", "window_3", "window_64", "window_65", "window_100"]


@functools.lru_cache(maxsize=None)
def _twin(name, agg):
    cw, batches = _case(name, agg)
    return _run(_mk(agg, "cpu", cw), batches)


@pytest.mark.parametrize("agg", AGGS)
@pytest.mark.parametrize("name", CASES)
def test_arg_rows_twin_cases_match_left_fold(name, agg):
    cw, batches = _case(name, agg)
    got, state = _twin(name, agg)
    _check_against_fold(batches, agg, cw, got, state)


def _expectations(name, agg, got):
    """What the named cases must show, whoever computed `got`."""
    srcs = [g[3] for g in got]
    if name == "all_equal_130":  # every tie keeps the first element, then the stored record
        assert (srcs[0] == 0).all() and (srcs[1] == -1).all() and len(srcs[1]) == 130
    if name in ("increasing_64_65", "decreasing_64_65"):
        best = (agg in _MAX) == (name == "increasing_64_65")  # every element is a new winner
        assert (srcs[0] == (got[0][2] if best else 0)).all()
        assert (srcs[1] == (got[1][2] if best else -1)).all() and len(srcs[1]) == 65
    if name == "second_batch_worse":
        assert (srcs[1] == -1).all() and len(srcs[1]) == 71 and (got[1][5] == -1).all()
    if name.startswith("window_"):
        assert any((g[5] == -2).any() for g in got)  # a batch that ends on a window end
        if name == "window_1":  # every element closes its own window: nothing is ever held
            assert all((g[5] == -2).all() and (g[3] == g[2]).all() for g in got)
        else:
            assert any((g[5] >= 0).any() for g in got) and any((g[3] == -1).any() for g in got)
    if name == "one_record_window":
        # windows (7, 7, 8) and (6, 9, ...): the tie keeps the first 7; 9 beats 6 only for max
        assert [g[5].tolist() for g in got] == [[0], [-1], [-2], [0], [0 if agg in _MAX else -1]]
        assert [g[3].tolist() for g in got] == ([[], [], [0], [], []] if agg in _MAX
                                                else [[], [], [-1], [], []])


@pytest.mark.parametrize("agg", AGGS)
@pytest.mark.parametrize("name", CASES)
def test_arg_rows_twin_case_expectations(name, agg):
    _expectations(name, agg, _twin(name, agg)[0])


# ---- 3. refusals, checkpoints ------------------------------------------------------------------
def test_arg_select_refusals():
    mk = functools.partial(KeyedRollingOperator, device="cpu", max_keys=64, arg_select=True)
    for agg in (K.AGG_SUM_I64, K.AGG_SUM_F64, K.AGG_COUNT, K.AGG_AVG_I64):
        with pytest.raises(ValueError):
            mk(agg=agg, count_window=4)
    with pytest.raises(ValueError):
        mk(agg=K.AGG_MAX_I64, spill=True)
    with pytest.raises(ValueError):
        mk(agg=K.AGG_MAX_I64, dense_keys=True)
    with pytest.raises(ValueError):
        mk(agg=K.AGG_MAX_I64, count_window=4, count_slide=2)
    with pytest.raises(ValueError):
        mk(agg=K.AGG_MAX_I64, filter_prog=E.compile_expr(E.var(0) > 1.0))
    for agg in AGGS:
        op = mk(agg=agg)
        assert op.arg_select and not op.sort_free
        assert mk(agg=agg, count_window=4).count_window == 4
    assert not KeyedRollingOperator(agg=K.AGG_MAX_I64, device="cpu", max_keys=64).arg_select


def test_arg_bindings_refuse_other_aggregates():
    m = load()
    z = torch.zeros(64, dtype=torch.int64)
    with pytest.raises(Exception):
        m.cpu_rolling_arg_rows(z.data_ptr(), z.data_ptr(), 1, 1, 8, 4, K.AGG_SUM_I64, z.data_ptr(),
                               z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(),
                               z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), 8,
                               z.data_ptr(), z.data_ptr(), z.data_ptr(), 0)
    assert hasattr(m, "gpu_rolling_argscan")


@pytest.mark.parametrize("cw", [0, 3])
def test_arg_select_checkpoint_records_the_mode(cw):
    cwn, batches = _case("segments", K.AGG_MAX_I64)
    whole = _mk(K.AGG_MAX_I64, "cpu", cw)
    ref, _ = _run(whole, batches)
    first = _mk(K.AGG_MAX_I64, "cpu", cw)
    _run(first, batches[:2])
    snap = first.snapshot_state()
    assert snap.meta["arg_select"] is True
    op = _mk(K.AGG_MAX_I64, "cpu", cw)
    op.restore_state(snap.columns, snap.meta)
    got, state = _run(op, batches[2:])
    for a, b in zip(got[0], ref[2]):
        assert np.array_equal(a, b)
    assert state == _state(whole)
    plain = KeyedRollingOperator(agg=K.AGG_MAX_I64, device="cpu", max_keys=300, count_window=cw)
    with pytest.raises(ValueError):
        plain.restore_state(snap.columns, snap.meta)
    psnap = plain.snapshot_state()
    assert "arg_select" not in psnap.meta
    with pytest.raises(ValueError):
        _mk(K.AGG_MAX_I64, "cpu", cw).restore_state(psnap.columns, psnap.meta)


# ---- 4. the kernel against the twin -----------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("direct", [True, False])
@pytest.mark.parametrize("agg", AGGS)
@pytest.mark.parametrize("name", CASES)
def test_argscan_gpu_equals_twin(gpu_device, name, agg, direct):
    cw, batches = _case(name, agg)
    want, want_state = _twin(name, agg)
    got, state = _run(_mk(agg, gpu_device, cw, direct), batches)
    for g, w in zip(got, want):
        for a, b in zip(g, w):
            assert a.dtype == b.dtype and np.array_equal(a, b)
    assert state == want_state
    _expectations(name, agg, got)


@pytest.mark.gpu
def test_argscan_gpu_rows_stay_on_device(gpu_device):
    cw, batches = _case("segments", K.AGG_MIN_I64)
    want, _ = _twin("segments", K.AGG_MIN_I64)
    op = _mk(K.AGG_MIN_I64, gpu_device, cw)
    k, v = batches[0]
    out_n = op.process(k.to(gpu_device), v.to(gpu_device), to_host=False)
    n = op.check()
    assert int(out_n.item()) == n == len(want[0][0])
    nw = int(op.win_n.item())
    assert op.out_src.is_cuda and op.win_src.is_cuda and nw == len(want[0][4])
    o = torch.argsort(op.out_tag[:n])
    assert np.array_equal(op.out_src[:n][o].cpu().numpy(), want[0][3])
    w = torch.argsort(op.win_key[:nw])
    assert np.array_equal(op.win_src[:nw][w].cpu().numpy(), want[0][5])


# ---- 5. G ranks through the exchange: tags with source bits (abits < shift) --------------------
_PER, _NKEYS = 3000, 97


def _rank_batch(rank, step):
    g = torch.Generator().manual_seed(1000 * step + rank)
    return (torch.randint(0, _NKEYS, (_PER,), generator=g, dtype=torch.int64),
            # (a later rank reaches higher: winners come from every source, not only rank 0)
            torch.randint(0, 4, (_PER,), generator=g, dtype=torch.int64) + rank)


def _flat(tag, per):
    """src << 32 | arrival -> the record's index in the ranks' batches laid end to end."""
    return np.where(tag >= 0, (tag >> 32) * per + (tag & 0xFFFFFFFF), tag)


def _keyed_rows(rows, per, acc):
    o = np.argsort(_flat(rows.tags, per), kind="stable")
    for k, v, t, s in zip(rows.keys[o].tolist(), rows.values[o].tolist(),
                          _flat(rows.tags[o], per).tolist(), _flat(rows.srcs[o], per).tolist()):
        acc.setdefault(k, []).append((v, t, s))
    for k, s in zip(rows.win_keys.tolist(), _flat(rows.win_srcs, per).tolist()):
        acc.setdefault(("win", k), []).append(s)


@functools.lru_cache(maxsize=None)
def _world_reference(world, cw):
    op = KeyedRollingOperator(agg=K.AGG_MAX_I64, device="cpu", max_keys=300,
                              batch_capacity=_PER * world, count_window=cw, arg_select=True)
    ref = {}
    for step in range(3):
        parts = [_rank_batch(r, step) for r in range(world)]
        _keyed_rows(op.process(torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])),
                    1 << 32, ref)  # one source: tags are the flat indices already
    return ref


def _loopback_case(dev, world, cw):
    from mxstream.parallel.comm import run_loopback

    def rank_fn(comm):
        op = KeyedRollingOperator(agg=K.AGG_MAX_I64, device=dev, comm=comm, max_keys=300,
                                  parallelism=comm.world, batch_capacity=_PER, count_window=cw,
                                  arg_select=True)
        got = {}
        for step in range(3):
            k, v = _rank_batch(comm.rank, step)
            _keyed_rows(op.process(k.to(dev), v.to(dev)), _PER, got)
        return got

    merged = {}
    for g in run_loopback(world, rank_fn, device=torch.device(dev)):
        assert not set(g) & set(merged)  # one owner per key
        merged.update(g)
    ref = _world_reference(world, cw)
    assert merged == ref and len(ref) > _NKEYS
    # winners from every source rank, not only the first
    assert any(s >= _PER for k, seq in ref.items() if isinstance(k, int) for _, _, s in seq)


@pytest.mark.parametrize("cw", [0, 5])
@pytest.mark.parametrize("world", [2, 4])
def test_arg_select_invariant_to_world_cpu(world, cw):
    _loopback_case("cpu", world, cw)


@pytest.mark.gpu
@pytest.mark.parametrize("cw", [0, 5])
def test_arg_select_invariant_to_world_gpu(gpu_device, cw):
    _loopback_case("cuda", 2, cw)
