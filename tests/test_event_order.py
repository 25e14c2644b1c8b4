"""The event-time reorder buffer (csrc/mxs_reorder.h): the engine (runtime/reorder_operator.py)
over the C++ twins against a plain Python list of (ts, seq, key, bits), and the gfx950 kernels
against the twins array for array. Everything is an integer or a bit pattern and compares exactly,
row for row and in order."""
from __future__ import annotations

import functools
import subprocess

import numpy as np
import pytest
import torch

from mxstream.ops import kernels as K
from mxstream.runtime.reorder_operator import EventOrderBuffer

LIM = K.SUSTAIN_TS_LIMIT
SEEDS = [0, 1]


def T(a, dev="cpu") -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev)


class Model:
    """The buffer as a list: release is the rows with ts <= W sorted by (ts, seq); late is
    ts <= wm on arrival. A row remembers the batch it came in."""

    def __init__(self):
        self.rows, self.wm, self.seq, self.late, self.batch = [], K.I64_MIN, 0, 0, 0
        self.max_batches = 0    # the most batches that fed one release
        self.cross_ties = 0     # released neighbours of one timestamp from two batches

    def push(self, keys, ts, bits):
        for k, t, b in zip(*(np.asarray(x).tolist() for x in (keys, ts, bits))):
            if t <= self.wm:
                self.late += 1
            else:
                self.rows.append((t, self.seq, k, b, self.batch))
            self.seq += 1
        self.batch += 1

    def release(self, w) -> list:
        """Rows (key, ts, bits) in (ts, seq) order."""
        if w <= self.wm:
            return []
        self.wm = w
        due = sorted(r for r in self.rows if r[0] <= w)
        self.rows = [r for r in self.rows if r[0] > w]
        self.max_batches = max(self.max_batches, len({r[4] for r in due}))
        self.cross_ties += sum(a[0] == b[0] and a[4] != b[4] for a, b in zip(due, due[1:]))
        return [(k, t, b) for t, _, k, b, _ in due]

    def contents(self) -> list:
        return [(k, t, b) for t, _, k, b, _ in sorted(self.rows)]


def _tuples(cols) -> list:
    return [] if cols is None else list(zip(*(c.cpu().tolist() for c in cols)))


def _run(calls, dev="cpu", snapshot_at=None, seed=0, **kw):
    """The calls ("p", keys, ts, bits) / ("w", W) on a buffer: per call the released rows (None
    for a push), and a trace of what the engine did -- the chunks that fed each release, the
    arena-order rows after every push, capacity and consolidations."""
    buf = EventOrderBuffer(dev, **kw)
    out, trace = [], []
    for i, c in enumerate(calls):
        if i == snapshot_at:
            snap = buf.snapshot_state()
            assert snap.meta["kind"] == "reorder" and snap.meta["wm"] == buf.wm
            assert snap.meta["late"] == buf.metrics.num_late_records_dropped
            assert set(snap.columns) == {"key", "ts", "bits", "ord"}
            assert snap.columns["ord"].tolist() == list(range(buf.rows_buffered))
            assert snap.kg.size == buf.rows_buffered
            # key groups come back in any order
            o = np.random.default_rng(seed).permutation(buf.rows_buffered)
            late = buf.metrics.num_late_records_dropped
            buf = EventOrderBuffer(dev, **kw)
            buf.restore_state({k: v[o] for k, v in snap.columns.items()}, snap.meta)
            assert buf.metrics.num_late_records_dropped == late and len(buf.chunks) <= 1
        if c[0] == "w":
            got = buf.release(c[1])
            assert got is None or (len(got) == 3 and got[0].numel() > 0)
            out.append(_tuples(got))
            trace.append(("w", buf.last_contrib))
        else:
            buf.push(*(T(x, dev) for x in c[1:]))
            out.append(None)
            trace.append(("p", [x.tolist() for x in buf.rows()], buf.cap, buf.consolidations,
                          [list(ch) for ch in buf.chunks]))
    return buf, out, trace


def _model(calls):
    m, out = Model(), []
    for c in calls:
        out.append(m.release(c[1]) if c[0] == "w" else m.push(*c[1:]))
    return m, out


def _agrees(buf, out, calls):
    m, want = _model(calls)
    assert out == want
    assert _tuples([torch.from_numpy(x) for x in buf.contents()]) == m.contents()
    assert buf.metrics.num_late_records_dropped == m.late
    assert buf.rows_buffered == len(m.rows)
    assert buf.metrics.num_records_in == m.seq
    assert buf.metrics.num_records_out == sum(len(o) for o in want if o)
    return m


# ---- hand-built call lists: every path of the engine ---------------------------------------------
def _batch(rng, n, t0, t1, nkeys=50):
    return ("p", rng.integers(0, nkeys, n), rng.integers(t0, t1, n),
            rng.integers(K.I64_MIN, K.I64_MAX, n))


def _hand_cases():
    """name -> (calls, buffer keywords)."""
    c = {}
    rng = np.random.default_rng(5)
    # chunks of every length around the wave and the collect's tile, one timestamp range: every
    # release draws on all of them
    calls = [_batch(rng, n, 1000, 1100) for n in (0, 1, 63, 64, 65, 4095, 4096, 4097, 8193)]
    calls += [("w", w) for w in (999, 1000, 1009, 1029, 1029, 1000, 1030, 1098)]
    calls += [_batch(rng, 4097, 1090, 1200), ("w", 1150), ("w", K.I64_MAX), ("w", K.I64_MAX)]
    c["chunk_lengths"] = (calls, {})
    # release totals on both sides of the collect's 4096-position tile, from two chunks
    for total in (4095, 4096, 4097, 8191, 8192, 8193):
        a, b = np.arange(5000) * 2, np.arange(5000) * 2 + 1
        c[f"release_total_{total}"] = (
            [("p", a % 7, a, a + 1), ("p", b % 7, b, -b), ("w", total - 1), ("w", K.I64_MAX)], {})
    # 1 contributing chunk (the slice path), 2, 3; then more than max_chunks: consolidation
    calls = [("p", [1, 1, 1], [10, 50, 90], [1, 2, 3]), ("p", [2, 2, 2], [40, 60, 95], [4, 5, 6]),
             ("p", [3, 3, 3], [70, 80, 99], [7, 8, 9]), ("w", 10), ("w", 55), ("w", 92)]
    calls += [("p", [4 + i], [100 + 10 * (i % 2) - i], [i]) for i in range(6)]
    calls += [("w", 96), ("w", 104), ("w", K.I64_MAX)]
    c["contributing_chunks_and_consolidation"] = (calls, {"max_chunks": 4})
    # an arena of 64 rows: it fills, grows and compacts
    calls, now = [], 0
    for s in range(12):
        calls.append(_batch(rng, (40, 40, 100, 7)[s % 4], now, now + 90))
        if s % 3 == 2:
            calls.append(("w", now + 20))
        now += 30
    c["arena_growth"] = (calls + [("w", K.I64_MAX)], {"capacity": 64})
    # equal timestamps inside a chunk and across chunks; W equal to a row's ts releases it and
    # makes a later arrival with that ts late; repeated and smaller watermarks
    c["ties_and_watermarks"] = (
        [("w", -5), ("p", [1, 2, 3, 4], [20, 10, 20, 10], [1, 2, 3, 4]),
         ("p", [5, 6, 7], [20, 10, 30], [5, 6, 7]), ("p", [8, 9], [10, 20], [8, 9]),
         ("w", 9), ("w", 10), ("p", [10, 11, 12], [10, 20, 11], [10, 11, 12]), ("w", 10),
         ("w", 3), ("w", 20), ("p", [13, 14], [20, 21], [13, 14]), ("w", 19), ("w", 1000),
         ("w", K.I64_MAX)], {})
    # negative timestamps; rows 2**62 - 2 apart and at both ends of the range (a 63-bit sort)
    far = [-(LIM - 1), -1, LIM - 1]
    c["timestamp_range"] = (
        [("p", [1, 2], [far[2], far[0]], [1, 2]), ("p", [3, 4, 5], [far[1], far[0], -7], [3, 4, 5]),
         ("p", [6, 7, 8], far, [6, 7, 8]), ("w", -LIM), ("w", -1), ("w", K.I64_MAX)], {})
    c["timestamp_range_one_release"] = (
        [("p", [1, 2], [far[2], far[0]], [1, 2]), ("p", [3, 4, 5], [far[1], far[0], -7], [3, 4, 5]),
         ("w", K.I64_MAX)], {})
    # a batch that is entirely late, one that is partly late, one row alone late
    c["late_rows"] = (
        [("p", [1, 2], [5, 9], [1, 2]), ("w", 7), ("p", [3, 4, 5], [7, 1, -3], [3, 4, 5]),
         ("p", [6, 7, 8, 9], [8, 7, 12, 2], [6, 7, 8, 9]), ("p", [1], [7], [1]), ("p", [1], [8], [1]),
         ("w", 8), ("w", K.I64_MAX), ("p", [1, 2], [LIM - 1, 0], [1, 2])], {})
    c["empty"] = ([("w", 5), ("p", [], [], []), ("w", 6), ("p", [1], [7], [1]), ("p", [], [], []),
                   ("w", 7), ("w", 8)], {})
    return c


HAND = _hand_cases()


def _check_hand(name, trace, m):
    contrib = [t[1] for t in trace if t[0] == "w"]
    pushes = [t for t in trace if t[0] == "p"]
    if name == "chunk_lengths":
        assert contrib[0] == 0 and max(contrib) >= 7   # nothing below every row; then all chunks
    if name.startswith("release_total_"):
        assert contrib == [2, 2] and m.cross_ties == 0
    if name == "contributing_chunks_and_consolidation":
        assert contrib[:3] == [1, 2, 3] and pushes[-1][3] >= 1 and m.cross_ties == 0
        assert all(len(p[4]) <= 4 for p in pushes)
    if name == "arena_growth":
        assert pushes[0][2] == 64 and pushes[-1][2] > 64 and pushes[-1][3] >= 2
    if name == "ties_and_watermarks":
        assert m.cross_ties >= 2 and m.late == 2
    if name.startswith("timestamp_range"):
        assert max(contrib) >= 2
    if name == "late_rows":
        assert m.late == 3 + 2 + 1 + 2 and contrib == [1, 2, 2]


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_built_calls_equal_the_model(name):
    calls, kw = HAND[name]
    buf, out, trace = _run(calls, **kw)
    m = _agrees(buf, out, calls)
    _check_hand(name, trace, m)
    if calls[-1] == ("w", K.I64_MAX):
        assert buf.rows_buffered == 0 and buf.chunks == [] and buf.tail == 0


def test_exact_rows_of_a_small_example():
    buf = EventOrderBuffer()
    buf.push(T([1, 2, 3]), T([30, 10, 20]), T([7, 8, 9]))
    buf.push(T([4, 5]), T([10, 40]), T([1, 2]))
    assert buf.release(5) is None and buf.last_contrib == 0
    assert _tuples(buf.release(10)) == [(2, 10, 8), (4, 10, 1)]
    assert buf.last_contrib == 2 and buf.wm == 10
    buf.push(T([6, 7]), T([10, 25]), T([1, 2]))
    assert buf.metrics.num_late_records_dropped == 1
    assert [x.tolist() for x in buf.contents()] == [[3, 7, 1, 5], [20, 25, 30, 40], [9, 2, 7, 2]]
    # one chunk contributes: slices of the arena, no copy
    got = buf.release(20)
    assert _tuples(got) == [(3, 20, 9)] and buf.last_contrib == 1
    assert got[1].data_ptr() == buf.arena[1, 1:].data_ptr()
    assert _tuples(buf.release(K.I64_MAX)) == [(7, 25, 2), (1, 30, 7), (5, 40, 2)]
    assert buf.chunks == [] and buf.metrics.num_fires == 3


def test_nothing_due_makes_no_launch_and_no_readback(monkeypatch):
    buf = EventOrderBuffer()
    buf.push(T([1, 2]), T([50, 60]), T([0, 0]), bounds=(50, 60))
    monkeypatch.setattr(K, "reorder_cut", lambda *a, **k: pytest.fail("a launch"))
    assert buf.release(10) is None and buf.release(49) is None and buf.wm == 49
    buf.push(T([]), T([]), T([]))
    monkeypatch.undo()
    assert _tuples(buf.release(50)) == [(1, 50, 0)]


# ---- the random stream ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stream(seed: int, nkeys: int = 300, steps: int = 24):
    """The burst-alert tests' call generator: 0 to 399 rows per step, +-30 ms of disorder, 10 % of
    the rows 500 ms behind, equal timestamps, empty batches, repeated and regressing
    watermarks."""
    rng = np.random.default_rng(seed)
    calls, now, wm = [], 1_000, 0
    for s in range(steps):
        n = 0 if s % 7 == 3 else int(rng.integers(1, 400))
        keys = rng.integers(0, nkeys, n).astype(np.int64)
        ts = now + rng.integers(-30, 30, n)
        late = rng.random(n) < 0.1
        ts = np.where(late, ts - 500, ts).astype(np.int64)
        if n > 2:
            ts[1] = ts[0]
            keys[1] = keys[0]
        calls.append(("p", keys, ts, rng.integers(K.I64_MIN, K.I64_MAX, n)))
        if s % 5 == 4:
            calls.append(("p", np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)))
        if rng.random() < 0.7:
            wm = max(wm, now - int(rng.integers(0, 80)))
            calls.append(("w", wm))
            if rng.random() < 0.4:
                calls.append(("w", wm))
            if rng.random() < 0.2:
                calls.append(("w", wm - 50))
        now += int(rng.integers(5, 60))
    return calls + [("w", K.I64_MAX)]


@pytest.mark.parametrize("seed", SEEDS)
def test_streams_hold_late_rows_wide_releases_and_cross_chunk_ties(seed):
    m, _ = _model(_stream(seed))
    assert m.late >= 1 and m.max_batches >= 3 and m.cross_ties >= 1
    assert sum(c[0] == "p" and len(c[1]) == 0 for c in _stream(seed)) >= 1


@pytest.mark.parametrize("kw", [{}, {"max_chunks": 2}, {"capacity": 64}], ids=str)
@pytest.mark.parametrize("seed", SEEDS)
def test_random_stream_equals_the_model(seed, kw):
    calls = _stream(seed)
    buf, out, trace = _run(calls, **kw)
    _agrees(buf, out, calls)
    if not kw:
        assert max(t[1] for t in trace if t[0] == "w") >= 3 and buf.consolidations == 0
    else:
        assert buf.consolidations >= 1


@pytest.mark.parametrize("kw", [{}, {"max_chunks": 2}], ids=str)
@pytest.mark.parametrize("seed", SEEDS)
def test_snapshot_in_mid_stream_continues_to_the_same_output(seed, kw):
    calls = _stream(seed)[:-1]   # rows are left at the end
    at = len(calls) // 2
    ref, want, _ = _run(calls, **kw)
    buf, out, _ = _run(calls, snapshot_at=at, seed=seed, **kw)
    assert ref.rows_buffered > 0 and out == want
    assert all(np.array_equal(a, b) for a, b in zip(buf.contents(), ref.contents()))
    assert buf.wm == ref.wm
    assert buf.metrics.num_late_records_dropped == ref.metrics.num_late_records_dropped
    _agrees(buf, out, calls)


def test_snapshot_of_an_empty_buffer_and_a_foreign_checkpoint():
    buf = EventOrderBuffer()
    buf.release(7)
    snap = buf.snapshot_state()
    assert all(v.size == 0 for v in snap.columns.values()) and snap.meta["wm"] == 7
    fresh = EventOrderBuffer(capacity=1)
    fresh.restore_state(snap.columns, snap.meta)
    assert fresh.wm == 7 and fresh.chunks == []
    with pytest.raises(ValueError, match="different operator"):
        fresh.restore_state(snap.columns, {"kind": "burst"})
    cols = {k: np.array([1], dtype=np.int64) for k in ("key", "bits", "ord")}
    with pytest.raises(ValueError, match="behind its watermark"):
        fresh.restore_state({**cols, "ts": np.array([7])}, snap.meta)
    fresh.restore_state({**cols, "ts": np.array([8])}, snap.meta)
    assert _tuples(fresh.release(8)) == [(1, 8, 1)]


# ---- refusals ------------------------------------------------------------------------------------
def test_unsupported_batches_and_parameters_are_refused():
    buf = EventOrderBuffer()
    for ts in ([LIM], [-LIM], [0, K.I64_MIN]):
        with pytest.raises(TypeError):
            buf.push(T([1] * len(ts)), T(ts), T([0] * len(ts)))
    with pytest.raises(TypeError):
        buf.push(T([1]).to(torch.int32), T([1]), T([1]))
    with pytest.raises(TypeError):
        buf.push(T([1, 2]), T([1]), T([1]))
    assert buf.rows_buffered == 0 and buf.metrics.num_records_in == 0
    for bad in (0, -1, True, 2.0, None):
        with pytest.raises(ValueError):
            EventOrderBuffer(capacity=bad)
    for bad in (0, K.REORDER_MAX_CHUNKS, True, None):
        with pytest.raises(ValueError):
            EventOrderBuffer(max_chunks=bad)
    m = K.load()
    assert (m.REORDER_TILE, m.REORDER_MAX_CHUNKS) == (K.REORDER_TILE, K.REORDER_MAX_CHUNKS)
    ts, err, cut = T([1, 2, 3, 4]), T([0]), T([0, 0])
    for begins, ends in (([1], [5]), ([2], [1]), ([-1], [2]), ([], []), ([0], [1, 2])):
        with pytest.raises(ValueError):
            K.reorder_cut(ts, 4, begins, ends, 9, cut)
    with pytest.raises(ValueError):
        K.reorder_cut(ts, 5, [0], [4], 9, cut)   # more rows than the column holds
    for begins, counts in (([2], [3]), ([-1], [1]), ([0], [-1]), ([], [])):
        with pytest.raises(ValueError):
            K.reorder_collect(ts, 4, begins, counts, 0, err)
    cols, dst = (ts, ts, ts), tuple(T([0, 0]) for _ in range(3))
    for perm in ([0, 4], [-1, 0]):
        with pytest.raises(ValueError):
            K.reorder_gather(T(perm), cols, 4, dst, err)
    with pytest.raises(ValueError):
        K.reorder_gather(T([0]), cols, 4, dst, err)   # one index, two rows of output
    assert cut.tolist() == [0, 0] and err.tolist() == [0] and not any(d.any() for d in dst)
    K.reorder_cut(ts, 4, [0, 2], [4, 4], 2, cut)
    assert cut.tolist() == [2, 2]
    key, src = K.reorder_collect(ts, 4, [2, 0], [2, 1], 1, err)
    assert (key.tolist(), src.tolist()) == ([2, 3, 0], [2, 3, 0])


# ---- sanitizer -----------------------------------------------------------------------------------
def test_sanitizer_harness_runs_clean():
    from mxstream.build import build_sanitize_reorder

    res = subprocess.run([str(build_sanitize_reorder())], capture_output=True, text=True,
                         timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.strip().splitlines()[-1] == "reorder sanitize ok"


# ---- GPU: the kernels against the twins, array for array -----------------------------------------
def _same_as_the_twin(calls, gpu_device, **kw):
    twin, want, wtrace = _run(calls, **kw)
    buf, got, gtrace = _run(calls, dev=gpu_device, **kw)
    assert buf.device.type == "cuda"
    assert got == want and gtrace == wtrace
    assert all(np.array_equal(a, b) for a, b in zip(buf.rows(), twin.rows()))
    assert buf.metrics == twin.metrics and (buf.wm, buf.tail, buf.cap) == (twin.wm, twin.tail,
                                                                           twin.cap)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(HAND))
def test_gpu_hand_built_calls_equal_the_twin(gpu_device, name):
    calls, kw = HAND[name]
    _same_as_the_twin(calls, gpu_device, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [{}, {"max_chunks": 2}, {"capacity": 64}], ids=str)
@pytest.mark.parametrize("seed", SEEDS)
def test_gpu_random_stream_equals_the_twin(gpu_device, seed, kw):
    _same_as_the_twin(_stream(seed), gpu_device, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_gpu_snapshot_in_mid_stream_continues_to_the_same_output(gpu_device, seed):
    calls = _stream(seed)[:-1]
    ref, want, _ = _run(calls)
    buf, out, _ = _run(calls, dev=gpu_device, snapshot_at=len(calls) // 2, seed=seed)
    assert out == want
    assert all(np.array_equal(a, b) for a, b in zip(buf.contents(), ref.contents()))


@pytest.mark.gpu
def test_gpu_kernels_equal_the_twins_on_raw_columns(gpu_device):
    """The three kernels alone, on chunk tables the engine would not build: empty chunks between
    full ones, 1023 chunks, totals around the tile."""
    rng = np.random.default_rng(3)
    for k, total_hint in ((1, 1), (2, 4096), (3, 4097), (7, 9000), (1023, 20000)):
        lens = rng.multinomial(total_hint, np.ones(k) / k)
        lens[rng.random(k) < 0.3] = 0
        offs = np.concatenate([[0], np.cumsum(lens + rng.integers(0, 3, k))])
        n_arena = int(offs[-1]) + 5
        ts = np.zeros(n_arena, dtype=np.int64)
        for o, n in zip(offs[:-1], lens):
            ts[o:o + n] = np.sort(rng.integers(-50, 50, n))
        begins, ends = offs[:-1].tolist(), (offs[:-1] + lens).tolist()
        cols = [rng.integers(K.I64_MIN, K.I64_MAX, n_arena) for _ in range(2)]
        res = {}
        for dev in ("cpu", gpu_device):
            t, err = T(ts, dev), T([0], dev)
            cut = T(np.zeros(k), dev)
            K.reorder_cut(t, n_arena, begins, ends, 3, cut)
            counts = [c - b for c, b in zip(cut.tolist(), begins)]
            key, src = K.reorder_collect(t, n_arena, begins, counts, -50, err)
            dst = tuple(T(np.zeros(key.numel()), dev) for _ in range(3))
            K.reorder_gather(src, (T(cols[0], dev), t, T(cols[1], dev)), n_arena, dst, err)
            res[dev] = [x.cpu().tolist() for x in (cut, key, src, *dst, err)]
        assert res["cpu"] == res[gpu_device]
        assert res["cpu"][-1] == [0] and (k == 1 or len(res["cpu"][1]) > 0)
