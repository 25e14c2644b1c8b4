"""Native per-key distinct-count windows: ``WindowDistinctCount`` -> planner -> ``NativeMedianOp``
-> ``KeyedListWindowOperator(func="distinct")`` -> ``segment_distinct_short`` / ``_long``.

The count is exact (a hash set, no sketch), so every comparison is ``==`` on integers.

* the C++ twin (sort + count boundaries) equals ``np.unique`` per segment at the kernels' path
  thresholds (64 lanes, kDistinctLds = 1024 words of LDS table input per wave), with an empty
  segment, non-finite doubles (every NaN one value, -0.0 and 0.0 two) and raw words that contain
  the table's empty marker (all ones);
* the operator equals a plain per-(window, key) oracle on the ranked, mapped and restored firing
  paths, values drawn from ~20 possibilities so that one value lies in several panes of a
  sliding window; a snapshot of a ``func="median"`` operator restores into a distinct one;
* an API job prints the same ``(host3,17)`` lines natively and on the host operator for a float
  and an int field, on 2 loopback ranks, after a restart from a checkpoint, and with a value of
  2**53 + 1 (no double: the host route);
* validation errors;
* GPU (marked): the HIP kernels equal the twin on the set above plus 70 k tiny segments and hot
  segments (many workgroups on one table), and the operator on the GPU equals the one on the CPU.
"""
from collections import Counter
from functools import lru_cache

import numpy as np
import pytest
import torch

from mxstream.ops import kernels as K
from mxstream.runtime.list_window_operator import KeyedListWindowOperator

SEG_LENS = (1, 2, 3, 63, 64, 65, 255, 1023, 1024, 1025, 2049, 4100, 20_000)
K_DISTINCT_LDS = 1024  # csrc/mxs_listwin.h kDistinctLds: longer segments count in the scratch
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


@lru_cache(maxsize=None)
def _segments(gpu_extras: bool):
    """(heads, words as int64, expected counts by np.unique) -- built once, read-only."""
    rng = np.random.default_rng(23)
    segs = []
    for n in SEG_LENS:
        segs.append(rng.permutation(n).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15))
        segs.append(np.full(n, 0x1234_5678_9ABC_DEF0, dtype=np.uint64))
        segs.append(rng.choice(rng.integers(0, 2**63, 7).astype(np.uint64), n))
    segs.insert(5, np.zeros(0, dtype=np.uint64))  # an empty segment between two others
    nan2 = np.array([0x7FF8000000000000, 0x7FF8000000000001], dtype=np.uint64).view(np.float64)
    dbl = np.array([-0.0, 0.0, np.inf, -np.inf, nan2[0], nan2[1], nan2[0], 0.0, -0.0])
    segs.append(K.f64_order_bits(torch.from_numpy(dbl.view(np.int64).copy()))
                .numpy().view(np.uint64))
    n_dbl = len(segs) - 1
    # raw words with the empty marker several times among others (short, and long below)
    segs.append(np.array([5, ALL_ONES, 9, ALL_ONES, 5, 0, ALL_ONES, ALL_ONES - np.uint64(1)],
                         dtype=np.uint64))
    n_raw = len(segs) - 1
    if gpu_extras:
        segs += [rng.integers(0, 3, n).astype(np.uint64)
                 for n in rng.integers(1, 4, 70_000).tolist()]
        segs.append(rng.choice(rng.integers(0, 2**64 - 1, 1000, dtype=np.uint64), 300_000))
        segs.append(rng.permutation(50_000).astype(np.uint64) + np.uint64(1 << 40))
        one = np.full(50_001, 77, dtype=np.uint64)
        one[31_007] = ALL_ONES
        segs.append(one)
    lens = np.array([len(s) for s in segs], dtype=np.int64)
    heads = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    words = np.concatenate(segs).view(np.int64)
    want = np.array([len(np.unique(s)) for s in segs], dtype=np.int64)
    for arr in (heads, words, want):
        arr.setflags(write=False)
    return heads, words, want, n_dbl, n_raw


# ---- 1. twin against numpy ------------------------------------------------------------------
def test_twin_equals_numpy_unique():
    heads, words, want, n_dbl, n_raw = _segments(False)
    got = K.segment_distinct(torch.from_numpy(heads.copy()), torch.from_numpy(words.copy()))
    assert got.dtype == torch.int64 and got.shape == (len(heads),)
    assert np.array_equal(got.numpy(), want)
    assert want[5] == 0  # the empty segment
    assert want[n_dbl] == 5  # -0.0, 0.0, inf, -inf, and every NaN as one value
    assert want[n_raw] == 5  # 5, 9, 0, all ones - 1, and the all-ones word itself
    # all distinct / all equal / 7 values, at every length
    for i, n in enumerate(SEG_LENS):
        j = 3 * i + (1 if 3 * i >= 5 else 0)
        assert want[j] == n


# ---- 2. operator against a plain oracle -----------------------------------------------------
def _events(n, nkeys, span, seed, nvals=20, late_every=0):
    rng = np.random.default_rng(seed)
    k = rng.integers(0, nkeys, n).astype(np.int64)
    t = np.sort(rng.integers(0, span, n)).astype(np.int64)
    v = rng.choice(rng.normal(50, 20, nvals).round(2), n)
    if late_every:
        t[::late_every] -= 2500
    return k, t, v


def _rows(fired):
    return [(s, e, int(key), int(c[i])) for s, e, ks, c in fired for i, key in enumerate(ks)]


def _spy(op, calls):
    for name in ("_fire_ranked", "_fire_dense", "_fire_mapped"):
        if name not in vars(op):
            def spy(*a, _f=getattr(op, name), _n=name, **kw):
                calls[_n] += 1
                return _f(*a, **kw)
            setattr(op, name, spy)


def _run_op(dev, k, t, v, *, size, slide, lateness, steps, bound=500, restore_at=None,
            first_func="distinct"):
    mk = lambda f="distinct": KeyedListWindowOperator(  # noqa: E731
        size=size, slide=slide, lateness=lateness, device=dev, func=f)
    op = mk(first_func)
    calls = Counter()
    out = []
    n = len(k)
    per = -(-n // steps)
    for i in range(steps):
        sl = slice(i * per, min(n, (i + 1) * per))
        if sl.start >= n:
            break
        if i == restore_at:
            snap = op.snapshot_state()
            op = mk()
            op.restore_state(snap.columns, snap.meta)
        _spy(op, calls)
        kt = torch.from_numpy(k[sl]).to(dev)
        tt = torch.from_numpy(t[sl]).to(dev)
        vt = torch.from_numpy(v[sl].view(np.int64)).to(dev)
        fired = op.process(kt, tt, vt) + op.advance_watermark(int(t[sl].max()) - bound)
        if op.distinct:
            out += fired
    out += op.advance_watermark(2**63 - 1)
    for s, e, ks, c in out:
        assert c.shape == (len(ks),) and c.dtype == np.int64
    return op, _rows(out), calls


def _oracle(k, t, v, size, slide, first_end=None):
    """Every (window, key) -> the number of different values among all of the window's."""
    res = {}
    starts = set()
    for ti in t.tolist():
        s = ti - (ti % slide)
        while s > ti - size:
            starts.add(s)
            s -= slide
    for s in sorted(starts):
        if first_end is not None and s + size <= first_end:
            continue
        sel = (t >= s) & (t < s + size)
        for key in np.unique(k[sel]).tolist():
            res[(s, key)] = len(np.unique(v[sel & (k == key)]))
    return res


WINDOWS = [(4000, 4000), (6000, 2000)]


@pytest.mark.parametrize("size,slide", WINDOWS)
def test_operator_ranked_path_equals_oracle(size, slide):
    k, t, v = _events(6000, 37, 40_000, seed=3)
    op, rows, calls = _run_op("cpu", k, t, v, size=size, slide=slide, lateness=0, steps=9)
    ref = _oracle(k, t, v, size, slide)
    assert {(s, key): c for s, e, key, c in rows} == ref
    assert calls["_fire_ranked"] and not calls["_fire_dense"] and not calls["_fire_mapped"]
    assert 10 < max(ref.values()) <= 20  # 20 possible values, repeated within a window
    assert op.metrics.num_late_records_dropped == 0


@pytest.mark.parametrize("size,slide", WINDOWS)
def test_operator_mapped_path_equals_oracle(size, slide):
    k, t, v = _events(3000, 29, 20_000, seed=9)
    big = (k * (1 << 35) + 7).astype(np.int64)
    _, rows, calls = _run_op("cpu", big, t, v, size=size, slide=slide, lateness=0, steps=5)
    ref = {(s, key * (1 << 35) + 7): c for (s, key), c in _oracle(k, t, v, size, slide).items()}
    assert {(s, key): c for s, e, key, c in rows} == ref
    assert calls["_fire_mapped"] and not calls["_fire_ranked"]


@pytest.mark.parametrize("size,slide", WINDOWS)
def test_operator_restored_dense_path_equals_oracle(size, slide):
    """Restored from its own snapshot halfway: restored panes carry no element ranks, so the
    windows that hold them fire through the counting sort (the unranked dense path)."""
    k, t, v = _events(6000, 37, 40_000, seed=3)
    _, rows, calls = _run_op("cpu", k, t, v, size=size, slide=slide, lateness=0, steps=10,
                             restore_at=5)
    assert {(s, key): c for s, e, key, c in rows} == _oracle(k, t, v, size, slide)
    assert calls["_fire_dense"] and not calls["_fire_mapped"]


@pytest.mark.parametrize("size,slide", WINDOWS)
def test_median_snapshot_restores_into_distinct(size, slide):
    """The arena is shared: the panes a median operator kept are the panes a distinct one
    counts. Windows the median operator fired before the snapshot are not fired again."""
    k, t, v = _events(6000, 37, 40_000, seed=3)
    op, rows, calls = _run_op("cpu", k, t, v, size=size, slide=slide, lateness=0, steps=10,
                              restore_at=5, first_func="median")
    assert op.distinct and calls["_fire_dense"]
    wm_at_restore = int(t[5 * 600 - 1]) - 500
    ref = _oracle(k, t, v, size, slide, first_end=wm_at_restore + 1)
    assert ref and {(s, key): c for s, e, key, c in rows} == ref


# ---- 3. API job -----------------------------------------------------------------------------
def _value(i: int, kind: str, big_at, collide=False):
    if kind == "float":
        return float((i * 37) % 23) / 4
    if big_at is not None and i in (big_at, big_at + 7):
        # two ids of one host, 280 ms apart, that are one double: 2**53 + 1 rounds to 2**53
        return 2**53 + (1 if i == big_at and not collide else 0)
    return (i * 37) % 23 - 11  # negative ids too


def _distinct_job(tmp_path=None, fault=None, comm=None, native="auto", kind="float", big_at=None,
                  collide=False):
    from mxstream.api.aggregations import WindowDistinctCount
    from mxstream.api.environment import (FsStateBackend, RestartStrategies,
                                          StreamExecutionEnvironment)
    from mxstream.api.time import Time, TimeCharacteristic
    from mxstream.api.tuples import Tuple2
    from mxstream.api.watermarks import BoundedOutOfOrdernessTimestampExtractor
    from mxstream.runtime.executor import ManualClock

    out = []
    env = StreamExecutionEnvironment(4, clock=ManualClock(0)).set_output(out.append)
    env.config.native = native
    env.config.fault_injection = fault
    env._comm = comm
    env.set_stream_time_characteristic(TimeCharacteristic.EventTime)
    if tmp_path is not None:
        env.enable_checkpointing(500)
        env.set_state_backend(FsStateBackend(str(tmp_path)))
        env.set_restart_strategy(RestartStrategies.fixed_delay_restart(2, 0))
    ev = [(i * 40 + 10, (f"host{i % 7}", _value(i, kind, big_at, collide), i * 40)) for i in range(400)]
    (env.from_timed_collection(ev)
     .assign_timestamps_and_watermarks(
         BoundedOutOfOrdernessTimestampExtractor(Time.milliseconds(100), extractor=lambda e: e[2]))
     .map(lambda e: Tuple2(e[0], e[1]))
     .key_by(0)
     .time_window(Time.milliseconds(3000), Time.milliseconds(1000))
     .process(WindowDistinctCount(1))
     .print())
    res = env.execute("distinct-ft")
    return out, res


@pytest.fixture
def native_ops_built(monkeypatch):
    """The functions of the list-window operators built (the native path)."""
    built = []
    init = KeyedListWindowOperator.__init__

    def spy(self, *a, **kw):
        init(self, *a, **kw)
        built.append(kw.get("func"))

    monkeypatch.setattr(KeyedListWindowOperator, "__init__", spy)
    return built


@pytest.mark.parametrize("kind", ["float", "int"])
def test_api_job_native_equals_host(native_ops_built, kind):
    import re

    host, _ = _distinct_job(native="off", kind=kind)
    assert not native_ops_built
    clean, _ = _distinct_job(kind=kind)
    assert native_ops_built and all(f == "distinct" for f in native_ops_built)
    assert Counter(clean) == Counter(host)
    # 7 hosts x 18 sliding windows over 16 s of events, one "(host3,17)" line each
    assert len(clean) == 7 * 18
    assert all(re.fullmatch(r"(\d+> )?\(host[0-6],\d+\)", ln) for ln in clean), clean[:3]
    assert len({ln[ln.index("("):] for ln in clean}) > 7  # counts differ between windows


def test_api_job_invariant_to_world():
    from mxstream.parallel.comm import run_loopback

    ref, _ = _distinct_job(kind="int")
    res = run_loopback(2, lambda comm: _distinct_job(comm=comm, kind="int"))
    got = [line for out, _ in res for line in out]
    assert Counter(got) == Counter(ref)


def test_api_job_restarts_from_checkpoint(tmp_path):
    clean, _ = _distinct_job(kind="int")
    got, res = _distinct_job(tmp_path / "ft", fault="Window:200", kind="int")
    assert res.metrics["numRestarts"] == 1
    assert res.metrics["restoredCheckpointId"] >= 1
    assert set(got) == set(clean)


def test_api_job_integer_beyond_2_53_takes_the_host_route(monkeypatch):
    """2**53 + 1 is no double (as one it would be counted as the 2**53 beside it): the batch
    that holds it is "mixed value types" and the exact host operator prints the lines."""
    from mxstream.runtime.native_ops import NativeMedianOp

    routed = []
    to_fallback = NativeMedianOp._to_fallback

    def spy(self):
        routed.append(self.kind)
        to_fallback(self)

    monkeypatch.setattr(NativeMedianOp, "_to_fallback", spy)
    host, _ = _distinct_job(native="off", kind="int", big_at=0)
    assert not routed
    got, _ = _distinct_job(kind="int", big_at=0)
    assert routed == ["distinct"]
    assert Counter(got) == Counter(host) and len(got) == 7 * 18
    # the two large ids are two values: were they one (as doubles they are), a count drops
    merged, _ = _distinct_job(native="off", kind="int", big_at=0, collide=True)
    assert Counter(merged) != Counter(host)


def test_host_function_equality_is_javas():
    from mxstream.api.aggregations import WindowDistinctCount

    class Out:
        def collect(self, v):
            self.v = v

    nan2 = np.array([0x7FF8000000000000, 0x7FF8000000000001], dtype=np.uint64).view(np.float64)
    vals = [-0.0, 0.0, float(nan2[0]), float(nan2[1]), 1, 1.0, 1, "1", 2**53, 2**53 + 1]
    out = Out()
    WindowDistinctCount(0).process("k", None, [(v,) for v in vals], out)
    # -0.0, 0.0, NaN, 1, 1.0, "1", 2**53, 2**53 + 1
    assert tuple(out.v) == ("k", 8) and type(out.v[1]) is int


# ---- 4. validation --------------------------------------------------------------------------
def test_validation_errors():
    from mxstream.api.aggregations import WindowDistinctCount

    for bad in (-1, 1.0, "1", True, None):
        with pytest.raises(ValueError):
            WindowDistinctCount(bad)
    assert WindowDistinctCount(2).native == ("distinct", 2)
    for bad in ("distinct_count", ("distinct",), ("distinct", 1), None):
        with pytest.raises(ValueError):
            KeyedListWindowOperator(size=1000, func=bad)
    ob = torch.zeros(4, dtype=torch.int64)
    for bad in ([1, 2], [0, 4], [0, 5, 2], [0, 3, 2]):
        with pytest.raises(ValueError):
            K.segment_distinct(torch.tensor(bad, dtype=torch.int64), ob)
    with pytest.raises(TypeError):
        K.segment_distinct(torch.zeros(1, dtype=torch.int32), ob)
    with pytest.raises(TypeError):
        K.segment_distinct(torch.zeros(1, dtype=torch.int64), ob.to(torch.float64))
    with pytest.raises(ValueError):
        K.segment_distinct(torch.zeros(4, dtype=torch.int64)[::2], ob)
    assert K.segment_distinct(torch.zeros(0, dtype=torch.int64), ob).numel() == 0


# ---- GPU ------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_kernel_equals_twin(gpu_device):
    """The HIP kernels against the twin, count for count: LDS tables up to kDistinctLds words,
    scratch tables beyond; 70 k segments of 1 to 3 words so that the grid-stride loop over
    segments runs (the grid covers 65,536 at once); a hot segment of 300,000 words holding
    1,000 values (many workgroups and heavy duplicate traffic on one table); 50,000 distinct
    words (the table exactly half full); 50,000 copies of one word plus the empty marker (every
    lane meets the same slot); and the error word clear afterwards."""
    heads, words, want, _, _ = _segments(True)
    assert len(heads) > 16384 * 4 and len(words) > 600_000
    h = torch.from_numpy(heads.copy())
    w = torch.from_numpy(words.copy())
    twin = K.segment_distinct(h, w)
    assert np.array_equal(twin.numpy(), want)
    assert want[-3] == 1000 and want[-2] == 50_000 and want[-1] == 2
    hg, wg = h.to(gpu_device), w.to(gpu_device)
    got, meta = K.segment_distinct_launch(hg, hg.numel(), wg.numel(), wg)
    torch.cuda.synchronize()
    assert meta is not None and meta.tolist()[1] == 0  # no probe bound was hit
    K.segment_distinct_check(meta)
    assert torch.equal(got.cpu(), twin)
    assert torch.equal(K.segment_distinct(hg, wg).cpu(), twin)


@pytest.mark.gpu
@pytest.mark.parametrize("size,slide,lateness", [(4000, 4000, 0), (6000, 2000, 3000)])
def test_gpu_operator_equals_cpu_operator(gpu_device, size, slide, lateness):
    k, t, v = _events(40_000, 500, 24_000, seed=11, late_every=97 if lateness else 0)
    # one key with 5,000 values, 3,000 of them different, inside the tumbling window
    # [8000, 12000) (and so inside the sliding windows that cover it): a long segment
    hot = np.nonzero((t >= 8000) & (t < 12_000))[0][:5000]
    assert len(hot) == 5000 > K_DISTINCT_LDS
    k[hot] = 123
    v[hot] = np.random.default_rng(5).permutation(np.arange(5000) % 3000) / 8 + 1000.0
    _, g, _ = _run_op(gpu_device, k, t, v, size=size, slide=slide, lateness=lateness, steps=8)
    _, c, _ = _run_op("cpu", k, t, v, size=size, slide=slide, lateness=lateness, steps=8)
    assert len(c) > 500 and sorted(g) == sorted(c)
    assert max(cnt for _, _, key, cnt in c if key == 123) >= 3000
