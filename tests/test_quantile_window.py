"""Native per-key quantile windows: ``WindowQuantiles`` -> planner -> ``NativeMedianOp`` ->
``KeyedListWindowOperator(func=("quantiles", ppm))`` -> ``segment_quantile_select``.

Semantics under test (identical on the GPU, in the C++ twin and in the host function): a
quantile is an integer ``ppm = round(q * 1e6)``; of n >= 1 ascending values (order bits order:
-0.0 < 0.0, NaN last) it selects index ``clamp((n * ppm + 999_999) // 1_000_000 - 1, 0, n - 1)``
-- the element itself, so every comparison is on bit patterns or exact values, no tolerance.

* the C++ twin equals ``np.sort`` on the order bits + the rank rule, at the kernel's path
  thresholds (64 lanes, kMedLds = 2048 values of LDS per wave), with ties and non-finite values;
* the operator equals a plain per-(window, key) oracle on the ranked, mapped and restored
  (unranked dense) firing paths;
* an API job prints the same lines natively and on the host operator, on 2 loopback ranks, and
  after a restart from a checkpoint;
* ``func="median"`` is what the operator does without ``func``;
* validation errors;
* GPU (marked): the HIP kernel equals the twin bit for bit (grid-stride over 70 k segments), and
  the operator on the GPU equals the operator on the CPU, long (global-memory) segments included.
"""
from collections import Counter
from functools import lru_cache

import numpy as np
import pytest
import torch

from mxstream.ops import kernels as K
from mxstream.runtime.list_window_operator import KeyedListWindowOperator

PPM = (0, 500_000, 900_000, 990_000, 999_999, 1_000_000, 500_000)  # the duplicate is intended
OP_PPM = (500_000, 950_000, 0, 1_000_000, 950_000)
SEG_LENS = (1, 2, 3, 63, 64, 65, 255, 2047, 2048, 2049, 4100)
K_MED_LDS = 2048  # csrc/kernels_hip.hip kMedLds: longer segments select over global memory


def _rank(n: int, ppm: int) -> int:
    return min(max((n * ppm + 999_999) // 1_000_000 - 1, 0), n - 1)


def _from_order_bits(o: np.ndarray) -> np.ndarray:
    """u64 order bits -> f64 bit patterns (inverse of f64_order_bits), as int64."""
    top = (o >> np.uint64(63)).astype(bool)
    return np.where(top, o & np.uint64(0x7FFFFFFFFFFFFFFF), ~o).view(np.int64)


@lru_cache(maxsize=None)
def _segments(many_short: bool):
    """(heads, order bits, expected int64 bit patterns [Q, nseg]) -- built once, read-only."""
    rng = np.random.default_rng(17)
    segs = [rng.normal(50, 20, n).round(2) for n in SEG_LENS]
    segs.append(np.full(300, 12.5))  # every value ties
    segs.append(np.array([-0.0, 0.0, -np.inf, np.inf, np.nan, np.nan]))
    if many_short:
        segs += [rng.normal(0, 1, n) for n in rng.integers(1, 4, 70_000).tolist()]
    lens = np.array([len(s) for s in segs], dtype=np.int64)
    heads = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    vals = np.concatenate(segs)
    ob = K.f64_order_bits(torch.from_numpy(vals.view(np.int64).copy()))
    obu = ob.numpy().view(np.uint64)
    want = np.empty((len(PPM), len(segs)), dtype=np.int64)
    for i, (a, n) in enumerate(zip(heads.tolist(), lens.tolist())):
        so = np.sort(obu[a:a + n])
        want[:, i] = _from_order_bits(so[[_rank(n, p) for p in PPM]])
    for arr in (heads, want):
        arr.setflags(write=False)
    return heads, ob, want


# ---- 1. twin against numpy ------------------------------------------------------------------
def test_twin_equals_numpy_sort_and_rank_rule():
    heads, ob, want = _segments(False)
    got = K.segment_quantiles(torch.from_numpy(heads.copy()), ob, PPM)
    assert got.shape == (len(PPM), len(heads)) and got.dtype == torch.float64
    assert np.array_equal(got.view(torch.int64).numpy(), want)
    # ppm 0 / 1e6 are the minimum / maximum; the duplicated quantile fills both columns
    assert np.array_equal(want[1], want[6])
    nan_seg = len(SEG_LENS) + 1
    assert got[0, nan_seg].item() == -np.inf and np.isnan(got[5, nan_seg].item())
    # sorted: -inf, -0.0, 0.0, inf, NaN, NaN -- the median rank 2 is +0.0, after -0.0
    assert got[1, nan_seg].item() == 0.0 and not np.signbit(got[1, nan_seg].item())


# ---- 2. operator against a plain oracle -----------------------------------------------------
def _events(n, nkeys, span, seed, late_every=0):
    rng = np.random.default_rng(seed)
    k = rng.integers(0, nkeys, n).astype(np.int64)
    t = np.sort(rng.integers(0, span, n)).astype(np.int64)
    v = rng.normal(50, 20, n).round(2)
    if late_every:
        t[::late_every] -= 2500
    return k, t, v


def _rows(fired):
    return [(s, e, int(key), tuple(float(x) for x in q[:, i]))
            for s, e, ks, q in fired for i, key in enumerate(ks)]


def _run_op(dev, k, t, v, *, size, slide, lateness, steps, bound=500, ppm=OP_PPM,
            restore_at=None):
    mk = lambda: KeyedListWindowOperator(size=size, slide=slide, lateness=lateness,  # noqa: E731
                                         device=dev, func=("quantiles", ppm))
    op = mk()
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
        for name in ("_fire_ranked", "_fire_dense", "_fire_mapped"):
            if name not in vars(op):
                def spy(*a, _f=getattr(op, name), _n=name, **kw):
                    calls[_n] += 1
                    return _f(*a, **kw)
                setattr(op, name, spy)
        kt = torch.from_numpy(k[sl]).to(dev)
        tt = torch.from_numpy(t[sl]).to(dev)
        vt = torch.from_numpy(v[sl].view(np.int64)).to(dev)
        out += op.process(kt, tt, vt)
        out += op.advance_watermark(int(t[sl].max()) - bound)
    out += op.advance_watermark(2**63 - 1)
    for s, e, ks, q in out:
        assert q.shape == (len(ppm), len(ks)) and q.dtype == np.float64
    return op, _rows(out), calls


def _oracle(k, t, v, size, slide, ppm=OP_PPM):
    """Every (window, key) -> its quantile elements over all of the window's values."""
    res = {}
    starts = set()
    for ti in t.tolist():
        s = ti - (ti % slide)
        while s > ti - size:
            starts.add(s)
            s -= slide
    for s in sorted(starts):
        sel = (t >= s) & (t < s + size)
        for key in np.unique(k[sel]).tolist():
            so = np.sort(v[sel & (k == key)])
            res[(s, key)] = tuple(float(so[_rank(len(so), p)]) for p in ppm)
    return res


WINDOWS = [(4000, 4000), (6000, 2000)]


@pytest.mark.parametrize("size,slide", WINDOWS)
def test_operator_ranked_path_equals_oracle(size, slide):
    k, t, v = _events(6000, 37, 40_000, seed=3)
    op, rows, calls = _run_op("cpu", k, t, v, size=size, slide=slide, lateness=0, steps=9)
    assert {(s, key): q for s, e, key, q in rows} == _oracle(k, t, v, size, slide)
    assert calls["_fire_ranked"] and not calls["_fire_dense"] and not calls["_fire_mapped"]
    assert op.metrics.num_late_records_dropped == 0


@pytest.mark.parametrize("size,slide", WINDOWS)
def test_operator_mapped_path_equals_oracle(size, slide):
    k, t, v = _events(3000, 29, 20_000, seed=9)
    big = (k * (1 << 35) + 7).astype(np.int64)
    _, rows, calls = _run_op("cpu", big, t, v, size=size, slide=slide, lateness=0, steps=5)
    ref = {(s, key * (1 << 35) + 7): q for (s, key), q in _oracle(k, t, v, size, slide).items()}
    assert {(s, key): q for s, e, key, q in rows} == ref
    assert calls["_fire_mapped"] and not calls["_fire_ranked"]


@pytest.mark.parametrize("size,slide", WINDOWS)
def test_operator_restored_dense_path_equals_oracle(size, slide):
    """A run restored from its own snapshot halfway: restored panes carry no element ranks, so
    the windows that hold them fire through the counting sort (the unranked dense path)."""
    k, t, v = _events(6000, 37, 40_000, seed=3)
    _, rows, calls = _run_op("cpu", k, t, v, size=size, slide=slide, lateness=0, steps=10,
                             restore_at=5)
    assert {(s, key): q for s, e, key, q in rows} == _oracle(k, t, v, size, slide)
    assert calls["_fire_dense"] and not calls["_fire_mapped"]


# ---- 3. API job -----------------------------------------------------------------------------
def _quantile_job(tmp_path=None, fault=None, comm=None, native="auto", qs=(0.5, 0.95, 1.0)):
    from mxstream.api.aggregations import WindowQuantiles
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
    ev = [(i * 40 + 10, (f"h{i % 7}", float((i * 37) % 101) / 4, i * 40)) for i in range(400)]
    (env.from_timed_collection(ev)
     .assign_timestamps_and_watermarks(
         BoundedOutOfOrdernessTimestampExtractor(Time.milliseconds(100), extractor=lambda e: e[2]))
     .map(lambda e: Tuple2(e[0], e[1]))
     .key_by(0)
     .time_window(Time.milliseconds(2000))
     .process(WindowQuantiles(1, list(qs)))
     .print())
    res = env.execute("quantiles-ft")
    return out, res


@pytest.fixture
def native_ops_built(monkeypatch):
    """Counts the list-window operators built with a quantile function (the native path)."""
    built = []
    init = KeyedListWindowOperator.__init__

    def spy(self, *a, **kw):
        init(self, *a, **kw)
        built.append(self.ppm)

    monkeypatch.setattr(KeyedListWindowOperator, "__init__", spy)
    return built


def test_api_job_native_equals_host(native_ops_built):
    host, _ = _quantile_job(native="off")
    assert not native_ops_built
    clean, _ = _quantile_job()
    assert native_ops_built and all(p == [500_000, 950_000, 1_000_000] for p in native_ops_built)
    assert Counter(clean) == Counter(host)
    # 7 hosts x 8 windows of 2 s over 16 s of events, one "(key,p50,p95,max)" line each
    assert len(clean) == 56 and all(ln.count(",") == 3 and "(h" in ln for ln in clean)


def test_api_job_eight_quantiles_native_equals_host(native_ops_built):
    """The widest row, key + 8 quantiles (nine columns in one batch), duplicates included."""
    qs = (0.0, 0.25, 0.5, 0.75, 0.9, 0.99, 1.0, 0.5)
    clean, _ = _quantile_job(qs=qs)
    assert native_ops_built
    host, _ = _quantile_job(native="off", qs=qs)
    assert Counter(clean) == Counter(host) and len(clean) == 56
    assert all(ln.count(",") == 8 for ln in clean)


def test_api_job_invariant_to_world():
    from mxstream.parallel.comm import run_loopback

    ref, _ = _quantile_job()
    res = run_loopback(2, lambda comm: _quantile_job(comm=comm))
    got = [line for out, _ in res for line in out]
    assert Counter(got) == Counter(ref)


def test_api_job_restarts_from_checkpoint(tmp_path):
    clean, _ = _quantile_job()
    got, res = _quantile_job(tmp_path / "ft", fault="Window:200")
    assert res.metrics["numRestarts"] == 1
    assert res.metrics["restoredCheckpointId"] >= 1
    assert set(got) == set(clean)


# ---- 4. func="median" is unchanged ----------------------------------------------------------
def test_median_func_is_the_default():
    k, t, v = _events(4000, 23, 20_000, seed=6)
    outs = []
    for kw in ({}, {"func": "median"}):
        op = KeyedListWindowOperator(size=6000, slide=2000, device="cpu", **kw)
        fired = op.process(torch.from_numpy(k), torch.from_numpy(t),
                           torch.from_numpy(v.view(np.int64)))
        fired += op.advance_watermark(2**63 - 1)
        assert all(m.ndim == 1 for _, _, _, m in fired)
        outs.append([(s, e, ks.tolist(), m.view(np.int64).tolist()) for s, e, ks, m in fired])
    assert outs[0] and outs[0] == outs[1]


# ---- 5. validation --------------------------------------------------------------------------
def test_validation_errors():
    from mxstream.api.aggregations import WindowQuantiles

    for bad in ([], [0.1] * 9, [1.5], [-0.01], [float("nan")], ["0.5"]):
        with pytest.raises(ValueError):
            WindowQuantiles(1, bad)
    assert WindowQuantiles(1, [0, 1, 0.999]).native == ("quantiles", 1, (0, 1_000_000, 999_000))
    heads = torch.zeros(1, dtype=torch.int64)
    ob = torch.zeros(4, dtype=torch.int64)
    for bad in ((1_000_001,), (-1,), (), (1,) * 9, (0.5,)):
        with pytest.raises(ValueError):
            K.segment_quantiles(heads, ob, bad)
    with pytest.raises(ValueError):
        KeyedListWindowOperator(size=1000, func=("quantiles", (2_000_000,)))
    with pytest.raises(ValueError):
        KeyedListWindowOperator(size=1000, func="p99")


# ---- GPU ------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_kernel_equals_twin(gpu_device):
    """The HIP kernel against the twin, bit for bit: the LDS path up to kMedLds values, the
    global-memory path beyond, ties, non-finite values, and 70 k segments of 1 to 3 values so
    that the grid-stride loop over segments runs (the grid covers 65,536 segments at once)."""
    heads, ob, want = _segments(True)
    assert len(heads) > 16384 * 4
    h = torch.from_numpy(heads.copy())
    twin = K.segment_quantiles(h, ob, PPM)
    assert np.array_equal(twin.view(torch.int64).numpy(), want)
    got = K.segment_quantiles(h.to(gpu_device), ob.to(gpu_device), PPM)
    torch.cuda.synchronize()
    assert torch.equal(got.cpu().view(torch.int64), twin.view(torch.int64))


@pytest.mark.gpu
@pytest.mark.parametrize("size,slide,lateness", [(4000, 4000, 0), (6000, 2000, 3000)])
def test_gpu_operator_equals_cpu_operator(gpu_device, size, slide, lateness):
    k, t, v = _events(40_000, 500, 24_000, seed=11, late_every=97 if lateness else 0)
    # one key with 5,000 values inside the tumbling window [8000, 12000) (and so inside the
    # sliding windows that cover it): its segment is longer than kMedLds
    hot = np.nonzero((t >= 8000) & (t < 12_000))[0][:5000]
    assert len(hot) == 5000 > K_MED_LDS
    k[hot] = 123
    _, g, _ = _run_op(gpu_device, k, t, v, size=size, slide=slide, lateness=lateness, steps=8)
    _, c, _ = _run_op("cpu", k, t, v, size=size, slide=slide, lateness=lateness, steps=8)
    assert len(c) > 500 and sorted(g) == sorted(c)


def _lw_scan(counts: np.ndarray, kmin: int, dev):
    """lw_scan of the key counts: (offs, heads, head_keys) with the heads cut to their number."""
    m, nk = K.load(), counts.size
    c = torch.from_numpy(counts.astype(np.int32)).to(dev)
    cuda = c.is_cuda
    offs = torch.empty(nk + 1, dtype=torch.int64, device=dev)
    heads = torch.full((nk,), -1, dtype=torch.int64, device=dev)
    hkeys = torch.full((nk,), -1, dtype=torch.int64, device=dev)
    nh = torch.zeros(1, dtype=torch.int64, device=dev)
    scratch = torch.empty(max(16, m.lw_scan_scratch_bytes(nk)), dtype=torch.uint8, device=dev)
    m.lw_scan(cuda, c.data_ptr(), nk, kmin, scratch.data_ptr(), offs.data_ptr(), heads.data_ptr(),
              hkeys.data_ptr(), nh.data_ptr(), torch.cuda.current_stream().cuda_stream if cuda else 0)
    k = int(nh.item())
    return offs.cpu(), heads[:k].cpu(), hkeys[:k].cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("ends", [0, 3], ids=["ends-empty", "ends-nonempty"])
@pytest.mark.parametrize("n", [1, 4095, 4096, 4097])
def test_gpu_key_scan_tile_seams_equal_the_twin(gpu_device, n, ends):
    rng = np.random.default_rng(n)
    counts = rng.integers(0, 4, n) * (rng.random(n) < 0.5)
    counts[0] = counts[-1] = ends
    want, got = _lw_scan(counts, 1000, "cpu"), _lw_scan(counts, 1000, gpu_device)
    ne = np.nonzero(counts)[0]
    excl = np.concatenate([[0], np.cumsum(counts)])
    assert np.array_equal(want[0].numpy(), excl) and np.array_equal(want[2].numpy(), 1000 + ne)
    assert np.array_equal(want[1].numpy(), excl[ne])
    for a, b in zip(got, want):
        assert torch.equal(a, b)
