"""One-pass narrow partition (8-byte records, one destination) vs the C++ twin (needs an MI355X).

Every case partitions the same events on the GPU -- through K.partition (the production
dispatch) or the variant binding, which sets the round size and the events per workgroup -- and
with the C++ twin, and compares per bucket the live records (pane nibble != 15) as multisets.
Below cursor[b] everything that is not a live record must be a padding hole, and a bucket holds
at most kCG - 1 = 3 holes per round that reserved a run in it.
"""
import numpy as np
import pytest
import torch

from mxstream.ops import kernels as K
from mxstream.runtime.window_operator import KeyedWindowOperator

pytestmark = pytest.mark.gpu

V_TWOPASS = 20                                  # gpu_partition_variant numbers
V_ONEPASS = {8192: 21, 16384: 23}
R = 16384                                       # production round (csrc/mxs_common.h kOnePassRound)
GRAN = 4                                        # reservation granule (kPartGranule)
EPG = 2 * R + 4096 + 2                          # events per group: two full rounds + a partial one
HOLE = np.uint64(0xFFFFFFFFFFFFFFFF)
SENTINEL = 0x5A5A5A5A5A5A5A5A


def _events(n, nkeys=50_000, seed=3, span=5000):
    """Events generated once on the CPU: ts in [1000, 1000 + span + 300], values < 1000."""
    keys = torch.empty(n, dtype=torch.int64)
    ts = torch.empty_like(keys)
    vals = torch.empty_like(keys)
    if n:
        K.gen_events(keys, ts, vals, seed=seed, stream_id=1, idx0=17, nkeys=nkeys, ts_base=1000,
                     ts_span=span, disorder=300, val_lo=0, val_span=1000, val_f64=False)
    return keys, ts, vals


def _plan(nsub_log2, bucket_cap, late_ts=None, dense_bits=0):
    return K.PartitionPlan(max_parallelism=128, nsub_log2=nsub_log2, nranks=1, window_mode=1,
                           drop_late=0 if late_ts is None else 1, hash_mode=0,
                           bucket_cap=bucket_cap, late_ts=0 if late_ts is None else late_ts,
                           tbase=500, pane=500, rec_words=1, dense_bits=dense_bits,
                           dense_mul=0x9E3779B1 & ((1 << dense_bits) - 1) | 1 if dense_bits else 0)


def _cap(n, nb, rounds):
    """Room for every record of a bucket three times over, plus the padding holes."""
    return (3 * n // nb + 64 + GRAN * rounds + 7) & ~7


def _rounds(n, epg, r=R):
    """Reservations one bucket can receive: rounds per group, summed over the groups."""
    full, rest = divmod(n, epg)
    return full * -(-epg // r) + -(-rest // r)


def _run(native, dev, ev, plan, variant=None, epg=0, late_cap=None, tail=0, fill=0):
    keys, ts, vals = (x.to(dev) for x in ev)
    n, nb = keys.numel(), plan.nbuckets
    words = nb * plan.bucket_cap * 3
    buf = torch.full((words + tail,), fill, dtype=torch.int64, device=dev)
    out = buf[:words]
    cursor = torch.zeros(nb, dtype=torch.int32, device=dev)
    stats = K.new_stats(dev)
    kg = torch.zeros(128, dtype=torch.int32, device=dev)
    late = None if late_cap is None else torch.full((late_cap,), -1, dtype=torch.int32, device=dev)
    if variant is None:
        K.partition(keys, ts, vals, plan, kg, cursor, out, stats, late_idx=late)
    else:
        native.gpu_partition_variant(keys.data_ptr(), ts.data_ptr(), vals.data_ptr(), 0, n,
                                     plan.as_dict(), kg.data_ptr(), cursor.data_ptr(),
                                     out.data_ptr(), stats.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream, variant,
                                     events_per_group=epg,
                                     late_idx=0 if late is None else late.data_ptr(),
                                     late_cap=0 if late is None else late_cap)
    recs = buf.cpu().numpy().view(np.uint64)
    return dict(cursor=cursor.cpu().numpy().astype(np.int64), stats=stats.cpu(),
                recs=recs[:nb * plan.bucket_cap].reshape(nb, plan.bucket_cap),
                rest=recs[nb * plan.bucket_cap:],
                late=None if late is None else late.cpu().numpy())


def _live(a):
    return a[((a >> np.uint64(32)) & np.uint64(15)) != np.uint64(15)]


def _check(g, c, rounds):
    """GPU result g against the twin's c: stats, live multisets, holes."""
    sg, sc = g["stats"].clone(), c["stats"]
    assert int(sg[K.STAT_MAXBUCKET]) == int(g["cursor"].max())
    sg[K.STAT_MAXBUCKET] = 0
    assert torch.equal(sg, sc)
    assert int(sg[K.STAT_OVERFLOW]) == 0
    for b in range(len(g["cursor"])):
        a = g["recs"][b, :g["cursor"][b]]
        e = c["recs"][b, :c["cursor"][b]]
        live = _live(a)
        assert np.array_equal(np.sort(live), np.sort(e)), f"bucket {b}"
        assert np.all(a[((a >> np.uint64(32)) & np.uint64(15)) == np.uint64(15)] == HOLE)
        assert g["cursor"][b] % GRAN == 0
        assert g["cursor"][b] - len(live) <= (GRAN - 1) * rounds


@pytest.fixture(scope="module")
def events():
    """The largest batch once; every test slices it."""
    return _events(2 * EPG + 1001)


def _head(ev, n, off=0):
    return tuple(x[off:off + n] for x in ev)


@pytest.mark.parametrize("n", [1, 1023, R, R + 1, 2 * EPG + 1001])
def test_round_edges(native, gpu_device, events, n):
    """Full, partial and one-event rounds; three groups of 2R + 4096 + 2 events at the largest n
    (odd: the last PAIR is split). The production dispatch runs the same events."""
    ev = _head(events, n)
    rounds = max(_rounds(n, EPG), -(-n // 4096))  # production: groups of >= 4096 events
    plan = _plan(6, _cap(n, 64, rounds))
    c = _run(native, "cpu", ev, plan)
    _check(_run(native, gpu_device, ev, plan, V_ONEPASS[R], EPG), c, _rounds(n, EPG))
    _check(_run(native, gpu_device, ev, plan), c, rounds)


def test_half_size_rounds(native, gpu_device, events, r=8192):
    """The 8192-record instantiation (kept for A/B runs)."""
    n = 2 * r + 4096 + 2 + 777
    ev = _head(events, n)
    epg = 2 * r + 4096 + 2
    plan = _plan(6, _cap(n, 64, _rounds(n, epg, r)))
    _check(_run(native, gpu_device, ev, plan, V_ONEPASS[r], epg), _run(native, "cpu", ev, plan),
           _rounds(n, epg, r))


@pytest.mark.parametrize("nsub_log2", [0, 3, 9])
def test_bucket_counts(native, gpu_device, events, nsub_log2):
    """One and 8 buckets: every run is longer than a wave's 128-record store. 512 buckets at
    3000 events: most buckets of a round hold a few records, some none."""
    n = 3000 if nsub_log2 == 9 else EPG + 3000
    ev = _head(events, n)
    nb = 1 << nsub_log2
    plan = _plan(nsub_log2, _cap(n, nb, _rounds(n, EPG)))
    _check(_run(native, gpu_device, ev, plan, V_ONEPASS[R], EPG), _run(native, "cpu", ev, plan),
           _rounds(n, EPG))


def test_dense_keys(native, gpu_device, events):
    """Dense ids (dense_bits, dense_mul) instead of the hashed sub-table."""
    n = EPG + 5000
    ev = _head(events, n)  # keys < 50_000 < 2^16
    plan = _plan(5, _cap(n, 32, _rounds(n, EPG)), dense_bits=16)
    _check(_run(native, gpu_device, ev, plan, V_ONEPASS[R], EPG), _run(native, "cpu", ev, plan),
           _rounds(n, EPG))


@pytest.mark.parametrize("with_idx", [False, True])
def test_late_events(native, gpu_device, events, with_idx):
    """late_ts inside the data: the late count (and the side-output indices) equal the twin's,
    and late events cost no hole -- the bound of three per round holds with a third or more of
    the events dropped."""
    n = EPG + 5000
    ev = _head(events, n)
    plan = _plan(4, _cap(n, 16, _rounds(n, EPG)), late_ts=2200)  # ts of this slice: ~700 .. 4100
    cap = n if with_idx else None
    c = _run(native, "cpu", ev, plan, late_cap=cap)
    nlate = int(c["stats"][K.STAT_LATE])
    assert n // 4 < nlate < 3 * n // 4
    for variant, epg in ((V_ONEPASS[R], EPG), (None, 0)):
        g = _run(native, gpu_device, ev, plan, variant, epg, late_cap=cap)
        _check(g, c, max(_rounds(n, EPG), -(-n // 4096)))
        if with_idx:
            assert np.array_equal(np.sort(g["late"][:nlate]), np.sort(c["late"][:nlate]))
            assert np.all(g["late"][nlate:] == -1)


def test_misaligned_views(native, gpu_device, events):
    """keys[1:], ts[1:], vals[1:] are 8 bytes off a 16-byte boundary: the lane-strided
    instantiation, same multisets."""
    n = EPG + 2001
    big = tuple(x.to(gpu_device) for x in _head(events, n + 1))
    ev = tuple(x[1:] for x in big)
    assert all(x.data_ptr() % 16 == 8 for x in ev)
    plan = _plan(6, _cap(n, 64, _rounds(n, EPG)))
    c = _run(native, "cpu", _head(events, n, 1), plan)
    _check(_run(native, gpu_device, ev, plan, V_ONEPASS[R], EPG), c, _rounds(n, EPG))
    _check(_run(native, gpu_device, ev, plan), c, -(-n // 4096))


@pytest.mark.parametrize("cap,variant", [(64, V_ONEPASS[R]), (20_000, None)])
def test_one_hot_key_overflow(native, gpu_device, cap, variant):
    """Every event on one key, bucket_cap too small: the overflow bit is set, and neither the
    other buckets nor a sentinel tail behind `out` is written. cap 64: the first round already
    does not fit. cap 20000, production groups of 4096: the bucket fills, later groups overflow."""
    n = 40_000
    keys = torch.full((n,), 7, dtype=torch.int64)
    ts = torch.full((n,), 2000, dtype=torch.int64)
    vals = torch.arange(n, dtype=torch.int64) % 1000
    plan = _plan(3, cap)
    g = _run(native, gpu_device, (keys, ts, vals), plan, variant, 0, tail=4096, fill=SENTINEL)
    assert int(g["stats"][K.STAT_OVERFLOW]) & 1
    hot = int(np.argmax(g["cursor"]))
    assert g["cursor"][hot] >= n and np.all(np.delete(g["cursor"], hot) == 0)
    assert np.all(np.delete(g["recs"], hot, axis=0) == np.uint64(SENTINEL))
    assert np.all(g["rest"] == np.uint64(SENTINEL))
    written = g["recs"][hot][g["recs"][hot] != np.uint64(SENTINEL)]
    assert np.all((written & np.uint64(0xFFFFFFFF)) == np.uint64(7))  # only its own records


@pytest.mark.parametrize("what", ["value", "key"])
def test_width_misfits_flagged(native, gpu_device, events, what):
    """A value >= 2^27 or a key >= 2^32 does not fit the 8-byte record: the same flag bits as
    the two-pass kernel and the twin (the host then redoes the step with wider records)."""
    n = R + 100
    keys, ts, vals = (x.clone() for x in _head(events, n))
    if what == "value":
        vals[R // 2] = 1 << 27
    else:
        keys[R + 50] = (1 << 32) + 5
    plan = _plan(4, _cap(n, 16, 2))
    flags = [int(_run(native, d, (keys, ts, vals), plan, v)["stats"][K.STAT_OVERFLOW])
             for d, v in ((gpu_device, V_ONEPASS[R]), (gpu_device, V_TWOPASS), ("cpu", None))]
    assert flags[0] == flags[1] == flags[2] == 16


@pytest.mark.parametrize("key_dtype", [torch.int64, torch.int32])
def test_operator_end_to_end(gpu_device, key_dtype):
    """KeyedWindowOperator(dense_keys, narrow) over 6 steps of 64K events: the GPU's fired rows
    (int64 and int32 key columns) equal the C++ twin's."""

    def run(dev, dtype):
        op = KeyedWindowOperator(size=3000, slide=1000, agg=K.AGG_SUM_I64, device=dev,
                                 max_keys=20_000, batch_capacity=1 << 16, ooo_bound=400,
                                 dense_keys=True, narrow=dev != "cpu")
        rows = []
        for step in range(6):
            k = torch.empty(1 << 16, dtype=dtype, device=dev)
            t = torch.empty(1 << 16, dtype=torch.int64, device=dev)
            v = torch.empty_like(t)
            K.gen_events(k, t, v, seed=13, stream_id=0, idx0=step << 16, nkeys=18_000,
                         ts_base=step * 1000, ts_span=1000, disorder=400, val_lo=0,
                         val_span=5000)
            rows += op.process(k, t, v)
        rows += op.finish()
        return sorted((r.window_start, int(a), int(b), int(c))
                      for r in rows for a, b, c in zip(r.keys, r.raw, r.counts))

    assert run(gpu_device, key_dtype) == run("cpu", torch.int64)
