"""Lean front end of window_agg for 8-byte records vs the C++ twin (needs an MI355X).

K.window_agg folds hand-built 8-byte record buffers (key | (value << 4 | pane) << 32, hole =
all ones) on the GPU and with the twin; acc_g, cnt_g, dirty_g, flags (and the key tables) must be
equal bit for bit. The shapes are the ones the operator never produces on demand: segment counts
around the wave chunk of 512 records, holes at chunk edges, panes outside the step's rows, pane
groups, sparse pane rows, ids outside the dense space, unaligned segments and split shares.
Hashed cases start from the twin's key table, so no slot depends on an insertion race.
"""
import numpy as np
import pytest
import torch

from mxstream.ops import kernels as K
from mxstream.runtime.window_operator import KeyedWindowOperator

pytestmark = pytest.mark.gpu

CHUNK = 512                 # records a wave folds without a bounds check (csrc kLeanChunk)
HOLE = np.uint64(0xFFFFFFFFFFFFFFFF)
NSUB, CAP_LOG2, RING = 4, 6, 16
DENSE_BITS = 8              # nsub * cap = 256 dense ids
DENSE_MUL = 0x9E3779B1 & 0xFF | 1
PANE_BASE = 100


def _recs(rng, n, dense, tlo=0, thi=15, nkeys=None):
    """n live records: keys inside the dense space (or 40 hashed keys), values over the whole
    28-bit range, panes in [tlo, thi)."""
    if dense:
        key = rng.integers(0, nkeys or (1 << DENSE_BITS), n, dtype=np.uint64)
    else:
        key = rng.integers(0, nkeys or 40, n, dtype=np.uint64) * np.uint64(0x01000193) & np.uint64(0xFFFFFFFE)
    val = rng.integers(-(1 << 27), 1 << 27, n, dtype=np.int64)
    t = rng.integers(tlo, thi, n, dtype=np.uint64)
    return _pack(key, val, t)


def _pack(key, val, t):
    vt = ((np.asarray(val, dtype=np.int64) << 4).astype(np.uint64) | np.asarray(t, dtype=np.uint64)) \
        & np.uint64(0xFFFFFFFF)
    return np.asarray(key, dtype=np.uint64) | (vt << np.uint64(32))


def _plan(bucket_cap, dense, agg=K.AGG_SUM_I64, p_lo=0, np_step=15, pg=15, **kw):
    return K.AggPlan(cap_log2=CAP_LOG2, nsub=NSUB, ring=RING, agg=agg, nsrc=1,
                     bucket_cap=bucket_cap, np_step=np_step, pg=pg, pane_base=PANE_BASE, p_lo=p_lo,
                     fired_hi=PANE_BASE + 6, rec_words=1, dense_bits=DENSE_BITS if dense else 0,
                     dense_mul=DENSE_MUL if dense else 0, **kw)


def _fold(dev, segs, plan, keys0=None):
    """One window_agg call over segs (a list of NSUB uint64 arrays, one per sub-table) on state
    that already holds data (so the write-back combines)."""
    buf = np.full(NSUB * plan.bucket_cap * 3 + 2, HOLE, dtype=np.uint64)
    for b, s in enumerate(segs):
        buf[b * plan.bucket_cap:b * plan.bucket_cap + len(s)] = s
    recs = torch.from_numpy(buf.view(np.int64)).to(dev)
    counts = torch.tensor([len(s) for s in segs], dtype=torch.int32, device=dev)
    nslots = NSUB << CAP_LOG2
    keys = (torch.full((nslots,), -1, dtype=torch.int64) if keys0 is None else keys0.clone()).to(dev)
    g = torch.Generator().manual_seed(5)
    cnt = torch.randint(0, 3, (RING * nslots,), generator=g, dtype=torch.int32)
    acc = torch.randint(-1000, 1000, (RING * nslots,), generator=g, dtype=torch.int64) * (cnt > 0)
    acc, cnt = acc.to(dev), cnt.to(dev)
    dirty = torch.zeros(RING * nslots, dtype=torch.uint8, device=dev)
    occ = torch.zeros(NSUB, dtype=torch.int32, device=dev)
    flags = torch.zeros(1, dtype=torch.int32, device=dev)
    K.window_agg(recs, counts, plan, keys, acc, cnt, dirty, occ, flags)
    return dict(acc=acc.cpu(), cnt=cnt.cpu(), dirty=dirty.cpu(), flags=flags.cpu(),
                keys=keys.cpu(), occ=occ.cpu())


def _same(g, c, what=("acc", "cnt", "dirty", "flags", "keys")):
    for name in what:
        assert torch.equal(g[name], c[name]), name


def _check(gpu_device, segs, plan, dense, gpu_plan=None, flag=0):
    """GPU (gpu_plan, default plan) against the twin; hashed: on the twin's key table."""
    c0 = _fold("cpu", segs, plan)
    keys0 = None if dense else c0["keys"]
    c = c0 if dense else _fold("cpu", segs, plan, keys0)
    g = _fold(gpu_device, segs, gpu_plan or plan, keys0)
    _same(g, c)
    assert int(c["flags"][0]) == flag
    assert int(c["cnt"].sum()) > 0 or not any(len(s) for s in segs)
    return g


@pytest.fixture(scope="module")
def rng():
    return np.random.default_rng(11)


@pytest.mark.parametrize("dense", [True, False], ids=["dense", "hashed"])
@pytest.mark.parametrize("counts", [(0, 1, 3, 777), (CHUNK, CHUNK + 1, 19 * CHUNK + 77, 2 * CHUNK + 5),
                                    (16 * CHUNK, 17 * CHUNK, 33 * CHUNK - 1, 0)])
def test_segment_counts(gpu_device, rng, dense, counts):
    """Empty, tiny and odd segments, exactly one chunk, one chunk + 1, a chunk for each of the 16
    waves, a second round for some waves, and ragged tails -- different per sub-table."""
    segs = [_recs(rng, n, dense) for n in counts]
    _check(gpu_device, segs, _plan(33 * CHUNK, dense), dense)


@pytest.mark.parametrize("dense", [True, False], ids=["dense", "hashed"])
def test_holes(gpu_device, rng, dense):
    """A hole at every granule end (as the one-pass partition pads), a segment of holes only,
    and holes as the first and the last record of a chunk."""
    a = _recs(rng, 3 * CHUNK + 100, dense)
    a[3::4] = HOLE
    b = np.full(2 * CHUNK + 4, HOLE, dtype=np.uint64)
    c = _recs(rng, 18 * CHUNK, dense)
    for k in (0, 1, 16, 17):
        c[k * CHUNK] = HOLE
        c[k * CHUNK + CHUNK - 1] = HOLE
    _check(gpu_device, [a, b, c, _recs(rng, 9, dense)], _plan(18 * CHUNK, dense), dense)


@pytest.mark.parametrize("dense", [True, False], ids=["dense", "hashed"])
@pytest.mark.parametrize("pg", [4, 2, 3])
def test_pane_rows(gpu_device, rng, dense, pg):
    """Records of panes 0..14, rows 3..6 in the step: the others are skipped. pg 2 and 3 fold
    the four rows in two pane groups (3: the second group is a partial one)."""
    segs = [_recs(rng, n, dense) for n in (3 * CHUNK + 9, 2 * CHUNK, 700, 17 * CHUNK + 3)]
    _check(gpu_device, segs, _plan(18 * CHUNK, dense, p_lo=3, np_step=4, pg=pg), dense)


@pytest.mark.parametrize("dense", [True, False], ids=["dense", "hashed"])
@pytest.mark.parametrize("pg", [3, 2])
def test_sparse_pane_rows(gpu_device, rng, dense, pg):
    """Sparse rows (pmask = panes 1, 4 and 14, the highest a record can carry) equal the dense
    range [1, 15) of the twin; pg 2: two pane groups."""
    panes = np.array([1, 4, 14], dtype=np.uint64)
    segs = []
    for n in (2 * CHUNK + 31, 17 * CHUNK, 5, CHUNK):
        r = _recs(rng, n, dense)
        t = panes[rng.integers(0, 3, n)]
        segs.append(r & ~np.uint64(15 << 32) | (t << np.uint64(32)))
    plan = _plan(17 * CHUNK, dense, p_lo=1, np_step=14, pg=14)
    sparse = _plan(17 * CHUNK, dense, p_lo=1, np_step=3, pg=pg, pmask=1 << 1 | 1 << 4 | 1 << 14)
    _check(gpu_device, segs, plan, dense, gpu_plan=sparse)


def test_dense_key_outside_range(gpu_device, rng):
    """One id >= 2^dense_bits in the middle of a chunk: the overflow flag is set, that record is
    dropped and its neighbours are kept. A second one in a pane outside the step sets nothing."""
    a = _recs(rng, 2 * CHUNK, True, tlo=3, thi=7)
    a[CHUNK + 200] = _pack(1 << DENSE_BITS | 5, 77, 4)
    b = _recs(rng, 2 * CHUNK, True, tlo=3, thi=7)
    b[100] = _pack(1 << 31, 1, 9)
    plan = _plan(2 * CHUNK, True, p_lo=3, np_step=4, pg=4)
    _check(gpu_device, [a, b[:CHUNK], b[:7], b[:0]], plan, True, flag=1)
    _check(gpu_device, [b, b, b, b], plan, True, flag=0)


@pytest.mark.parametrize("dense", [True, False], ids=["dense", "hashed"])
def test_odd_bucket_cap(gpu_device, rng, dense):
    """bucket_cap odd: the odd sub-tables start 8 bytes off a 16-byte boundary and take the
    8-byte loads."""
    segs = [_recs(rng, n, dense) for n in (3 * CHUNK + 1, 3 * CHUNK + 1, 17 * CHUNK, 17 * CHUNK)]
    _check(gpu_device, segs, _plan(17 * CHUNK + 1, dense), dense)


@pytest.mark.parametrize("half", [5 * CHUNK + 1, 5 * CHUNK])
def test_split_shares(gpu_device, rng, half):
    """Two workgroups per sub-table (forced split): the second share starts at record `half`,
    odd (8-byte loads) or even (its own chunks)."""
    segs = [_recs(rng, n, True) for n in (2 * half, 2 * half, 2, 2 * CHUNK)]
    plan = _plan(2 * half, True)
    _check(gpu_device, segs, plan, True, gpu_plan=_plan(2 * half, True, split=-2))


def test_hashed_insert_into_nearly_full_table(gpu_device, rng):
    """62 of a sub-table's 64 slots taken; one new key arrives inside a chunk: it is inserted
    where the twin inserts it, and the occupancy is reported."""
    old = [_recs(rng, 2 * CHUNK, False, nkeys=62) for _ in range(NSUB)]
    plan = _plan(2 * CHUNK, False)
    keys0 = _fold("cpu", old, plan)["keys"]
    assert all(int((keys0.view(NSUB, -1)[b] != -1).sum()) == 62 for b in range(NSUB))
    new = [s.copy() for s in old]
    new[1][CHUNK + 17] = _pack(0xABCDEF01, -5, 2)
    new[2][3] = _pack(0xABCDEF01, 9, 14)
    c = _fold("cpu", new, plan, keys0)
    g = _fold(gpu_device, new, plan, keys0)
    _same(g, c, ("acc", "cnt", "dirty", "flags", "keys", "occ"))
    assert c["occ"].tolist() == [0, 63, 63, 0]


@pytest.mark.parametrize("agg", [K.AGG_AVG_I64, K.AGG_MIN_I64, K.AGG_MAX_I64, K.AGG_COUNT])
def test_other_aggregates(gpu_device, rng, agg):
    """The other integer aggregates through the same front end (AVG: the packed word)."""
    segs = [_recs(rng, n, True) for n in (3 * CHUNK + 9, 17 * CHUNK, 700, 0)]
    _check(gpu_device, segs, _plan(17 * CHUNK, True, agg=agg), True)


def _operator_rows(dev):
    op = KeyedWindowOperator(size=3000, slide=1000, agg=K.AGG_SUM_I64, device=dev,
                             max_keys=20_000, batch_capacity=1 << 16, ooo_bound=400,
                             dense_keys=True, narrow=dev != "cpu")
    rows = []
    for step in range(6):
        k = torch.empty(1 << 16, dtype=torch.int64, device=dev)
        t = torch.empty_like(k)
        v = torch.empty_like(k)
        K.gen_events(k, t, v, seed=13, stream_id=0, idx0=step << 16, nkeys=18_000,
                     ts_base=step * 1000, ts_span=1000, disorder=400, val_lo=0, val_span=5000)
        rows += op.process(k, t, v)
    rows += op.finish()
    return sorted((r.window_start, int(a), int(b), int(c))
                  for r in rows for a, b, c in zip(r.keys, r.raw, r.counts))


@pytest.fixture(scope="module")
def operator_cpu_rows():
    return _operator_rows("cpu")


@pytest.mark.parametrize("lean", ["1", "0"])
def test_operator_lean_on_and_off(gpu_device, operator_cpu_rows, monkeypatch, lean):
    """KeyedWindowOperator, dense keys, 8-byte records, six steps of 2^16 events: with
    MXS_AGG_LEAN on and off the fired rows equal the twin's (the switch is read per launch)."""
    monkeypatch.setenv("MXS_AGG_LEAN", lean)
    assert _operator_rows(gpu_device) == operator_cpu_rows


@pytest.mark.parametrize("dense", [True, False], ids=["dense", "hashed"])
def test_lean_off_is_the_same_fold(gpu_device, rng, dense, monkeypatch):
    """MXS_AGG_LEAN=0 (the per-record loop alone) on chunked and ragged segments."""
    monkeypatch.setenv("MXS_AGG_LEAN", "0")
    segs = [_recs(rng, n, dense) for n in (3 * CHUNK + 9, 17 * CHUNK, 700, 0)]
    _check(gpu_device, segs, _plan(17 * CHUNK, dense), dense)
