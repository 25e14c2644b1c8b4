"""Kernel-level tests of the vector-metric window kernels through ``mxstream.ops.vector``
(csrc/vector_hip.hip: vec_window_agg_kernel<MODE, RW>, vec_window_fire_kernel, vec_gather_kernel;
csrc/vector_cpu.cpp: the C++ twins).

Every case runs on the CPU twin (unmarked) and on the GPU (``gpu`` mark; the aggregation in both
MODE_MFMA and MODE_VALU), against a plain numpy float64 reference of the same operation. The
record packing, the reference and every bound are therefore proven on a machine without a GPU.

Tolerances are derived, not measured:

* aggregation, a cell with ``c`` records: ``(c + 3) * 2^-24 * sum|v_i| + 3 * c * 2^-126``. The
  first term bounds an f32 sum of c values in any order and any tree (the per-run partial sums and
  their flush atomics included); the second covers bf16 split terms below FLT_MIN, which the matrix
  cores may flush.
* fire, over ``npanes`` pane accumulators: ``(npanes + 1) * 2^-24 * sum|acc| / cnt`` plus one ulp
  of the result (the division).
* counts, keys, dirty bytes, flags and occupancy are exact.
"""
import numpy as np
import pytest
import torch

from mxstream.ops import vector as V

U = 2.0 ** -24
TINY = 2.0 ** -126
HOLE = 0xFFFFFFFF
EMPTY = -1
OCC_SENTINEL = 0x5A5A5A

AGG_TARGETS = [
    pytest.param(("cpu", V.MODE_MFMA), id="cpu"),
    pytest.param(("cuda", V.MODE_MFMA), id="gpu-mfma", marks=pytest.mark.gpu),
    pytest.param(("cuda", V.MODE_VALU), id="gpu-valu", marks=pytest.mark.gpu),
]
DEVICES = [pytest.param("cpu", id="cpu"), pytest.param("cuda", id="gpu", marks=pytest.mark.gpu)]


def _device(name):
    if name == "cuda":
        if not torch.cuda.is_available():
            pytest.skip("no GPU")
        return torch.device("cuda", 0)
    return torch.device("cpu")


# ---- helpers ---------------------------------------------------------------------------------
def pack_recs(keys, rows, t, rec_words):
    """int64 record words [n, rec_words]. 3: (key, val, t | aux << 32); 2: (key, val | t << 32).
    val is the record's vector row; a hole is t = 0xFFFFFFFF."""
    keys = np.asarray(keys, dtype=np.int64).view(np.uint64)
    rows = np.asarray(rows, dtype=np.uint64)
    t = np.asarray(t, dtype=np.uint64)
    out = np.zeros((len(keys), rec_words), dtype=np.uint64)
    out[:, 0] = keys
    if rec_words == 3:
        aux = (np.arange(len(keys), dtype=np.uint64) * np.uint64(2654435761)) & np.uint64(HOLE)
        out[:, 1] = rows
        out[:, 2] = t | (aux << np.uint64(32))
    else:
        out[:, 1] = rows | (t << np.uint64(32))
    return out.view(np.int64)


def ref_agg(keys, t, x, p_lo, np_step):
    """{(pane, key): (sum[D] f64, sum|v|[D] f64, count)} of the records (keys[i], t[i], x[i]):
    holes and panes outside [p_lo, p_lo + np_step) are skipped."""
    keys, t = np.asarray(keys, dtype=np.int64), np.asarray(t, dtype=np.int64)
    ok = (t != HOLE) & (t >= p_lo) & (t < p_lo + np_step)
    k, tt, xv = keys[ok], t[ok], np.asarray(x)[ok].astype(np.float64)
    out = {}
    with np.errstate(invalid="ignore", over="ignore"):
        for pt, pk in {(int(a), int(b)) for a, b in zip(tt, k)}:
            sel = (tt == pt) & (k == pk)
            out[(pt, pk)] = (xv[sel].sum(0), np.abs(xv[sel]).sum(0), int(sel.sum()))
    return out


def agg_bound(sumabs, c):
    return (c + 3) * U * sumabs + 3 * c * TINY


def _within(got, ref, bound):
    """Finite reference: |got - ref| <= bound. Non-finite reference: the same IEEE class."""
    got = np.asarray(got, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        same = (np.isnan(ref) & np.isnan(got)) | (got == ref)
        near = np.abs(got - ref) <= bound
    return np.where(np.isfinite(ref), near, same)


class Bucket:
    """Records of one (source, sub-table) bucket, in bucket order."""

    def __init__(self, keys=(), t=(), x=None, dim=32):
        self.keys = np.asarray(keys, dtype=np.int64)
        self.t = np.asarray(t, dtype=np.int64)
        self.x = (np.zeros((0, dim), np.float32) if x is None else np.asarray(x, np.float32))
        assert len(self.keys) == len(self.t) == len(self.x)


class AggHarness:
    """Window state of one aggregation target plus the cumulative float64 expectation."""

    def __init__(self, target, *, dim=32, ring=8, cap_log2=6, nsub=1, occ_fill=OCC_SENTINEL):
        dev_name, self.mode = target
        self.dev = _device(dev_name)
        self.dim, self.ring, self.cap_log2, self.nsub = dim, ring, cap_log2, nsub
        self.cap = 1 << cap_log2
        self.nslots = nsub << cap_log2
        d = self.dev
        self.keys_g = torch.full((self.nslots,), EMPTY, dtype=torch.int64, device=d)
        self.acc_g = torch.zeros(ring * self.nslots * dim, dtype=torch.float32, device=d)
        self.cnt_g = torch.zeros(ring * self.nslots, dtype=torch.int32, device=d)
        self.dirty_g = torch.zeros(ring * self.nslots, dtype=torch.uint8, device=d)
        self.occ = torch.full((nsub,), occ_fill, dtype=torch.int32, device=d)
        self.flags = torch.zeros(1, dtype=torch.int32, device=d)
        self.cells = {}                      # (ring row, key) -> [sum, sumabs, count, dirty]
        self.known = [set() for _ in range(nsub)]
        self.exp_occ = [occ_fill] * nsub
        self.rng = np.random.default_rng(1234)

    def fill_occ(self, v):
        self.occ.fill_(v)
        self.exp_occ = [v] * self.nsub

    def agg(self, buckets, *, nsrc=1, bucket_cap=None, counts=None, positional=1, rec_words=3,
            p_lo=0, np_step=1, pane_base=0, fired_hi=-(1 << 62)):
        """buckets[src * nsub + sub]: Bucket. Launches the kernel and folds the same records into
        the expectation. ``counts`` overrides the per-bucket record counts (clamp case)."""
        nb = nsrc * self.nsub
        assert len(buckets) == nb
        D = self.dim
        bcap = bucket_cap or max(1, max(len(b.keys) for b in buckets))
        # Unused record slots and vector rows hold live-looking garbage: a record read past its
        # bucket's count would be aggregated and seen.
        recs = np.empty((nb * bcap, rec_words), dtype=np.int64)
        recs[:] = pack_recs([0x7777777], [0], [p_lo], rec_words)[0]
        nvec = nb * bcap if positional else nb * bcap + 13
        vec = np.full((nvec, D), 1.0e30, dtype=np.float32)
        perm = self.rng.permutation(nvec)
        cnts = np.zeros(nb, dtype=np.int64)
        for b, bk in enumerate(buckets):
            n = len(bk.keys)
            assert n <= bcap
            pos = b * bcap + np.arange(n)
            rows = pos if positional else perm[pos]
            vec[rows] = bk.x
            # positional: the record's value field is not a row; make it one that would be wrong
            val = (rows + 1) % nvec if positional else rows
            recs[pos] = pack_recs(bk.keys, val, bk.t & HOLE, rec_words)
            cnts[b] = n
        given = cnts if counts is None else np.asarray(counts, dtype=np.int64)
        plan = V.VecAggPlan(cap_log2=self.cap_log2, nsub=self.nsub, ring=self.ring, dim=D,
                            nsrc=nsrc, bucket_cap=bcap, np_step=np_step, positional=positional,
                            rec_words=rec_words, mode=self.mode, pane_base=pane_base, p_lo=p_lo,
                            fired_hi=fired_hi)
        d = self.dev
        V.vec_window_agg(torch.from_numpy(recs.reshape(-1)).to(d),
                         torch.from_numpy(given.astype(np.uint32).view(np.int32)).to(d), plan,
                         torch.from_numpy(vec).to(d), self.keys_g, self.acc_g, self.cnt_g,
                         self.dirty_g, self.occ, self.flags)
        # expectation
        for b, bk in enumerate(buckets):
            sub = b % self.nsub
            n = min(int(given[b]), bcap)
            assert n <= len(bk.keys)
            ref = ref_agg(bk.keys[:n], bk.t[:n], bk.x[:n], p_lo, np_step)
            new = {k for _, k in ref} - self.known[sub]
            for (pt, k), (s, sa, c) in ref.items():
                row = (pane_base + pt) & (self.ring - 1)
                cell = self.cells.setdefault((row, k), [np.zeros(D), np.zeros(D), 0, 0, sub])
                with np.errstate(invalid="ignore", over="ignore"):
                    cell[0] = cell[0] + s
                    cell[1] = cell[1] + sa
                cell[2] += c
                if pane_base + pt <= fired_hi:
                    cell[3] = 1
            if new:
                self.known[sub] |= new
                self.exp_occ[sub] = min(len(self.known[sub]), self.cap)

    def check(self, overflow=False):
        D, ns = self.dim, self.nslots
        keys_g = self.keys_g.cpu().numpy()
        acc = self.acc_g.cpu().numpy().reshape(self.ring, ns, D)
        cnt = self.cnt_g.cpu().numpy().reshape(self.ring, ns)
        dirty = self.dirty_g.cpu().numpy().reshape(self.ring, ns)
        stored = {}
        for s in np.nonzero(keys_g != EMPTY)[0]:
            assert int(keys_g[s]) not in stored, "key stored twice"
            stored[int(keys_g[s])] = int(s)
        want = set().union(*self.known)
        if overflow:
            assert int(self.flags.item()) & 1
            assert set(stored) <= want and len(stored) == self.cap
        else:
            assert int(self.flags.item()) == 0
            assert set(stored) == want
        for sub, ks in enumerate(self.known):
            for k in ks & set(stored):
                assert stored[k] >> self.cap_log2 == sub, "key outside its sub-table"
        assert self.occ.cpu().tolist() == self.exp_occ
        exp = np.zeros((self.ring, ns, D))
        bound = np.zeros((self.ring, ns, D))
        exp_cnt = np.zeros((self.ring, ns), dtype=np.int64)
        exp_dirty = np.zeros((self.ring, ns), dtype=np.uint8)
        for (row, k), (s, sa, c, dflag, _sub) in self.cells.items():
            if k not in stored:
                assert overflow
                continue
            with np.errstate(invalid="ignore", over="ignore"):
                exp[row, stored[k]], bound[row, stored[k]] = s, agg_bound(sa, c)
            exp_cnt[row, stored[k]], exp_dirty[row, stored[k]] = c, dflag
        assert np.array_equal(cnt, exp_cnt)
        assert np.array_equal(dirty, exp_dirty)
        ok = _within(acc, exp, bound)   # untouched cells: bound 0, exactly 0.0
        if not ok.all():
            bad = np.argwhere(~ok)[0]
            raise AssertionError(f"acc[row {bad[0]}, slot {bad[1]}, metric {bad[2]}] = "
                                 f"{acc[tuple(bad)]!r}, want {exp[tuple(bad)]!r} +- "
                                 f"{bound[tuple(bad)]!r} ({int((~ok).sum())} cells off)")


def _values(rng, n, dim):
    return rng.uniform(-50.0, 100.0, size=(n, dim)).astype(np.float32)


# ---- aggregation -----------------------------------------------------------------------------
@pytest.mark.parametrize("target", AGG_TARGETS)
@pytest.mark.parametrize("pattern", ["one_key", "distinct", "runs3"])
@pytest.mark.parametrize("nrec", [1, 31, 32, 33, 64, 65, 95])
def test_agg_tile_edges(target, pattern, nrec):
    """Tiles of exactly 1, 31, 32, 33 ... records; one run over all tiles, 32 distinct segments
    per tile, and runs of three (sorted records 30-32 are one key across the tile edge)."""
    rng = np.random.default_rng(nrec)
    keys = {"one_key": np.full(nrec, 900), "distinct": 1000 + 17 * np.arange(nrec),
            "runs3": 500 + np.arange(nrec) // 3}[pattern]
    keys = keys[rng.permutation(nrec)]
    h = AggHarness(target, cap_log2=7 if pattern == "distinct" else 6)
    h.agg([Bucket(keys, np.zeros(nrec), _values(rng, nrec, 32))])
    h.check()


@pytest.mark.parametrize("target", AGG_TARGETS)
@pytest.mark.parametrize("positional", [0, 1])
@pytest.mark.parametrize("rec_words", [2, 3])
@pytest.mark.parametrize("dim", [32, 64, 128, 256])
def test_agg_shapes(target, dim, rec_words, positional):
    rng = np.random.default_rng(dim + rec_words)
    n = 200
    h = AggHarness(target, dim=dim)
    h.agg([Bucket(3000 + rng.integers(0, 40, n), rng.integers(0, 2, n), _values(rng, n, dim))],
          positional=positional, rec_words=rec_words, np_step=2)
    h.check()


@pytest.mark.parametrize("target", AGG_TARGETS)
def test_agg_rounds_and_clamp(target):
    """More than one LDS round (c > 16384), counts > bucket_cap clamped, runs of ~1000 records
    across tiles and the round boundary."""
    rng = np.random.default_rng(3)
    bcap = 16384 + 40
    keys = 70 + np.sort(rng.integers(0, 16, bcap))   # long runs also in arrival order
    h = AggHarness(target)
    bk = Bucket(keys, np.zeros(bcap), _values(rng, bcap, 32))
    # counts[0] is past the bucket: the expectation folds min(count, bucket_cap) records
    h.agg([bk], bucket_cap=bcap, counts=[bcap + 1000])
    assert sum(c[2] for c in h.cells.values()) == bcap
    h.check()


@pytest.mark.parametrize("target", AGG_TARGETS)
@pytest.mark.parametrize("cap_log2", [11, 12])
def test_agg_pane_groups(target, cap_log2):
    """np_step = 3 with one (cap 2^12) or two (cap 2^11: uneven last group) panes per group;
    t = 4 and 8 are outside [5, 8); ring 4 with pane_base -6 wraps through negative panes."""
    rng = np.random.default_rng(cap_log2)
    n = 300
    h = AggHarness(target, cap_log2=cap_log2, ring=4)
    h.agg([Bucket(rng.integers(1, 50, n) * 7919, rng.integers(4, 9, n), _values(rng, n, 32))],
          p_lo=5, np_step=3, pane_base=-6)
    assert {r for r, _ in h.cells} == {3, 0, 1}
    h.check()


@pytest.mark.parametrize("target", AGG_TARGETS)
def test_agg_sources_and_subtables(target):
    rng = np.random.default_rng(5)
    nsrc, nsub, bcap = 3, 4, 40
    sizes = [40, 0, 17, 33, 0, 0, 1, 40, 25, 0, 32, 9]
    buckets = []
    for b, n in enumerate(sizes):
        sub = b % nsub
        buckets.append(Bucket(10_000 * (sub + 1) + rng.integers(0, 12, n), rng.integers(0, 2, n),
                              _values(rng, n, 32)))
    h = AggHarness(target, nsub=nsub)
    h.agg(buckets, nsrc=nsrc, bucket_cap=bcap, np_step=2, rec_words=2)
    h.check()
    assert h.exp_occ[1] == OCC_SENTINEL   # sub-table 1 has no record in any source


@pytest.mark.parametrize("target", AGG_TARGETS)
def test_agg_existing_state(target):
    """Second call on the same state: accumulators add up; occupancy is written only for the
    sub-tables that inserted a key."""
    rng = np.random.default_rng(6)
    nsub = 4

    def bucket(sub, ids, n):   # every id at least once
        return Bucket(10_000 * (sub + 1) + ids[rng.permutation(n) % len(ids)],
                      rng.integers(0, 2, n), _values(rng, n, 32))

    h = AggHarness(target, nsub=nsub)
    h.agg([bucket(s, np.arange(10), 50) for s in range(nsub)], np_step=2)
    h.check()
    assert h.exp_occ == [10] * nsub
    h.fill_occ(OCC_SENTINEL)
    h.agg([bucket(0, np.arange(10), 45),           # known keys only
           bucket(1, np.arange(20, 25), 30),       # new keys only
           Bucket(),                               # nothing
           bucket(3, np.arange(5, 15), 60)],       # both
          np_step=2)
    assert h.exp_occ[0] == h.exp_occ[2] == OCC_SENTINEL and h.exp_occ[1] == h.exp_occ[3] == 15
    h.check()


@pytest.mark.parametrize("target", AGG_TARGETS)
def test_agg_table_overflow(target):
    """70 distinct keys into a 64-slot sub-table: flags[0] bit 0, exactly 64 keys stored, every
    stored key complete. Which keys drop depends on the order and is not asserted."""
    rng = np.random.default_rng(7)
    keys = np.repeat(40_000 + 3 * np.arange(70), 2)[rng.permutation(140)]
    h = AggHarness(target)
    h.agg([Bucket(keys, np.zeros(140), _values(rng, 140, 32))])
    h.check(overflow=True)


@pytest.mark.parametrize("target", AGG_TARGETS)
def test_agg_dirty(target):
    """fired_hi in the middle of the step's panes: exactly the touched cells of panes <= fired_hi
    are marked."""
    rng = np.random.default_rng(8)
    n = 150
    h = AggHarness(target)
    h.agg([Bucket(rng.integers(0, 30, n) + 1, rng.integers(0, 3, n), _values(rng, n, 32))],
          np_step=3, pane_base=10, fired_hi=11)
    assert sorted({(r, c[3]) for (r, _), c in h.cells.items()}) == [(2, 1), (3, 1), (4, 0)]
    h.check()


@pytest.mark.parametrize("target", AGG_TARGETS)
def test_agg_numerics(target):
    """Wide dynamic range, exact cancellations and subnormal-range inputs: a dropped split term
    or a bf16-rounded input is far outside the f32 summation bound."""
    rng = np.random.default_rng(9)
    n, nk, D = 64, 8, 32
    keys = np.arange(n) % nk + 11
    x = (10.0 ** rng.uniform(-3, 8, (n, D)) * rng.choice([-1.0, 1.0], (n, D))).astype(np.float32)
    # metrics 10..19: each key's 8 records are three pairs (x, -x), one small value and a zero:
    # the exact sum is the small value
    for k in range(nk):
        idx = rng.permutation(np.nonzero(keys == k + 11)[0])
        assert len(idx) == 8
        big = (10.0 ** rng.uniform(2, 7, (3, 10))).astype(np.float32)
        x[idx[0:6:2], 10:20] = big
        x[idx[1:6:2], 10:20] = -big
        x[idx[6], 10:20] = rng.uniform(1e-3, 1e-2, 10).astype(np.float32)
        x[idx[7], 10:20] = 0.0
    # metrics 20..25: 1e-40 .. 1e-36 (f32 subnormals and the smallest normals)
    x[:, 20:26] = (10.0 ** rng.uniform(-40, -36, (n, 6))).astype(np.float32)
    h = AggHarness(target)
    h.agg([Bucket(keys, np.zeros(n), x)])
    h.check()


@pytest.mark.parametrize("target", AGG_TARGETS)
@pytest.mark.parametrize("dim,off", [(32, 0), (64, 32)])
def test_agg_nonfinite_isolation(target, dim, off):
    """One key carries NaN, +Inf, +Inf and -Inf, and 3.4e38 (bf16 rounds it to Inf). All 24
    records share one 32-record tile. Its cells have the IEEE class of the f32 sum; every cell of
    every other key stays within the bound."""
    rng = np.random.default_rng(10 + off)
    n, nk = 24, 6
    keys = np.arange(n) % nk + 100
    x = _values(rng, n, dim)
    own = np.nonzero(keys == 102)[0]
    x[own[0], off + 3] = np.nan
    x[own[1], off + 5] = np.inf
    x[own[0], off + 7] = np.inf
    x[own[2], off + 7] = -np.inf
    x[own[1], off + 9] = 3.4e38
    h = AggHarness(target, dim=dim)
    h.agg([Bucket(keys, np.zeros(n), x)])
    s = h.cells[(0, 102)][0]
    assert np.isnan(s[off + 3]) and s[off + 5] == np.inf and np.isnan(s[off + 7])
    assert np.isfinite(s[off + 9]) and np.isfinite(np.delete(s, [off + 3, off + 5, off + 7])).all()
    assert all(np.isfinite(c[0]).all() for (_, k), c in h.cells.items() if k != 102)
    h.check()


# ---- fire ------------------------------------------------------------------------------------
def _fire_state(rng, nslots, ring, dim):
    keys = (rng.permutation(4 * nslots)[:nslots] + 1).astype(np.int64)
    keys[rng.random(nslots) < 0.3] = EMPTY
    cnt = rng.integers(0, 4, (ring, nslots)).astype(np.int32)
    cnt[rng.random((ring, nslots)) < 0.4] = 0
    acc = rng.uniform(-50.0, 100.0, (ring, nslots, dim)).astype(np.float32) * cnt[:, :, None]
    # never-written or purged cells: the accumulator is whatever was there
    junk = np.where(rng.random((ring, nslots, dim)) < 0.5, np.float32(1e30), np.float32(np.nan))
    acc = np.where((cnt == 0)[:, :, None], junk, acc).astype(np.float32)
    # a pane is marked dirty only together with an element (csrc/vector_hip.hip, step 2)
    dirty = ((rng.random((ring, nslots)) < 0.4) & (cnt > 0)).astype(np.uint8)
    return keys, acc, cnt, dirty


def ref_fire(keys, acc, cnt, dirty, *, ring, p0, npanes, avg, only_dirty):
    """{key: (result[D] f64, bound[D], count)} of the windows the fire kernel must emit without
    a threshold."""
    rows = [(p0 + q) & (ring - 1) for q in range(npanes)]
    out = {}
    for s in np.nonzero(keys != EMPTY)[0]:
        c = int(cnt[rows, s].sum())
        if c == 0 or (only_dirty and not dirty[rows, s].any()):
            continue
        live = [r for r in rows if cnt[r, s]]
        a = acc[live, s].astype(np.float64)
        div = c if avg else 1
        res = a.sum(0) / div
        bound = (npanes + 1) * U * np.abs(a).sum(0) / div + np.spacing(np.abs(res).astype(np.float32))
        out[int(keys[s])] = (res, bound, c)
    return out


def _launch_fire(dev, state, *, dim, ring, p0, npanes, avg, only_dirty, threshold, out_cap,
                 slack=8):
    keys, acc, cnt, dirty = state
    SENT_K, SENT_C = -77, -5
    ok = torch.full((out_cap + slack,), SENT_K, dtype=torch.int64, device=dev)
    ov = torch.full(((out_cap + slack) * dim,), -12345.0, dtype=torch.float32, device=dev)
    oc = torch.full((out_cap + slack,), SENT_C, dtype=torch.int32, device=dev)
    on = torch.zeros(1, dtype=torch.int32, device=dev)
    V.vec_window_fire(torch.from_numpy(keys).to(dev), torch.from_numpy(acc.reshape(-1)).to(dev),
                      torch.from_numpy(cnt.reshape(-1)).to(dev),
                      torch.from_numpy(dirty.reshape(-1)).to(dev), dim=dim, npanes=npanes,
                      ring=ring, p0=p0, only_dirty=only_dirty, avg=avg, threshold=threshold,
                      out_keys=ok[:out_cap], out_vec=ov, out_cnt=oc, out_n=on)
    ok, ov, oc = ok.cpu().numpy(), ov.cpu().numpy().reshape(-1, dim), oc.cpu().numpy()
    n = int(on.item())
    w = min(n, out_cap)
    # nothing at or beyond the written rows / out_cap
    assert (ok[w:] == SENT_K).all() and (oc[w:] == SENT_C).all() and (ov[w:] == -12345.0).all()
    return n, ok[:w], ov[:w], oc[:w]


def _check_fire_rows(ok, ov, oc, want, complete):
    assert len(set(ok.tolist())) == len(ok), "a key emitted twice"
    if complete:
        assert set(ok.tolist()) == set(want)
    for k, v, c in zip(ok.tolist(), ov, oc.tolist()):
        assert k in want, k
        res, bound, cw = want[k]
        assert c == cw, k
        assert _within(v, res, bound).all(), k


def _pick_threshold(ref):
    """A threshold that no reference maximum is within its tolerance of: the middle of the widest
    gap between the sorted maxima of the middle half."""
    mx = np.array(sorted(r.max() for r, _, _ in ref.values()))
    lo, hi = len(mx) // 4, max(len(mx) // 4 + 2, 3 * len(mx) // 4)
    gaps = np.diff(mx[lo:hi])
    i = lo + int(np.argmax(gaps))
    thr = float(np.float32((mx[i] + mx[i + 1]) / 2))
    for r, b, _ in ref.values():   # asserted on the reference alone
        assert abs(r.max() - thr) > b.max()
    return thr


def _fire_case(dev_name, *, nslots, dim, npanes, avg, only_dirty, seed):
    dev = _device(dev_name)
    rng = np.random.default_rng(seed)
    ring = 4
    state = _fire_state(rng, nslots, ring, dim)
    p0 = 7 if npanes > 1 else 2     # rows 3, 0, 1: the window wraps the ring
    kw = dict(dim=dim, ring=ring, p0=p0, npanes=npanes, avg=avg, only_dirty=only_dirty)
    ref = ref_fire(*state, ring=ring, p0=p0, npanes=npanes, avg=avg, only_dirty=only_dirty)
    assert len(ref) >= 8
    n, ok, ov, oc = _launch_fire(dev, state, threshold=None, out_cap=nslots, **kw)
    assert n == len(ref)
    _check_fire_rows(ok, ov, oc, ref, complete=True)
    thr = _pick_threshold(ref)
    want = {k: v for k, v in ref.items() if v[0].max() > thr}
    assert 0 < len(want) < len(ref)
    n, ok, ov, oc = _launch_fire(dev, state, threshold=thr, out_cap=nslots, **kw)
    assert n == len(want)
    _check_fire_rows(ok, ov, oc, want, complete=True)
    return state, ref, kw


@pytest.mark.parametrize("dev_name", DEVICES)
@pytest.mark.parametrize("only_dirty", [False, True])
@pytest.mark.parametrize("avg", [False, True])
@pytest.mark.parametrize("npanes", [1, 3])
@pytest.mark.parametrize("dim", [32, 256])
def test_fire_modes(dev_name, dim, npanes, avg, only_dirty):
    _fire_case(dev_name, nslots=320, dim=dim, npanes=npanes, avg=avg, only_dirty=only_dirty,
               seed=dim + npanes)


@pytest.mark.parametrize("dev_name", DEVICES)
@pytest.mark.parametrize("nslots", [64, 192, 320, 4096])
def test_fire_slot_counts(dev_name, nslots):
    """Less than one 256-slot iteration, a partial one, two, and several workgroups."""
    _fire_case(dev_name, nslots=nslots, dim=64, npanes=3, avg=True, only_dirty=False, seed=nslots)


@pytest.mark.parametrize("dev_name", DEVICES)
def test_fire_out_cap_overflow(dev_name):
    dev = _device(dev_name)
    rng = np.random.default_rng(21)
    ring, nslots, dim = 4, 320, 32
    state = _fire_state(rng, nslots, ring, dim)
    kw = dict(dim=dim, ring=ring, p0=7, npanes=3, avg=True, only_dirty=False)
    ref = ref_fire(*state, **{k: v for k, v in kw.items() if k != "dim"})
    cap = len(ref) // 2
    n, ok, ov, oc = _launch_fire(dev, state, threshold=None, out_cap=cap, **kw)
    assert n == len(ref)            # out_n counts every live row
    assert len(ok) == cap           # and _launch_fire saw nothing written from out_cap on
    _check_fire_rows(ok, ov, oc, ref, complete=False)


# ---- gather ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dev_name", DEVICES)
@pytest.mark.parametrize("rec_words", [2, 3])
@pytest.mark.parametrize("dim", [32, 256])
def test_gather(dev_name, dim, rec_words):
    dev = _device(dev_name)
    rng = np.random.default_rng(dim + rec_words)
    nb, bcap, nvec = 5, 48, 300
    counts = np.array([0, 1, 47, 48, 20], dtype=np.int32)
    rows = rng.integers(0, nvec, nb * bcap)
    t = rng.integers(0, 5, nb * bcap)
    t[rng.random(nb * bcap) < 0.2] = HOLE
    t[bcap] = 0  # the single record of bucket 1 is live
    recs = pack_recs(rng.integers(1, 1000, nb * bcap), rows, t, rec_words)
    vec = rng.integers(-2**31, 2**31, (nvec, dim)).astype(np.int32)   # any bit pattern
    SENT = 0x7FC0BEEF
    out = torch.full((nb * bcap, dim), SENT, dtype=torch.int32, device=dev)
    V.vec_gather(torch.from_numpy(recs.reshape(-1)).to(dev), rec_words,
                 torch.from_numpy(counts).to(dev), nb, bcap,
                 torch.from_numpy(vec).to(dev).view(torch.float32), out.view(torch.float32))
    got = out.cpu().numpy()
    e = np.arange(nb * bcap) % bcap
    live = (e < counts[np.arange(nb * bcap) // bcap]) & (t != HOLE)
    assert live.sum() > 60 and (~live[:bcap]).all() and live[bcap]
    want = np.where(live[:, None], vec[rows], np.int32(SENT))
    assert np.array_equal(got, want)
