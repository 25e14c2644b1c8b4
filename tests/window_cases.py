"""Inputs and harness shared by test_window_model.py (C++ twin, CPU) and
test_window_fire_kernels.py (HIP kernels): the seeded state builder, the case lists, and one
`check_*` function per kernel that runs it on a device and compares everything it wrote with
tests/window_model.py.

Rules the inputs keep (a defect must show as a wrong row, never as a fault):
  * every slot id in a list -- entries past list_n included --, bucket id, jhash index and pane
    index stays inside its buffer whatever the kernel does with it;
  * a kernel told to write at most `cap` rows gets a `cap`-long view of a buffer that could hold
    every row, so a kernel that ignores the cap overwrites sentinels, not foreign memory;
  * every output and staging word starts as a sentinel (FILL) and must still hold it wherever
    the kernel had nothing to write.

On the CPU the twin emits rows in visiting order (`ordered`); the GPU's order is unspecified and
keys are unique per slot, so its rows are compared sorted by key. All comparisons are exact.
"""
import functools
from collections import Counter

import numpy as np
import torch

import window_model as M
from mxstream.ops import expr as E
from mxstream.ops import kernels as K
from mxstream.ops.native import load

FILL = 0x1122334455667788            # what untouched output words must still hold
FILL32 = 0x11223344
WSTART, WEND = 1_697_846_399_123, 1_697_846_459_123     # epoch ms, not round
REC24 = np.dtype([("key", "<u8"), ("val", "<u8"), ("t", "<u4"), ("aux", "<u4")])
F64_AGGS = (M.AGG_SUM_F64, M.AGG_MIN_F64, M.AGG_MAX_F64, M.AGG_AVG_F64)
NANS = (0x7FF8000000000001, 0xFFF8000000000000, 0x7FF4000000000000)   # bits must survive
_u64 = np.uint64


# ---- state builder ------------------------------------------------------------------------------
def _gen_acc(rng, agg, ring, nslots):
    shape = (ring, nslots)
    sel = rng.integers(0, 10, shape)
    if agg not in F64_AGGS:
        full = rng.integers(M.I64_MIN, M.I64_MAX, shape, dtype=np.int64, endpoint=True)
        small = rng.integers(-1000, 1000, shape, dtype=np.int64)
        acc = np.where(sel < 4, full, small)                   # full-range values: sums wrap
        acc = np.where(sel == 4, M.I64_MAX, acc)
        acc = np.where(sel == 5, M.I64_MIN, acc)
        acc = np.where(sel == 6, M.I64_MAX - np.abs(small), acc)
        return acc.astype(np.int64).view(_u64)
    v = rng.standard_normal(shape) * 10.0 ** rng.integers(-300, 300, shape)
    sign = np.where(rng.random(shape) < 0.5, -1.0, 1.0)
    if agg in (M.AGG_SUM_F64, M.AGG_AVG_F64):
        # one sign of infinity per slot: inf - inf would produce a NaN of unspecified bits
        inf = np.broadcast_to(np.where(np.arange(nslots) % 2, -np.inf, np.inf), shape)
    else:
        inf = sign * np.inf
    v = np.where(sel == 0, 0.0, v)
    v = np.where(sel == 1, -0.0, v)
    v = np.where(sel == 2, inf, v)
    v = np.where(sel == 3, sign * rng.integers(1, 1000, shape) * 5e-324, v)    # subnormals
    v = np.where(sel == 4, 1e16, v)          # 1e16 + 1 - 1e16 depends on the order
    v = np.where(sel == 5, -1e16, v)
    v = np.where(sel == 6, 1.0, v)
    return np.ascontiguousarray(v).view(_u64)


@functools.lru_cache(maxsize=4)
def build_state(seed, nslots, ring, agg=M.AGG_SUM_I64, big_keys=False, nan_panes=None,
                empty_panes=(), p_dirty=0.3):
    """About 60 % of the slots occupied (empty ones: key ~0, no counts); an occupied slot has
    counts (1 .. 2^20) in a random subset of panes, in exactly one, or in all; accumulators are
    set everywhere (also where the count is 0: a kernel must not read them); dirty bytes are
    independent of the counts. Keys are unique: below 2^32, or (big_keys) above 2^53, above 2^63
    and next to 2^64. nan_panes = (first, middle, last): three groups of slots carry a NaN there.
    The result is shared between tests and never written."""
    rng = np.random.default_rng(seed)
    occ = rng.random(nslots) < 0.6
    occ[0] = True
    slot = np.arange(nslots, dtype=_u64)
    if big_keys:
        keys = np.where(slot % _u64(3) == 0, _u64(1 << 53) + slot * _u64(3) + _u64(1),
                        np.where(slot % _u64(3) == 1, _u64(1 << 63) + slot * _u64(1025) + _u64(1),
                                 _u64(M.U64 - 2) - slot))
    else:
        keys = (slot * _u64(2654435761) + _u64(seed)) & _u64(0xFFFFFFFF)  # a bijection mod 2^32
    keys = np.where(occ, keys, _u64(M.EMPTY_KEY))
    kind = rng.integers(0, 4, nslots)
    has = rng.random((ring, nslots)) < np.where(kind == 3, 0.8, 0.35)
    one = np.flatnonzero(kind == 1)
    has[:, one] = False
    has[rng.integers(0, ring, len(one)), one] = True
    has[:, kind == 2] = True
    has[:, ~occ] = False
    has[[p % ring for p in empty_panes], :] = False
    cnt = np.where(has, rng.integers(1, (1 << 20) + 1, (ring, nslots)), 0).astype(np.uint32)
    acc = _gen_acc(rng, agg, ring, nslots).copy()
    if nan_panes is not None:
        for g, pane in enumerate(nan_panes):
            s = np.flatnonzero(occ & (np.arange(nslots) % 16 == g + 1))
            acc[pane % ring, s] = np.array(NANS, dtype=_u64)[np.arange(len(s)) % len(NANS)]
            cnt[pane % ring, s] = np.maximum(cnt[pane % ring, s], 1)
        s = np.flatnonzero(np.arange(nslots) % 16 == 4)       # only zeros, of both signs
        acc[:, s] = np.where(rng.random((ring, len(s))) < 0.5, _u64(0), _u64(1 << 63))
    dirty = (rng.random((ring, nslots)) < p_dirty).astype(np.uint8)
    mark = (rng.random(nslots) < 0.5).astype(np.uint32)
    st = M.State(keys, acc.reshape(-1), cnt.reshape(-1), dirty.reshape(-1), ring, mark)
    for a in (st.keys, st.acc, st.cnt, st.dirty, st.mark):
        a.setflags(write=False)
    return st


# ---- epilogue programs --------------------------------------------------------------------------
_r, _c, _ws, _we, _k, _raw, _m = (E.var(i) for i in range(7))
# (map, filter, reads keys >= 2^63); each once as chain programs ("VAR, (CONST|VAR, binop)*",
# evaluated in registers) and once as trees of depth >= 3 (the LDS stack VM)
EPILOGUES = {
    "map-chain": (_r * 8.0 / 60 / 1024, None, False),
    "filt-chain": (None, _r > 0.0, False),
    "both-chain": (_r * 0.5 + _c, _r < 1e18, False),
    "filtmapped-chain": (_r / 3.0, _m - 1000.0 >= _c, False),
    "vars-chain": ((_k + _raw - _c) * _ws / _we, None, True),
    "map-stack": ((_r + _c) * (_r - 3.0), None, False),
    "filt-stack": (None, (_r + _c) * (_r - 3.0) > (_c + 1.0) * (_c - _r), False),
    "both-stack": ((_r + _c) * (_r - 3.0), (_r + _c) * (_c - 3.0) > (_c + 1.0) * (_c - _r), False),
    "filtmapped-stack": ((_r + 1.0) / (_c + 2.0), (_m + _c) * (_m - _r) >= (_c - _m) * (_c + _r),
                         False),
    "vars-stack": ((_k + _raw) * (_we - _ws) / (_c + _ws), None, True),
}


def programs(name):
    mp, fp, big = EPILOGUES[name]
    mp, fp = E.compile_expr(mp), E.compile_expr(fp)
    chain = name.endswith("-chain")
    for prog in (mp, fp):
        if not prog.empty:
            assert bool(load().expr_is_chain(*prog.as_args())) == chain, name
    return mp, fp, big


# ---- case lists ---------------------------------------------------------------------------------
GEOM_PANES = [(0, 1), (5, 7), (5, 8), (5, 9), (12, 9), (-3, 6), (3, 16)]    # ring 16; kFireP = 8
GEOM = [(ns, p0, np_, od) for ns in (1, 1023, 4096, 4097) for p0, np_ in GEOM_PANES
        for od in (False, True)]
LIST = [(n, od) for n in (0, 1, 4096, 4097) for od in (True, False)]
OUTPUTS = ["key32", "cap-exact", "cap-minus-1", "cap-0", "append"]
BIG_NSLOTS = 1024 * 4096 + 4097      # the grid is capped at 1024 workgroups of 4096 slots
# 33 and 40 windows: a second pack of 32. The last window has no rows, so with 33 the second pack
# writes nothing; with 40 it holds seven windows that do.
MANY_SMALL = [(ns, k, k32) for ns in (255, 4096) for k in (1, 2, 32, 33, 40)
              for k32 in (False, True)]
MANY_BIG = [65536, 256 * 1024 + 1029]     # U = 4 from 65,536 slots; 256 workgroups of 1024
MANY_EMPTY = tuple(range(40, 48))    # ring-64 panes without any count: windows without rows


def many_wins(k):
    """k windows over a ring of 64 with different p0 (some wrapping, some negative) and npanes
    (60 among them); from k = 2 on the first, from k = 32 on also the last and some between have
    no rows (their panes hold no count)."""
    shapes = [(3, 60), (-7, 9), (58, 13), (17, 1), (30, 8), (126, 7), (-70, 64), (9, 17)]
    wins = []
    for i in range(k):
        p0, np_ = shapes[i % len(shapes)]
        p0 += 64 * (i // len(shapes))
        if (i == 0 and k > 1) or (k >= 32 and (i == k - 1 or i % 13 == 5)):
            p0, np_ = 40 + 64 * i, 1 + i % 8
        wins.append((p0, np_, float(WSTART + 5000 * i), float(WEND + 5000 * i)))
    return wins


REFIRE_U0 = 10                       # the union is panes 10 .. 25 of a ring of 16: it wraps


def refire_wins(k):
    """k windows whose union is exactly [10, 26)."""
    base = [(10, 6), (13, 8), (20, 6), (10, 16)]
    if k == 1:
        base = [(10, 16)]
    wins = []
    for i in range(k):
        if i < len(base):
            p0, np_ = base[i]
        else:
            p0 = 10 + (i * 5) % 16
            np_ = 1 + (i * 3) % (26 - p0)
        wins.append((p0, np_, float(WSTART + 7000 * i), float(WEND + 7000 * i)))
    assert M.refire_union(wins) == (10, 26)
    return wins


# (dlo, dmask_abs, epilogue, key32, clear_mark). The masks leave out union panes that do hold
# dirty bytes; the second has bit 31 set, which stands for no pane (only bits 0..30 count).
REFIRE_VARIANTS = {
    "all-chain-k64-clear": (0, 0, "both-chain", False, True),
    "mask-stack-k32": (8, sum(1 << (p - 8) for p in (11, 12, 15, 20, 25)), "both-stack", True,
                       False),
    "mask31-chain-k32-clear": (-10, sum(1 << (p + 10) for p in (11, 12, 15, 20, 21)),
                               "filtmapped-chain", True, True),
    "all-stack-k64": (0, 0, "filtmapped-stack", False, False),
}
REFIRE = [(n, k, v) for n in (0, 1, 255, 256, 257, 3000) for k in (1, 4, 32)
          for v in REFIRE_VARIANTS]
REFIRE_FALSE = ["k33", "union17", "ring8-union9", "no-list"]
DIRTY_CLEAR = [(n, p_lo, np_, delta) for n in (0, 1, 257, 1000)     # the list buffer has 300
               for p_lo, np_ in ((0, 16), (13, 5), (-2, 3), (4, 0)) for delta in (False, True)]
SCATTER = [(n, geom, mp, hm) for n in (0, 1, 8191, 8192, 8193, 20000)   # n_cap = 8200
           for geom in ((1, 0), (2, 3), (8, 6)) for mp in (128, 120) for hm in (0, 1)]
STEP_FINISH = [(fl, ev, lm, ovf) for fl in (None, 0, 1, 6) for ev in (0, 1)
               for lm in ("min", "below", "above") for ovf in (0, 1, 2, 4, 8, 16, 31)]
KEYGROUPS = [(hm, mp) for hm in (0, 1) for mp in (128, 120)]
TABLE = [(0, 4), (3, 6)]


# ---- device plumbing ----------------------------------------------------------------------------
def to_dev(a, dev):
    a = np.ascontiguousarray(a)
    if a.dtype in (np.uint64, np.uint32):
        a = a.view(np.int64 if a.dtype == np.uint64 else np.int32)
    return torch.from_numpy(a.copy()).to(dev)


def to_np(t, dtype=None):
    a = t.cpu().numpy()
    return a if dtype is None else a.view(dtype)


def filled(n, dev, dtype=torch.int64):
    if dtype == torch.float64:
        return torch.full((n,), FILL, dtype=torch.int64, device=dev).view(torch.float64)
    return torch.full((n,), FILL if dtype == torch.int64 else FILL32, dtype=dtype, device=dev)


def sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)


def stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else 0


def p(t):
    return 0 if t is None else t.data_ptr()


class DevState:
    def __init__(self, st, dev):
        self.dev = dev
        self.keys, self.acc = to_dev(st.keys, dev), to_dev(st.acc, dev)
        self.cnt, self.dirty = to_dev(st.cnt, dev), to_dev(st.dirty, dev)
        self.mark = to_dev(st.mark, dev)
        self.ring = st.ring

    def ptrs(self):
        return p(self.keys), p(self.acc), p(self.cnt), p(self.dirty)

    def assert_equals(self, st):
        sync(self.dev)
        assert np.array_equal(to_np(self.keys, _u64), st.keys)
        assert np.array_equal(to_np(self.acc, _u64), st.acc)
        assert np.array_equal(to_np(self.cnt, np.uint32), st.cnt)
        assert np.array_equal(to_np(self.dirty), st.dirty), "dirty bytes"
        assert np.array_equal(to_np(self.mark, np.uint32), st.mark), "slot marks"


class Columns:
    """The four row columns (raw / cnt absent for compact rows), sentinel-filled."""

    def __init__(self, n, dev, raw=True):
        self.keys, self.vals = filled(n, dev), filled(n, dev, torch.float64)
        self.raw = filled(n, dev) if raw else None
        self.cnt = filled(n, dev, torch.int32) if raw else None

    def ptrs(self):
        return p(self.keys), p(self.vals), p(self.raw), p(self.cnt)

    def host(self):
        return Host(to_np(self.keys, _u64), to_np(self.vals, _u64),
                    None if self.raw is None else to_np(self.raw, _u64),
                    None if self.cnt is None else to_np(self.cnt, np.uint32))


class Host:
    def __init__(self, keys, vals, raw, cnt):
        self.keys, self.vals, self.raw, self.cnt = keys, vals, raw, cnt

    def rows(self, lo, hi, key32, base=0):
        """Rows lo .. hi-1 of the region starting at word `base` (compact keys: uint32 from
        the region's first word on)."""
        out = np.zeros(hi - lo, M.ROW)
        out["key"] = (self.keys[base:].view(np.uint32) if key32 else self.keys[base:])[lo:hi]
        out["val"] = self.vals[base + lo:base + hi]
        if self.raw is not None:
            out["raw"], out["cnt"] = self.raw[base + lo:base + hi], self.cnt[base + lo:base + hi]
        return out

    def assert_untouched(self, lo, hi, key32, base=0):
        """Rows lo .. hi-1 of that region still hold the sentinel."""
        if key32:
            k = self.keys[base:base + hi].view(np.uint32)
            assert np.array_equal(k[lo:], np.full(hi, FILL, _u64).view(np.uint32)[lo:]), "keys"
        else:
            assert (self.keys[base + lo:base + hi] == FILL).all(), "keys past the rows"
        assert (self.vals[base + lo:base + hi] == FILL).all(), "values past the rows"
        if self.raw is not None:
            assert (self.raw[base + lo:base + hi] == FILL).all(), "raw past the rows"
            assert (self.cnt[base + lo:base + hi] == FILL32).all(), "counts past the rows"


def shown(rows, key32, raw):
    """What the columns can show of the model's rows."""
    rows = rows.copy()
    if key32:
        rows["key"] &= _u64(0xFFFFFFFF)
    if not raw:
        rows["raw"], rows["cnt"] = 0, 0
    return rows


def by_key(rows):
    return rows[np.argsort(rows["key"], kind="stable")]


def assert_rows(got, want, ordered):
    assert len(got) == len(want), f"{len(got)} rows, expected {len(want)}"
    if not ordered:
        got, want = by_key(got), by_key(want)
    for f in M.ROW.names:
        bad = np.flatnonzero(got[f] != want[f])
        assert not len(bad), f"{f}: {len(bad)} rows differ, first {got[bad[0]]} != {want[bad[0]]}"


def assert_members(got, want):
    """Distinct rows of the expected set (which ones is not determined)."""
    assert len(np.unique(got["key"])) == len(got), "a row twice"
    w = by_key(want)
    i = np.searchsorted(w["key"], got["key"])
    assert (i < len(w)).all()
    assert_rows(got, w[i], True)


def fire_plan(st, agg, only_dirty, mp, fp, key32, out_cap, p0=0, npanes=1, **extra):
    return dict(agg=agg, npanes=npanes, ring=st.ring, only_dirty=int(only_dirty),
                nslots=st.nslots, p0=p0, wstart=float(WSTART), wend=float(WEND), out_cap=out_cap,
                map=tuple(mp.as_args()), filt=tuple(fp.as_args()), key32=int(key32), **extra)


# ---- window_fire --------------------------------------------------------------------------------
def check_fire(dev, st, ordered, *, agg, p0, npanes, only_dirty, mp=E.EMPTY, fp=E.EMPTY,
               cap=lambda n: n + 5, key32=False, raw=True, slots=None, list_n=None, n0=0):
    """One window_fire launch against M.fire. cap: out_cap as a function of the row count
    (rows already there included); n0: rows already in the columns, out_n starting there."""
    visit = None if slots is None else slots[:list_n]
    want = shown(M.fire(st, agg, p0, npanes, only_dirty, WSTART, WEND, mp, fp, visit), key32, raw)
    n = n0 + len(want)
    cap = cap(n)
    size = max(n, cap, st.nslots if slots is None else len(slots)) + n0 + 8
    ds, cols = DevState(st, dev), Columns(size, dev, raw)
    pre = np.arange(1, n0 + 1, dtype=np.int64) * 1000003
    for col in (cols.keys, cols.raw, cols.cnt):
        if col is not None and n0:
            col[:n0] = torch.from_numpy(pre).to(dev).to(col.dtype)
    if n0:
        cols.vals[:n0] = torch.from_numpy(pre).to(dev).view(torch.float64)
    before = cols.host() if n0 else None
    out_n = torch.full((3,), FILL32, dtype=torch.int32, device=dev)
    out_n[0] = n0
    lst = {}
    if slots is not None:
        lst = dict(slot_list=to_dev(np.asarray(slots, dtype=np.int32), dev),
                   slot_list_n=torch.tensor([list_n], dtype=torch.int32, device=dev))
    K.window_fire(ds.keys, ds.acc, ds.cnt, ds.dirty, agg=agg, npanes=npanes, ring=st.ring, p0=p0,
                  wstart=WSTART, wend=WEND, only_dirty=only_dirty, map_prog=mp, filt_prog=fp,
                  out_keys=cols.keys[:cap], out_vals=cols.vals[:cap],
                  out_raw=None if cols.raw is None else cols.raw[:cap],
                  out_cnt=None if cols.cnt is None else cols.cnt[:cap], out_n=out_n[:1],
                  key32=key32, **lst)
    sync(dev)
    assert out_n.tolist() == [n, FILL32, FILL32], "out_n counts every row"
    host = cols.host()
    w = max(min(cap, n), n0)                                # rows the columns hold afterwards
    got = host.rows(n0, w, key32)
    if w == n:
        assert_rows(got, want, ordered)
    elif ordered:
        assert_rows(got, want[:w - n0], True)
    else:
        assert_members(got, want)
    host.assert_untouched(w, size, key32)
    if n0:
        assert_rows(host.rows(0, n0, key32), before.rows(0, n0, key32), True)
    ds.assert_equals(st)                                    # a firing only reads the state
    return len(want)


# ---- window_fire_many ---------------------------------------------------------------------------
def check_fire_many(dev, st, ordered, *, agg, wins, key32, mp=E.EMPTY, fp=E.EMPTY,
                    only_dirty=False, region=None):
    m = load()
    k, cuda = len(wins), dev.type == "cuda"
    region = st.nslots if region is None else region
    rows, bounds = M.fire_many(st, agg, only_dirty, mp, fp, wins)
    rows = shown(rows, key32, not key32)
    size = k * region + 8
    ds, cols = DevState(st, dev), Columns(size, dev, raw=not key32)
    stage_cols = Columns(k * region + 8, dev, raw=not key32) if cuda else None
    win_n = filled(k + 4, dev, torch.int32)
    bnd = filled(k + 4, dev, torch.int32)
    out_n = torch.tensor([0, FILL32], dtype=torch.int32, device=dev)
    stage = (*stage_cols.ptrs(), p(win_n), region) if cuda else None
    m.window_fire_many(cuda, *ds.ptrs(), fire_plan(st, agg, only_dirty, mp, fp, key32, size), wins,
                       *cols.ptrs(), p(out_n), p(bnd), stream(dev), stage)
    sync(dev)
    assert to_np(bnd, np.uint32).tolist() == bounds.tolist() + [FILL32] * 4, "bounds"
    assert out_n.tolist() == [len(rows), FILL32]
    host = cols.host()
    lo = 0
    for w, hi in enumerate(bounds.tolist()):
        assert_rows(host.rows(lo, hi, key32), rows[lo:hi], ordered)
        lo = hi
    host.assert_untouched(len(rows), size, key32)
    if cuda:
        per = np.diff(bounds.astype(np.int64), prepend=0)
        assert to_np(win_n, np.uint32).tolist() == per.tolist() + [FILL32] * 4, "window counters"
        sh = stage_cols.host()
        for w in range(k):
            sh.assert_untouched(int(per[w]), region, key32, base=w * region)
        sh.assert_untouched(0, 8, False, base=k * region)
    ds.assert_equals(st)
    return bounds


# ---- gpu_window_refire_many ---------------------------------------------------------------------
def check_refire(dev, st, *, agg, wins, slots, list_n, variant, region=None, plan_list=True):
    """One fused re-firing against M.refire_many (GPU only: it has no twin). region None: the
    list length rounded up to 4, as production sizes it. Returns the kernel's verdict."""
    m = load()
    dlo, dmask, epi, key32, clear = REFIRE_VARIANTS[variant]
    mp, fp, _ = programs(epi)
    k = len(wins)
    region = max(4, (list_n + 3) & ~3) if region is None else region
    model = M.refire_many(st, agg, mp, fp, wins, slots[:list_n] if plan_list else None, dlo, dmask,
                          clear=clear)
    size = k * region + 8
    ds, cols = DevState(st, dev), Columns(size, dev, raw=not key32)
    stage_cols = Columns(k * region + 8, dev, raw=not key32)
    win_n = filled(k + 4, dev, torch.int32)
    bnd = filled(k + 4, dev, torch.int32)
    out_n = torch.tensor([FILL32, FILL32], dtype=torch.int32, device=dev)
    ovf = torch.tensor([5, FILL32], dtype=torch.int32, device=dev)
    lst = to_dev(np.asarray(slots, dtype=np.int32), dev)
    lst_n = torch.tensor([list_n], dtype=torch.int32, device=dev)
    extra = dict(list=p(lst), list_n=p(lst_n)) if plan_list else {}
    if clear:
        extra["clear_mark"] = p(ds.mark)
    plan = fire_plan(st, agg, True, mp, fp, key32, size, **extra)
    ok = m.gpu_window_refire_many(*ds.ptrs(), plan, wins, *cols.ptrs(), p(out_n), p(bnd), p(ovf), stream(dev),
                                  (*stage_cols.ptrs(), p(win_n), region), dlo, dmask)
    sync(dev)
    host = cols.host()
    if model is None:
        assert ok is False
        host.assert_untouched(0, size, key32)
        stage_cols.host().assert_untouched(0, k * region + 8, key32)
        assert out_n.tolist() == [FILL32] * 2 and ovf.tolist() == [5, FILL32]
        assert (to_np(bnd, np.uint32) == FILL32).all() and (to_np(win_n, np.uint32) == FILL32).all()
        ds.assert_equals(st)
        return ok
    assert ok is True
    rows = shown(model[0], key32, not key32)
    per = np.diff(model[1].astype(np.int64), prepend=0)
    kept = np.minimum(per, region)                 # a region keeps `region` rows of its window
    assert to_np(win_n, np.uint32).tolist() == per.tolist() + [FILL32] * 4, "window counters"
    assert to_np(bnd, np.uint32).tolist() == np.cumsum(kept).tolist() + [FILL32] * 4, "bounds"
    assert out_n.tolist() == [int(kept.sum()), FILL32]
    # "bit 16" of the flags word in the sources' comments is the value 16
    assert ovf.tolist() == [5 | (16 if (per > region).any() else 0), FILL32]
    lo = mlo = 0
    for w in range(k):
        got, want = host.rows(lo, lo + int(kept[w]), key32), rows[mlo:mlo + int(per[w])]
        if per[w] <= region:
            assert_rows(got, want, False)
        else:
            assert_members(got, want)
        lo, mlo = lo + int(kept[w]), mlo + int(per[w])
    host.assert_untouched(lo, size, key32)
    sh = stage_cols.host()
    for w in range(k):
        sh.assert_untouched(int(kept[w]), region, key32, base=w * region)
    sh.assert_untouched(0, 8, False, base=k * region)
    ds.assert_equals(model[2] if clear else st)
    return ok


# ---- dirty_clear --------------------------------------------------------------------------------
def check_dirty_clear(dev, list_n, p_lo, np_, with_delta):
    st = build_state(31, 1023, 16, p_dirty=0.7)
    rng = np.random.default_rng(list_n * 100 + np_)
    slots = rng.permutation(st.nslots)[:300].astype(np.int32)
    delta = None
    if with_delta:
        delta = (rng.integers(1, 1 << 62, len(st.acc)).astype(_u64),
                 rng.integers(1, 1 << 30, len(st.acc)).astype(np.uint32))
    want, want_delta = M.dirty_clear(st, slots[:min(list_n, len(slots))], p_lo, np_, delta)
    ds = DevState(st, dev)
    dd = None if delta is None else (to_dev(delta[0], dev), to_dev(delta[1], dev))
    K.dirty_clear(to_dev(slots, dev), torch.tensor([list_n], dtype=torch.int32, device=dev),
                  ring=st.ring, nslots=st.nslots, dirty_g=ds.dirty, slot_mark=ds.mark, p_lo=p_lo,
                  np_=np_, dacc=None if dd is None else dd[0], dcnt=None if dd is None else dd[1])
    ds.assert_equals(want)
    if delta is not None:
        assert np.array_equal(to_np(dd[0], _u64), want_delta[0])
        assert np.array_equal(to_np(dd[1], np.uint32), want_delta[1])
    assert list_n == 0 or np_ == 0 or not np.array_equal(want.dirty, st.dirty)


# ---- scatter_partials ---------------------------------------------------------------------------
SCAT_NCAP, JHASH_LEN = 8200, 4096


def _scatter_input(seed, hash_mode, nrows=SCAT_NCAP):
    rng = np.random.default_rng(seed)
    if hash_mode:
        keys = rng.integers(0, JHASH_LEN, nrows).astype(_u64)
    else:
        keys = rng.integers(0, 1 << 64, nrows, dtype=_u64)     # the whole uint64 range
        keys[:4] = (0, M.U64, 1 << 63, (1 << 63) - 1)
    acc = rng.integers(0, 1 << 64, nrows, dtype=_u64)
    cnt = rng.integers(1, 1 << 32, nrows).astype(np.uint32)
    jhash = rng.integers(-(1 << 31), 1 << 31, JHASH_LEN).astype(np.int32)
    return keys, acc, cnt, jhash


def run_scatter(dev, ordered, keys, acc, cnt, jhash, n_dev, *, nranks, nsub_log2, max_par,
                hash_mode, kg_dest, cursor0, bucket_cap, flags0=4):
    """Launch scatter_partials and compare buckets, cursors, flag and untouched words with the
    model. bucket_cap None: the fullest bucket plus 3."""
    nb, n_cap = nranks << nsub_log2, len(keys)
    want, cur, ovf = M.scatter_partials(keys, acc, cnt, min(n_dev, n_cap), max_par, nranks,
                                        nsub_log2, kg_dest, jhash if hash_mode else None, 1 << 40,
                                        cursor0)
    if bucket_cap is None:
        bucket_cap = int(cur.max()) + 3
    else:
        ovf = bool((cur > bucket_cap).any())
    out = filled(nb * bucket_cap * K.REC_WORDS, dev)
    cursor = to_dev(np.asarray(cursor0, dtype=np.uint32), dev)
    flags = torch.tensor([flags0, FILL32], dtype=torch.int32, device=dev)
    K.scatter_partials(to_dev(keys, dev), to_dev(acc, dev), to_dev(cnt, dev),
                       torch.tensor([n_dev], dtype=torch.int32, device=dev), n_cap=n_cap,
                       max_parallelism=max_par, nranks=nranks, nsub_log2=nsub_log2,
                       hash_mode=hash_mode, jhash=to_dev(jhash, dev) if hash_mode else None,
                       kg_dest=to_dev(np.asarray(kg_dest, dtype=np.int32), dev),
                       bucket_cap=bucket_cap, cursor=cursor, out=out, flags=flags[:1])
    sync(dev)
    assert np.array_equal(to_np(cursor, np.uint32), cur), "cursors count every row"
    assert flags.tolist() == [flags0 | int(ovf), FILL32]
    words = to_np(out).reshape(nb, bucket_cap, K.REC_WORDS)
    recs = to_np(out).view(REC24).reshape(nb, bucket_cap)
    for b in range(nb):
        lo, hi = int(cursor0[b]), min(int(cur[b]), bucket_cap)
        got = [tuple(r) for r in recs[b, lo:max(lo, hi)].tolist()]
        if int(cur[b]) <= bucket_cap:
            same = (got == want[b]) if ordered else (Counter(got) == Counter(want[b]))
            assert same, f"bucket {b}"
        elif ordered:
            assert got == want[b][:hi - lo], f"bucket {b}"
        else:       # which rows an overflowing bucket keeps is not determined
            assert not Counter(got) - Counter(want[b]), f"bucket {b}: a record not sent to it"
        assert (words[b, :lo] == FILL).all() and (words[b, max(lo, hi):] == FILL).all(), \
            f"bucket {b}: words outside its new records changed"
    return cur, bucket_cap


def check_scatter(dev, ordered, n_dev, geom, max_par, hash_mode):
    nranks, nsub_log2 = geom
    keys, acc, cnt, jhash = _scatter_input(n_dev + max_par + hash_mode, hash_mode)
    kg_dest = [(g * 7 + 3) % nranks for g in range(max_par)]
    cursor0 = [(b * 5) % 4 for b in range(nranks << nsub_log2)]
    run_scatter(dev, ordered, keys, acc, cnt, jhash, n_dev, nranks=nranks, nsub_log2=nsub_log2,
                max_par=max_par, hash_mode=hash_mode, kg_dest=kg_dest, cursor0=cursor0,
                bucket_cap=None)


def check_scatter_hot(dev, ordered):
    """Most rows go to bucket 1 of 4, which holds 600: the flag, the full cursor, 600 distinct
    records sent to it, and untouched neighbours. A kernel without the cap would write into
    buckets 2 and 3 (1 * 600 + ~1700 < 4 * 600), never outside the buffer."""
    keys, acc, cnt, jhash = _scatter_input(77, 1, nrows=2000)
    jhash[keys[np.arange(2000) % 6 != 0].astype(np.int64)] = 12345
    kg = int(M.keygroups([0], 128, [12345])[0])
    kg_dest = [1 if g == kg else g % 4 for g in range(128)]
    acc = np.arange(2000, dtype=_u64) * _u64(3)                # records distinct whatever the keys
    cur, _ = run_scatter(dev, ordered, keys, acc, cnt, jhash, 2000, nranks=4, nsub_log2=0,
                         max_par=128, hash_mode=1, kg_dest=kg_dest, cursor0=[2, 1, 0, 3],
                         bucket_cap=600)
    assert cur[1] > 1500 and max(cur[0], cur[2], cur[3]) < 600


# ---- step_begin / step_finish -------------------------------------------------------------------
def check_step_begin(dev, nb):
    buf = filled(nb + 4, dev, torch.int32)
    stats = filled(M.STAT_COUNT + 2, dev)
    K.step_begin(buf[:nb], stats[:M.STAT_COUNT])
    sync(dev)
    cursor, want_stats = M.step_begin(nb)
    assert buf.tolist() == cursor + [FILL32] * 4
    assert stats.tolist() == want_stats + [FILL] * 2


def check_step_finish(dev, flags, event_mode, lm_kind, ovf):
    stats = M.stats_init()
    local = M.I64_MIN
    if lm_kind != "min":
        stats[:3] = [1_697_846_400_777, -12, 345]
        stats[3:] = [17, ovf, 4242, 99, 0x5A5A]
        local = stats[0] + (-5000 if lm_kind == "below" else 5000)
    else:
        stats[M.STAT_OVERFLOW] = ovf
    bound, now = 2500, 1_697_846_500_001
    want, want_lm = M.step_finish(stats, local, bound, event_mode, now, flags)
    d_stats = torch.tensor(stats, dtype=torch.int64, device=dev)
    d_lm = torch.tensor([local, FILL], dtype=torch.int64, device=dev)
    red = filled(M.RED_WORDS + 2, dev)
    d_flags = None if flags is None else torch.tensor([flags], dtype=torch.int32, device=dev)
    K.step_finish(d_stats, d_lm[:1], red[:M.RED_WORDS], bound=bound, event_mode=bool(event_mode),
                  proc_now=now, flags=d_flags)
    sync(dev)
    assert red.tolist() == want + [FILL] * 2
    assert d_lm.tolist() == [want_lm, FILL] and d_stats.tolist() == stats


# ---- keygroups / table_insert -------------------------------------------------------------------
def check_keygroups(dev, hash_mode, max_par):
    rng = np.random.default_rng(5 + hash_mode)
    n = 10001
    jhash = None
    if hash_mode:
        jhash = rng.integers(-(1 << 31), 1 << 31, JHASH_LEN).astype(np.int32)
        jhash[:3] = (-(1 << 31), (1 << 31) - 1, 0)
        keys = rng.integers(0, JHASH_LEN, n).astype(np.int64)
        keys[:3] = (0, 1, 2)
    else:
        keys = rng.integers(M.I64_MIN, M.I64_MAX, n, dtype=np.int64, endpoint=True)
        keys[:6] = (0, M.I64_MIN, M.I64_MAX, -1, -2, 1 << 32)
    got = K.keygroups(to_dev(keys, dev), max_parallelism=max_par, hash_mode=hash_mode,
                      jhash=None if jhash is None else to_dev(jhash, dev))
    sync(dev)
    assert np.array_equal(to_np(got), M.keygroups(keys.view(_u64), max_par, jhash))


def table_keys(nsub_log2, cap_log2):
    """Unique keys, each twice, in a shuffled order: one sub-table gets one key more than it
    holds, the others are about a third full."""
    cap, nsub = 1 << cap_log2, 1 << nsub_log2
    rng = np.random.default_rng(cap)
    full_sub = nsub - 3 if nsub > 1 else 0
    need = {s: cap + 1 if s == full_sub else cap // 3 for s in range(nsub)}
    keys = []
    while any(need.values()):
        cand = rng.integers(0, 1 << 64, 256, dtype=_u64)
        for k, s in zip(cand.tolist(), M.sub_table_of(cand, nsub_log2).tolist()):
            if need[s] and k < M.U64 - 1 and k not in keys:
                keys.append(k)
                need[s] -= 1
    return rng.permutation(np.array(keys + keys, dtype=_u64))


def check_table_insert(dev, nsub_log2, cap_log2):
    keys = table_keys(nsub_log2, cap_log2)
    nslots = (1 << nsub_log2) << cap_log2
    empty = np.full(nslots, M.EMPTY_KEY, _u64)
    want_table, want_slots, overflow = M.table_insert(empty, keys, nsub_log2, cap_log2)
    assert overflow == 2                       # the one key too many, both times
    buf = torch.full((nslots + 4,), -1, dtype=torch.int64, device=dev)
    buf[nslots:] = FILL
    slots = K.table_insert(to_dev(keys, dev), buf[:nslots], nsub_log2=nsub_log2, cap_log2=cap_log2)
    sync(dev)
    assert buf[nslots:].tolist() == [FILL] * 4
    table = to_np(buf, _u64)[:nslots]
    M.check_table(table, keys, to_np(slots), nsub_log2, cap_log2, overflow)
    if dev.type == "cpu":                      # one key after the other: the model's very table
        assert np.array_equal(table, want_table) and np.array_equal(to_np(slots), want_slots)


# ---- the window_fire / window_fire_many / re-firing cases, one function per case list -----------
_SUM = dict(agg=M.AGG_SUM_I64, p0=12, npanes=9, only_dirty=False)    # panes 12 .. 20 wrap ring 16


def case_geometry(dev, ordered, nslots, p0, npanes, only_dirty):
    check_fire(dev, build_state(11, nslots, 16), ordered, agg=M.AGG_SUM_I64, p0=p0, npanes=npanes,
               only_dirty=only_dirty)


def case_aggregate(dev, ordered, agg):
    nan = (12, 16, 20) if agg in (M.AGG_MIN_F64, M.AGG_MAX_F64) else None   # first, middle, last
    st = build_state(12, 4097, 16, agg=agg, nan_panes=nan)
    assert check_fire(dev, st, ordered, **dict(_SUM, agg=agg)) > 2000


def case_epilogue(dev, ordered, name):
    mp, fp, big = programs(name)
    st = build_state(13, 4097, 16, big_keys=big)
    n = check_fire(dev, st, ordered, mp=mp, fp=fp, **_SUM)
    every = len(M.fire(st, M.AGG_SUM_I64, 12, 9, False, WSTART, WEND))
    assert (every // 20 < n < every - every // 20) if not fp.empty else n == every


def case_outputs(dev, ordered, name):
    st = build_state(14, 4097, 16)
    kw = {"key32": dict(key32=True, raw=False), "cap-exact": dict(cap=lambda n: n),
          "cap-minus-1": dict(cap=lambda n: n - 1), "cap-0": dict(cap=lambda n: 0),
          "append": dict(n0=5)}[name]
    check_fire(dev, st, ordered, **_SUM, **kw)


def case_list(dev, ordered, list_n, only_dirty):
    st = build_state(15, 9000, 16)
    slots = np.random.default_rng(list_n).permutation(st.nslots)[:8192]    # no slot twice
    check_fire(dev, st, ordered, **dict(_SUM, only_dirty=only_dirty), slots=slots, list_n=list_n)


def case_second_round(dev, ordered):
    st = build_state(16, BIG_NSLOTS, 1, agg=M.AGG_MAX_I64)
    check_fire(dev, st, ordered, agg=M.AGG_MAX_I64, p0=0, npanes=1, only_dirty=False)


def case_many_small(dev, ordered, nslots, k, key32):
    st = build_state(17, nslots, 64, empty_panes=MANY_EMPTY)
    mp, fp, _ = programs("both-chain")
    bounds = check_fire_many(dev, st, ordered, agg=M.AGG_SUM_I64, wins=many_wins(k), key32=key32,
                             mp=mp, fp=fp)
    per = np.diff(bounds.astype(np.int64), prepend=0)
    assert per.max() > nslots // 8
    if k > 1:
        assert per[0] == 0 and (k < 32 or (per[-1] == 0 and per[5] == 0 and per[18] == 0))
    assert k != 40 or per[32:39].min() > 0


def case_many_big(dev, ordered, nslots):
    st = build_state(18, nslots, 16)
    mp, fp, _ = programs("filtmapped-stack")
    wins = [(3, 5, float(WSTART), float(WEND)), (12, 9, float(WSTART + 1), float(WEND + 1)),
            (-2, 16, float(WSTART + 2), float(WEND + 2))]
    check_fire_many(dev, st, ordered, agg=M.AGG_SUM_I64, wins=wins, key32=False, mp=mp, fp=fp)


def refire_input(ring=16):
    st = build_state(19, 4096, ring, p_dirty=0.5)
    return st, np.random.default_rng(19).permutation(st.nslots)[:3072]      # no slot twice


def case_refire(dev, list_n, k, variant):
    st, slots = refire_input()
    assert check_refire(dev, st, agg=M.AGG_SUM_I64, wins=refire_wins(k), slots=slots,
                        list_n=list_n, variant=variant)


REFIRE_SMALL_REGION = [(10, 16), (11, 1), (25, 1), (18, 2)]     # the first has far more rows


def refire_small_region(st, slots, variant, list_n=3000):
    """Windows and a region that holds every window but the first."""
    wins = [(p0, n, float(WSTART + i), float(WEND + i))
            for i, (p0, n) in enumerate(REFIRE_SMALL_REGION)]
    dlo, dmask, epi, _, _ = REFIRE_VARIANTS[variant]
    mp, fp, _ = programs(epi)
    bounds = M.refire_many(st, M.AGG_SUM_I64, mp, fp, wins, slots[:list_n], dlo, dmask)[1]
    per = np.diff(bounds.astype(np.int64), prepend=0)
    region = (int(per[1:].max()) + 3) & ~3
    assert per[0] > region > 0
    return wins, region


def case_refire_small_region(dev, variant):
    st, slots = refire_input()
    wins, region = refire_small_region(st, slots, variant)
    assert check_refire(dev, st, agg=M.AGG_SUM_I64, wins=wins, slots=slots, list_n=3000,
                        variant=variant, region=region)


def refire_false_input(name):
    """(state, windows, the plan has a list) of a re-firing that cannot be fused."""
    w = lambda *pn: [(p0, n, float(WSTART), float(WEND)) for p0, n in pn]
    if name == "k33":
        return refire_input()[0], refire_wins(33), True
    if name == "union17":
        return refire_input(32)[0], w((10, 9), (18, 9)), True
    if name == "ring8-union9":
        return refire_input(8)[0], w((2, 5), (6, 5)), True
    return refire_input()[0], refire_wins(4), False


def case_refire_false(dev, name):
    st, wins, has_list = refire_false_input(name)
    slots = refire_input()[1]
    assert not check_refire(dev, st, agg=M.AGG_SUM_I64, wins=wins, slots=slots, list_n=257,
                            variant="all-chain-k64-clear", plan_list=has_list)


def ids(cases):
    return ["-".join(str(x).replace(" ", "") for x in (c if isinstance(c, tuple) else (c,)))
            for c in cases]
