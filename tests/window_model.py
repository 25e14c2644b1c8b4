"""Plain reference model of the window firing path (csrc/kernels_hip.hip, "Window firing", and
its C++ twin in csrc/kernels_cpu.cpp): Python and numpy only -- no torch, no native code.

Every function states what one kernel computes, not where it puts it. The GPU kernels emit rows
in no particular order and concurrent inserts make slot positions nondeterministic, so rows are
keyed by their (unique) key, buckets are multisets and slot tables are checked by invariants.

The pane-major window state is `State`: keys (uint64, nslots), acc (uint64 bit patterns), cnt
(uint32), dirty (uint8) and -- for the touched-slot list -- mark (uint32, nslots); the ring arrays
are indexed ((pane mod ring) * nslots + slot). Python's % is right for negative panes; the
kernels use & (ring - 1).

Rows are a numpy record array (ROW: key, val, raw, cnt) in visiting order: val the f64 bit
pattern of the emitted value, raw the combined accumulator. The model is vectorised over slots
(the second-grid-round case has four million of them) and loops over panes and windows.

NaN: MIN/MAX_F64 select an operand and keep its bits, so a NaN's bits are specified. A NaN that
arithmetic *produces* (inf - inf) has no specified sign or payload; the test inputs avoid it.
"""
import copy

import numpy as np

from mxstream.ops import expr as E
from mxstream.utils import hashing as H
from session_model import slot_hash

(AGG_SUM_I64, AGG_SUM_F64, AGG_MIN_I64, AGG_MAX_I64, AGG_MIN_F64, AGG_MAX_F64, AGG_COUNT,
 AGG_AVG_F64, AGG_AVG_I64) = range(9)
AGGS = tuple(range(9))
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
U64 = (1 << 64) - 1
EMPTY_KEY = U64                      # ~0ull
REFIRE_PANES = 16                    # kRefireP: union panes one fused re-firing holds
FIRE_MULTI_MAX = 32                  # kFireMultiMax: windows per fused re-firing
STAT_COUNT, RED_WORDS = 8, 16
STAT_MAXTS, STAT_MINPANE, STAT_MAXPANE, STAT_LATE, STAT_OVERFLOW = range(5)

ROW = np.dtype([("key", "<u8"), ("val", "<u8"), ("raw", "<u8"), ("cnt", "<u4")])
_u64, _i64, _f64 = np.uint64, np.int64, np.float64


def i64(x):
    x &= U64
    return x - (1 << 64) if x >> 63 else x


# ---- aggregates (csrc/mxs_common.h: agg_combine, agg_identity, agg_result_f64) ------------------
def combine(agg, a, b):
    """Two partial accumulators (uint64 bit patterns, arrays or scalars) -> one."""
    a, b = np.asarray(a, dtype=_u64), np.asarray(b, dtype=_u64)
    with np.errstate(all="ignore"):
        if agg in (AGG_SUM_I64, AGG_AVG_I64, AGG_COUNT):
            return a + b                                      # wraps: two's complement
        if agg in (AGG_SUM_F64, AGG_AVG_F64):
            return (a.view(_f64) + b.view(_f64)).view(_u64)   # one rounding per addition
        if agg == AGG_MIN_I64:
            return np.where(a.view(_i64) < b.view(_i64), a, b)
        if agg == AGG_MAX_I64:
            return np.where(a.view(_i64) > b.view(_i64), a, b)
        if agg == AGG_MIN_F64:
            return np.where(a.view(_f64) < b.view(_f64), a, b)  # the chosen operand's bits
        if agg == AGG_MAX_F64:
            return np.where(a.view(_f64) > b.view(_f64), a, b)
    raise ValueError(agg)


def identity(agg):
    return {AGG_MIN_I64: I64_MAX, AGG_MAX_I64: 1 << 63, AGG_MIN_F64: 0x7FF0000000000000,
            AGG_MAX_F64: 0xFFF0000000000000}.get(agg, 0)


def result(agg, acc, cnt):
    """The window result as f64 (what the chained map sees)."""
    acc, cnt = np.asarray(acc, dtype=_u64), np.asarray(cnt, dtype=np.uint32)
    with np.errstate(all="ignore"):
        if agg in (AGG_SUM_F64, AGG_MIN_F64, AGG_MAX_F64):
            return acc.view(_f64)
        if agg == AGG_AVG_F64:
            return np.where(cnt == 0, 0.0, acc.view(_f64) / cnt.astype(_f64))
        if agg == AGG_AVG_I64:
            return np.where(cnt == 0, 0.0, acc.view(_i64).astype(_f64) / cnt.astype(_f64))
        if agg == AGG_COUNT:
            return cnt.astype(_f64)
        return acc.view(_i64).astype(_f64)


# ---- state --------------------------------------------------------------------------------------
class State:
    def __init__(self, keys, acc, cnt, dirty, ring, mark=None):
        self.keys = np.ascontiguousarray(keys, dtype=_u64)
        self.nslots, self.ring = len(self.keys), ring
        self.acc = np.ascontiguousarray(acc, dtype=_u64)
        self.cnt = np.ascontiguousarray(cnt, dtype=np.uint32)
        self.dirty = np.ascontiguousarray(dirty, dtype=np.uint8)
        self.mark = (np.zeros(self.nslots, np.uint32) if mark is None
                     else np.ascontiguousarray(mark, dtype=np.uint32))
        assert len(self.acc) == len(self.cnt) == len(self.dirty) == ring * self.nslots

    def index(self, pane, slots):
        return (pane % self.ring) * self.nslots + slots

    def copy(self):
        return copy.deepcopy(self)


def _epilogue(agg, key, acc, cnt, wstart, wend, map_prog, filt_prog):
    """(mapped value bits, emit mask) of combined slots. Variables, in order: result, count,
    window start, window end, (double)(uint64)key, (double)(int64)acc, mapped."""
    res = np.ascontiguousarray(result(agg, acc, cnt))
    n = len(key)
    vars_ = [res, cnt.astype(_f64), _f64(wstart), _f64(wend), key.astype(_f64),
             acc.view(_i64).astype(_f64), res]
    mapped = res
    if map_prog is not None and not map_prog.empty:
        mapped = np.ascontiguousarray(np.broadcast_to(E.eval_numpy(map_prog, vars_), (n,)))
    emit = np.ones(n, dtype=bool)
    if filt_prog is not None and not filt_prog.empty:
        vars_[E.VAR_MAPPED] = mapped
        emit = np.broadcast_to(E.eval_numpy(filt_prog, vars_), (n,)) != 0.0
    return mapped.astype(_f64).view(_u64), emit


def _combine_window(st, agg, p0, npanes, s, dirty_pane=None):
    """Panes p0 .. p0+npanes-1 of slots s that have a count, combined in ascending pane order.
    -> (acc, total count (uint32, wraps), some counted pane is dirty [and passes dirty_pane])."""
    acc = np.zeros(len(s), _u64)
    cnt = np.zeros(len(s), np.uint32)
    have = np.zeros(len(s), bool)
    dirty = np.zeros(len(s), bool)
    for pane in range(p0, p0 + npanes):
        gi = st.index(pane, s)
        c = st.cnt[gi]
        m = c != 0
        a = st.acc[gi]
        acc = np.where(m, np.where(have, combine(agg, acc, a), a), acc)
        have |= m
        cnt = cnt + np.where(m, c, np.uint32(0)).astype(np.uint32)
        if dirty_pane is None or dirty_pane(pane):
            dirty |= m & (st.dirty[gi] != 0)
    return acc, cnt, dirty


def fire(st, agg, p0, npanes, only_dirty, wstart, wend, map_prog=None, filt_prog=None, slots=None,
         dirty_pane=None):
    """window_fire: one row per visited slot (all of them, or the listed ones, in that order)
    whose window has a count -- with only_dirty, whose window has a counted pane with its dirty
    byte set -- and whose epilogue filter passes."""
    s = np.arange(st.nslots, dtype=_i64) if slots is None else np.asarray(slots, dtype=_i64)
    acc, cnt, dirty = _combine_window(st, agg, p0, npanes, s, dirty_pane)
    keep = cnt != 0
    if only_dirty:
        keep &= dirty
    s, acc, cnt = s[keep], acc[keep], cnt[keep]
    key = st.keys[s]
    val, emit = _epilogue(agg, key, acc, cnt, wstart, wend, map_prog, filt_prog)
    rows = np.empty(int(emit.sum()), dtype=ROW)
    rows["key"], rows["val"], rows["raw"], rows["cnt"] = key[emit], val[emit], acc[emit], cnt[emit]
    return rows


def fire_many(st, agg, only_dirty, map_prog, filt_prog, wins, slots=None):
    """window_fire_many: `fire` per window (p0, npanes, wstart, wend); rows in window order and
    the cumulative row counts."""
    per = [fire(st, agg, p0, npanes, only_dirty, ws, we, map_prog, filt_prog, slots)
           for p0, npanes, ws, we in wins]
    bounds = np.cumsum([len(r) for r in per], dtype=np.int64).astype(np.uint32)
    return (np.concatenate(per) if per else np.empty(0, ROW)), bounds


def refire_union(wins):
    u0 = min(w[0] for w in wins)
    return u0, max(w[0] + w[1] for w in wins)


def refire_many(st, agg, map_prog, filt_prog, wins, slots, dlo=0, dmask_abs=0, clear=False):
    """window_refire_many over the touched-slot list. None: the windows cannot be fused. Else
    (rows, bounds), and with `clear` the state afterwards as a third item."""
    k = len(wins)
    if k <= 0 or k > FIRE_MULTI_MAX or slots is None:
        return None
    u0, u1 = refire_union(wins)
    if u1 - u0 > REFIRE_PANES or u1 - u0 > st.ring:
        return None

    def in_mask(pane):
        b = pane - dlo
        return dmask_abs == 0 or (0 <= b < 31 and bool(dmask_abs >> b & 1))

    s = np.asarray(slots, dtype=_i64)
    per = [fire(st, agg, p0, npanes, True, ws, we, map_prog, filt_prog, s, in_mask)
           for p0, npanes, ws, we in wins]
    bounds = np.cumsum([len(r) for r in per], dtype=np.int64).astype(np.uint32)
    rows = np.concatenate(per)
    if not clear:
        return rows, bounds
    after = st.copy()
    after.mark[s] = 0
    for pane in range(u0, u1):
        if in_mask(pane):
            gi = st.index(pane, s)
            hit = gi[(st.cnt[gi] != 0) & (st.dirty[gi] != 0)]
            after.dirty[hit] = 0
    return rows, bounds, after


def dirty_clear(st, slots, p_lo, np_, delta=None):
    """dirty_clear_kernel: the listed slots' marks, and their dirty bytes (and delta ring
    entries, delta = (dacc, dcnt)) in panes p_lo .. p_lo + min(np_, ring) - 1.
    -> (state afterwards, delta afterwards)."""
    after = st.copy()
    s = np.asarray(slots, dtype=_i64)
    delta = None if delta is None else (delta[0].copy(), delta[1].copy())
    after.mark[s] = 0
    for pane in range(p_lo, p_lo + min(np_, st.ring)):
        gi = st.index(pane, s)
        after.dirty[gi] = 0
        if delta is not None:
            delta[0][gi] = 0
            delta[1][gi] = 0
    return after, delta


# ---- hashing ------------------------------------------------------------------------------------
def sub_table_of(key, nsub_log2):
    """csrc/mxs_common.h sub_table_of over uint64 keys (array or int)."""
    k = np.atleast_1d(np.asarray(key, dtype=_u64))
    if nsub_log2 == 0:
        return np.zeros(len(k), np.uint32)
    m = _u64(0xFFFFFFFF)
    h = ((k & m) * _u64(0x9E3779B1) & m) ^ ((k >> _u64(32)) * _u64(0x85EBCA77) & m)
    h ^= h >> _u64(15)
    h = h * _u64(0x2C1B3C6D) & m
    h ^= h >> _u64(13)
    return (h >> _u64(32 - nsub_log2)).astype(np.uint32)


def keygroups(keys, max_parallelism, jhash=None):
    """Flink key group of every key: murmur(Long.hashCode(key)) -- or murmur(jhash[key]) for
    dictionary ids -- mod max_parallelism."""
    out = []
    for k in np.asarray(keys, dtype=_u64).tolist():
        h = int(jhash[k]) if jhash is not None else H.java_long_hash(k)
        out.append(H.flink_murmur(h) % max_parallelism)
    return np.array(out, dtype=np.int32)


def scatter_partials(keys, acc, cnt, n, max_parallelism, nranks, nsub_log2, kg_dest, jhash,
                     bucket_cap, cursor=None):
    """scatter_partials_kernel: the first n rows -> records (key, acc, 0, cnt) of bucket
    (kg_dest[key group] << nsub_log2) | sub_table_of(key).
    -> (per bucket the list of every record sent to it, in row order -- a bucket stores
    bucket_cap - cursor of them at most --, the cursors afterwards (they count every row),
    the overflow flag)."""
    nb = nranks << nsub_log2
    keys = np.asarray(keys, dtype=_u64)[:n]
    cur = np.zeros(nb, np.int64) if cursor is None else np.asarray(cursor, dtype=np.int64).copy()
    kg = keygroups(keys, max_parallelism, jhash)
    b = (np.asarray(kg_dest)[kg].astype(np.int64) << nsub_log2) | sub_table_of(keys, nsub_log2)
    buckets = [[] for _ in range(nb)]
    for i, bi in enumerate(b.tolist()):
        buckets[bi].append((int(keys[i]), int(acc[i]), 0, int(cnt[i])))
        cur[bi] += 1
    return buckets, cur.astype(np.uint32), bool((cur > bucket_cap).any())


# ---- step prologue / epilogue -------------------------------------------------------------------
def stats_init():
    return [I64_MIN, I64_MAX, I64_MIN, 0, 0, 0, 0, 0]


def step_begin(nb):
    """step_begin_kernel: (cursors, stats) afterwards."""
    return [0] * nb, stats_init()


def step_finish(stats, local_maxts, bound, event_mode, proc_now, flags=None):
    """step_finish_kernel: (the 16-word all-reduce vector, local_maxts afterwards).
    [-qmax, qmin, wm, -bucket_ovf, -pane_ovf, record width, -table_full, -reserved key, stats[8]]"""
    lm = max(local_maxts, stats[STAT_MAXTS])
    wm = (I64_MIN if lm == I64_MIN else i64(lm - bound)) if event_mode else proc_now
    ovf = stats[STAT_OVERFLOW]
    qmax = stats[STAT_MAXPANE]
    red = [I64_MAX if qmax == I64_MIN else i64(-qmax), stats[STAT_MINPANE], wm, -(ovf & 1),
           -((ovf >> 1) & 1), -2 if ovf & 4 else -1 if ovf & 16 else 0,
           0 if flags is None else -(flags & 1), -((ovf >> 3) & 1)] + list(stats)
    assert len(red) == RED_WORDS
    return red, lm


# ---- slot table ---------------------------------------------------------------------------------
def table_insert(keys_g, keys, nsub_log2, cap_log2):
    """table_insert_kernel, one key after the other: a key takes the first empty slot of its
    chain in its sub-table (or the slot that already holds it).
    -> (keys_g afterwards, slots (-1: sub-table full), number of -1 entries)."""
    table = [int(k) for k in np.asarray(keys_g, dtype=_u64)]
    cap = 1 << cap_log2
    slots = []
    for key in np.asarray(keys, dtype=_u64).tolist():
        sub = int(sub_table_of(key, nsub_log2)[0])
        s = slot_hash(key) & (cap - 1)
        found = -1
        for _ in range(cap):
            k = table[sub * cap + s]
            if k == key or k == EMPTY_KEY:
                table[sub * cap + s] = key
                found = sub * cap + s
                break
            s = (s + 1) & (cap - 1)
        slots.append(found)
    return np.array(table, dtype=_u64), np.array(slots, dtype=np.int64), slots.count(-1)


def check_table(keys_g, keys, slots, nsub_log2, cap_log2, overflow):
    """Invariants of table_insert's result whatever the order of concurrent inserts."""
    cap = 1 << cap_log2
    table = np.asarray(keys_g, dtype=_u64).tolist()
    keys = np.asarray(keys, dtype=_u64).tolist()
    slots = np.asarray(slots).tolist()
    want_full = table_insert(np.full(len(table), EMPTY_KEY, _u64), sorted(set(keys)), nsub_log2,
                             cap_log2)
    full_subs = {int(sub_table_of(k, nsub_log2)[0])
                 for k, s in zip(sorted(set(keys)), want_full[1].tolist()) if s < 0}
    seen = {}
    for key, slot in zip(keys, slots):
        sub = int(sub_table_of(key, nsub_log2)[0])
        assert seen.setdefault(key, slot) == slot, f"key {key}: two slots"
        if slot < 0:
            assert slot == -1 and sub in full_subs, f"key {key}: -1 in a sub-table with room"
            assert key not in table[sub * cap:(sub + 1) * cap]
            continue
        assert slot // cap == sub and table[slot] == key, f"key {key}: slot {slot}"
        s = slot_hash(key) & (cap - 1)
        while sub * cap + s != slot:
            assert table[sub * cap + s] != EMPTY_KEY, f"empty slot before key {key}"
            s = (s + 1) & (cap - 1)
    assert slots.count(-1) == overflow
    live = [k for k in table if k != EMPTY_KEY]
    assert len(live) == len(set(live)) and set(live) <= set(keys)
