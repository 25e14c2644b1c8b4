"""Plain reference model of the session engine (csrc/kernels_hip.hip, "Session windows on the
GPU"): Python ints, lists and dicts only -- no torch, no native code.

It states what the kernels compute, not where they put it: concurrent inserts make slot positions
nondeterministic, so tables are checked by their invariants (`check_table`, `check_set`) and every
other result is keyed by the session key.

  * hashing: `mix64`, `slot_hash`, the home slots of the slot table and of the spill set;
  * aggregates: `agg_lift`, `agg_combine`, `agg_result` on 64-bit accumulator bit patterns;
  * the fold of one key: `split_runs` (runs split at ts > prev + gap) and `fold_key`, which merges
    the runs into at most K_SESS resident sessions exactly as `sess_merge` states;
  * `fire_key`, and `SessionTable` with fold / fire / evict as operations on
    key -> (sessions, due, last) (a rehash is the identity on that map).

A session is a tuple (start, end, acc, cnt, flags): [start, end), acc the accumulator as a signed
64-bit bit pattern (what an int64 tensor shows), flags bit 0 = fired, bit 1 = modified since.
"""
import struct

K_SESS = 4
EMPTY_KEY, TOMB_KEY = -1, -2        # ~0ull and ~1ull seen through an int64 tensor
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
U64 = (1 << 64) - 1
U32 = (1 << 32) - 1
HOLE_T = 0xFFFFFFFF                 # record time of a padding hole
LONG_SEG = 96                       # kSessLongSeg: longer key segments take the wave kernel
LOOKUP_CHUNK = 8192                 # kLookupChunk: records per workgroup of the global lookup

(AGG_SUM_I64, AGG_SUM_F64, AGG_MIN_I64, AGG_MAX_I64, AGG_MIN_F64, AGG_MAX_F64, AGG_COUNT,
 AGG_AVG_F64, AGG_AVG_I64) = range(9)


def u64(x):
    return x & U64


def i64(x):
    x &= U64
    return x - (1 << 64) if x >> 63 else x


def f64_bits(x):
    """The double x as a signed 64-bit pattern."""
    return struct.unpack("<q", struct.pack("<d", float(x)))[0]


def as_f64(bits):
    return struct.unpack("<d", struct.pack("<Q", u64(bits)))[0]


# ---- hashing ------------------------------------------------------------------------------------
def mix64(x):
    x = u64(u64(x) + 0x9E3779B97F4A7C15)
    x = u64((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9)
    x = u64((x ^ (x >> 27)) * 0x94D049BB133111EB)
    return x ^ (x >> 31)


def slot_hash(key):
    key = u64(key)
    h = ((key & U32) * 0xCC9E2D51 & U32) ^ ((key >> 32) * 0x1B873593 & U32)
    h ^= h >> 16
    h = h * 0x85EBCA6B & U32
    h ^= h >> 13
    return h


def set_home(key, mask):
    return (mix64(key) >> 32) & mask


def table_insert(keys, sub, cap_log2, key):
    """Host-side insert of `key` into sub-table `sub` of the list `keys` (first empty slot of its
    chain; builds the starting tables of the tests). Returns the slot."""
    cap = 1 << cap_log2
    s = slot_hash(key) & (cap - 1)
    for _ in range(cap):
        k = keys[sub * cap + s]
        if k == key or k == EMPTY_KEY:
            keys[sub * cap + s] = key
            return sub * cap + s
        s = (s + 1) & (cap - 1)
    raise ValueError("sub-table full")


def set_insert(table, key):
    mask = len(table) - 1
    s = set_home(key, mask)
    for _ in range(len(table)):
        if table[s] == key or table[s] == EMPTY_KEY:
            table[s] = key
            return
        s = (s + 1) & mask
    raise ValueError("set full")


def check_table(keys, nsub, cap_log2):
    """Invariants of a slot table: a key appears once in its sub-table, and no empty slot lies
    between its home slot and its position (tombstones may). Returns {key: slot}."""
    cap = 1 << cap_log2
    assert len(keys) == nsub * cap
    where = {}
    for sub in range(nsub):
        row = keys[sub * cap:(sub + 1) * cap]
        seen = set()
        for pos, k in enumerate(row):
            if k in (EMPTY_KEY, TOMB_KEY):
                continue
            assert k not in seen, f"key {k} twice in sub-table {sub}"
            seen.add(k)
            s = slot_hash(k) & (cap - 1)
            while s != pos:
                assert row[s] != EMPTY_KEY, f"empty slot {s} before key {k} at {pos} (sub {sub})"
                s = (s + 1) & (cap - 1)
            where[(sub, k)] = sub * cap + pos
    return where


def check_set(table, want):
    """A spill set holds exactly the keys `want`, each once, reachable from its home entry."""
    mask = len(table) - 1
    live = [k for k in table if k not in (EMPTY_KEY, TOMB_KEY)]
    assert len(live) == len(set(live)), "a key twice in the set"
    assert set(live) == set(want)
    for pos, k in enumerate(table):
        if k in (EMPTY_KEY, TOMB_KEY):
            continue
        s = set_home(k, mask)
        while s != pos:
            assert table[s] != EMPTY_KEY, f"empty entry {s} before key {k} at {pos}"
            s = (s + 1) & mask


def set_contains(table, key):
    mask = len(table) - 1
    s = set_home(key, mask)
    for _ in range(len(table)):
        if table[s] == key:
            return True
        if table[s] == EMPTY_KEY:
            return False
        s = (s + 1) & mask
    return False


def lookup_sort_lds(cap_log2, m_cap):
    """Dynamic LDS bytes of the fused lookup-sort for m_cap staged records."""
    cap = 1 << cap_log2
    return max(cap * 8, cap * 2 + m_cap * 2) + m_cap * 8


# ---- aggregates ---------------------------------------------------------------------------------
def agg_lift(agg, v):
    return 1 if agg == AGG_COUNT else i64(v)


def agg_combine(agg, a, b):
    if agg in (AGG_SUM_I64, AGG_AVG_I64, AGG_COUNT):
        return i64(a + b)
    if agg in (AGG_SUM_F64, AGG_AVG_F64):
        return f64_bits(as_f64(a) + as_f64(b))
    if agg == AGG_MIN_I64:
        return a if a < b else b
    if agg == AGG_MAX_I64:
        return a if a > b else b
    if agg == AGG_MIN_F64:
        return a if as_f64(a) < as_f64(b) else b
    if agg == AGG_MAX_F64:
        return a if as_f64(a) > as_f64(b) else b
    raise ValueError(agg)


def agg_result(agg, acc, cnt):
    if agg in (AGG_SUM_F64, AGG_MIN_F64, AGG_MAX_F64):
        return as_f64(acc)
    if agg == AGG_AVG_F64:
        return as_f64(acc) / cnt if cnt else 0.0
    if agg == AGG_AVG_I64:
        return i64(acc) / cnt if cnt else 0.0
    if agg == AGG_COUNT:
        return float(cnt)
    return float(i64(acc))


# ---- the fold of one key ------------------------------------------------------------------------
def split_runs(recs, gap, agg):
    """recs: [(ts, value bits)] in (ts, arrival) order -> runs (start, end, acc, cnt), a new run
    wherever ts > previous ts + gap."""
    runs = []
    prev = None
    for ts, v in recs:
        v = agg_lift(agg, v)
        if prev is not None and ts <= prev + gap:
            s, _, a, c = runs[-1]
            runs[-1] = (s, ts + gap, agg_combine(agg, a, v), c + 1)
        else:
            runs.append((ts, ts + gap, v, 1))
        prev = ts
    return runs


def sess_due(sessions, lateness):
    due = I64_MAX
    for _, end, _, _, flags in sessions:
        d = end - 1 + lateness if (flags & 1) and not (flags & 2) else end - 1
        due = min(due, d)
    return due


def merge_run(sessions, run, lateness, wm, agg):
    """sess_merge: 0 merged / inserted (sessions updated in place), 1 late, 2 overflow."""
    ms, me, macc, mcnt = run
    mflags = 0
    hit = [s for s in sessions if ms <= s[1] and me >= s[0]]
    # (the kernel tests every session against the run as it stood before the merge, and again
    # against the merged interval when it clears the absorbed ones: the union of intervals that
    # intersect the run only ever contains sessions that intersect the run, because resident
    # sessions are pairwise disjoint by more than touching)
    for s in hit:
        ms, me = min(ms, s[0]), max(me, s[1])
    if not hit and (me - 1) + lateness <= wm:
        return 1
    if not hit and len(sessions) >= K_SESS:
        return 2
    for s in sessions:  # in position order: acc = combine(session, acc)
        if s in hit:
            macc = agg_combine(agg, s[2], macc)
            mcnt += s[3]
            mflags |= s[4]
    if mflags & 1:
        mflags |= 2
    absorbed = [s for s in sessions if ms <= s[1] and me >= s[0]]
    sessions[:] = [s for s in sessions if s not in absorbed] + [(ms, me, macc, mcnt, mflags)]
    return 0


def fold_key(sessions, last, recs, gap, lateness, wm, agg):
    """Fold one key's records (in (ts, arrival) order) into its sessions. Returns a dict:
    sessions (live ones, any order), due, last, late (records dropped), ovf (overflow runs)."""
    sessions = list(sessions)
    late, ovf, overflow = 0, [], False
    for run in split_runs(recs, gap, agg):
        res = 2 if overflow else merge_run(sessions, run, lateness, wm, agg)
        if res == 1:
            late += run[3]
        elif res == 2:
            overflow = True
            ovf.append(run)
    return dict(sessions=sessions, due=sess_due(sessions, lateness),
                last=max(last, recs[-1][0]), late=late, ovf=ovf)


def fire_key(sessions, wm, lateness):
    """Sessions with end - 1 <= wm that are unfired or modified fire (flags become 1); sessions
    past end - 1 + lateness <= wm leave. Returns (fired [(start, end, acc, cnt)], sessions, due)."""
    fired, keep = [], []
    for start, end, acc, cnt, flags in sessions:
        if end - 1 <= wm and (not (flags & 1) or (flags & 2)):
            fired.append((start, end, acc, cnt))
            flags = 1
        if not (end - 1) + lateness <= wm:
            keep.append((start, end, acc, cnt, flags))
    return fired, keep, sess_due(keep, lateness)


class SessionTable:
    """key -> [sessions, due, last]: the slot table as a map (positions left out)."""

    def __init__(self, gap, lateness, agg):
        self.gap, self.lateness, self.agg = gap, lateness, agg
        self.rows = {}
        self.late = 0

    def fold(self, events, wm):
        """events: [(key, ts, value bits)] in arrival order. Returns {key: overflow runs}."""
        by_key = {}
        for k, t, v in events:
            by_key.setdefault(k, []).append((t, v))
        ovf = {}
        for k, recs in by_key.items():
            recs.sort(key=lambda r: r[0])  # stable: equal timestamps keep arrival order
            sessions, _, last = self.rows.get(k, ([], I64_MAX, I64_MIN))
            r = fold_key(sessions, last, recs, self.gap, self.lateness, wm, self.agg)
            self.rows[k] = [r["sessions"], r["due"], r["last"]]
            self.late += r["late"]
            if r["ovf"]:
                ovf[k] = r["ovf"]
        return ovf

    def fire(self, wm):
        """Rows (key, start, end, acc, cnt) of every key whose due time has passed."""
        out = []
        for k, row in self.rows.items():
            if row[1] > wm:
                continue
            fired, row[0], row[1] = fire_key(row[0], wm, self.lateness)
            out += [(k,) + f for f in fired]
        return out

    def evict(self, keys=None, idle_before=I64_MIN):
        """Listed keys, or keys idle since before `idle_before`, leave the table. Returns
        (spilled {key: sessions}, freed keys): a key without a live session is only freed."""
        take = [k for k, row in self.rows.items()
                if (k in keys if keys is not None else row[2] < idle_before)]
        spilled, freed = {}, []
        for k in take:
            sessions = self.rows.pop(k)[0]
            if sessions:
                spilled[k] = sessions
            else:
                freed.append(k)
        return spilled, freed
