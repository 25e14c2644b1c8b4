"""The session kernels, called directly, against the plain model (needs an MI355X).

tests/session_model.py states what lookup, merge, fire, evict, the slot-table rehash and the
spill-set kernels compute; test_session_model.py checks that model against the CPU engine. Here
hand-built bucketed records (24-byte Rec and 16-byte RecC, with holes), sorted (slot | ts, value)
arrays and slot tables go through the native bindings, and everything they write is compared with
the model. Slot positions depend on the order of concurrent inserts and are the one thing not
compared: results are decoded through keys_g (slot -> key) and the tables are checked by their
invariants (session_model.check_table / check_set).

One property of the unfused path is built into the inputs rather than asserted: the global
lookup kernel (cap_log2 > 12) gives every 8192-record chunk of every bucket its output range
with an atomic, so records of one key with equal timestamps keep their arrival order only
inside a chunk. That kernel therefore gets a version of each step whose ties sit next to each
other in one chunk of one bucket (LookupInput.for_global); the LDS lookup and the fused kernel,
which promise (source rank, position) order, get ties across buckets as well. Every path must
emit its input in (ts, arrival) order.
"""
import copy
from collections import Counter

import numpy as np
import pytest
import torch

import session_model as M
from mxstream.ops import expr as E
from mxstream.ops import kernels as K
from mxstream.ops.native import load

pytestmark = pytest.mark.gpu

SENT = M.I64_MAX
FILL = 0x1122334455667788           # what untouched output words must still hold
REC24 = np.dtype([("key", "<i8"), ("val", "<i8"), ("t", "<u4"), ("aux", "<u4")])
REC16 = np.dtype([("key", "<i8"), ("val", "<i4"), ("t", "<u4")])
LDS_BUDGET = 156 * 1024             # dynamic LDS the fused lookup-sort may ask for


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _filled(n, dev, dtype=torch.int64):
    return torch.full((n,), FILL if dtype == torch.int64 else 0x11223344, dtype=dtype, device=dev)


# ---- slot-table state ---------------------------------------------------------------------------
class State:
    """keys_g, sess [nslots, 4, 4], the interleaved (due, last) [nslots, 2], the spill set and
    the counters: host arrays to build a starting state, device tensors to run on."""

    def __init__(self, nsub, cap_log2, spill_log2=6):
        self.nsub, self.cap_log2 = nsub, cap_log2
        self.nslots = nsub << cap_log2
        self.keys = [M.EMPTY_KEY] * self.nslots
        self.sess = np.zeros((self.nslots, M.K_SESS, 4), dtype=np.int64)
        self.meta = np.empty((self.nslots, 2), dtype=np.int64)
        self.meta[:, 0], self.meta[:, 1] = M.I64_MAX, M.I64_MIN
        self.spill = [M.EMPTY_KEY] * (1 << spill_log2)

    def seed(self, sub, key, sessions=(), last=M.I64_MIN, lateness=0, first_pos=0):
        """Insert `key` with its sessions at positions first_pos, first_pos + 1, ... (mod 4)."""
        slot = M.table_insert(self.keys, sub, self.cap_log2, key)
        self.sess[slot] = 0
        for j, (s, e, a, c, f) in enumerate(sessions):
            self.sess[slot, (first_pos + j) % M.K_SESS] = (s, e, a, c | f << 32)
        self.meta[slot] = (M.sess_due(sessions, lateness), last)
        return slot

    def bury(self, sub, key):
        """Insert `key` and tombstone it (keys seeded later chain past it)."""
        slot = M.table_insert(self.keys, sub, self.cap_log2, key)
        self.keys[slot] = M.TOMB_KEY
        return slot

    def upload(self, dev):
        self.dev = dev
        self.keys_g = torch.tensor(self.keys, dtype=torch.int64, device=dev)
        self.sess_g = _dev(self.sess, dev)
        self.meta_g = _dev(self.meta, dev)
        self.spill_g = torch.tensor(self.spill, dtype=torch.int64, device=dev)
        self.ctr = torch.zeros(16, dtype=torch.int32, device=dev)
        self.late = torch.zeros(1, dtype=torch.int64, device=dev)
        return self

    @property
    def due_ptr(self):
        return self.meta_g.data_ptr()

    @property
    def last_ptr(self):
        return self.meta_g[:, 1].data_ptr()

    def download(self):
        torch.cuda.synchronize(self.dev)
        return (self.keys_g.cpu().tolist(), self.sess_g.cpu().numpy(), self.meta_g.cpu().numpy(),
                self.spill_g.cpu().tolist())


def slot_sessions(row):
    """A slot's [4, 4] record -> its live sessions, sorted; free positions must be all zero."""
    out = []
    for s, e, a, w in row.tolist():
        if w & M.U32:
            out.append((s, e, a, w & M.U32, w >> 32))
        else:
            assert (s, e, a, w) == (0, 0, 0, 0), "a free position is not zero"
    return sorted(out)


def table_rows(keys, sess, meta):
    """{key: (sessions, due, last)} of every live slot."""
    return {k: (slot_sessions(sess[i]), int(meta[i, 0]), int(meta[i, 1]))
            for i, k in enumerate(keys) if k not in (M.EMPTY_KEY, M.TOMB_KEY)}


# =================================================================================================
# a. Lookup equivalence
# =================================================================================================
def _rand_keys(rng, n):
    """n distinct keys over the whole 64-bit range (seen as int64), none of them a marker."""
    out = set()
    while len(out) < n:
        out.update(int(k) for k in rng.integers(M.I64_MIN, M.I64_MAX, n - len(out), dtype=np.int64)
                   if int(k) not in (M.EMPTY_KEY, M.TOMB_KEY))
    return sorted(out, key=lambda k: M.mix64(k))


def _slot_hash_np(k):
    """session_model.slot_hash over a uint64 array."""
    m = np.uint64(M.U32)
    h = ((k & m) * np.uint64(0xCC9E2D51) & m) ^ ((k >> np.uint64(32)) * np.uint64(0x1B873593) & m)
    h ^= h >> np.uint64(16)
    h = h * np.uint64(0x85EBCA6B) & m
    return h ^ (h >> np.uint64(13))


class LookupInput:
    """Bucketed records of one step and the table contents they meet.

    Per sub-table: `resident` keys (half of them receive records), `buried` tombstones, `fresh`
    keys new to the table and `spilled` keys that sit in the spill set. A sub-table's records
    are generated in arrival order (source-major) and cut into the nsrc buckets.

    Two versions of the records differ only in their equal timestamps. `words` repeats the key
    and time of any earlier record of the sub-table, in whatever bucket: the LDS lookup and the
    fused kernel promise (source rank, position) order for those. `for_global()` keeps only
    repeats of the direct predecessor inside one chunk of one bucket, the order the global
    lookup kernel fixes."""

    def __init__(self, seed, nsub, nsrc, counts, rw, *, nres=0, nburied=0, nfresh=0, nspilled=0,
                 holes=True, hot=None, bcap=None, over=0):
        rng = np.random.default_rng(seed)
        self.nsub, self.nsrc, self.rw = nsub, nsrc, rw
        dt = REC24 if rw == 3 else REC16
        self.resident, self.buried, self.fresh, self.spilled = [], [], [], []
        arrival, near, cuts = [], [], []
        for sub in range(nsub):
            ks = _rand_keys(rng, nres + nburied + nfresh + nspilled + 1)
            res, ks = ks[:nres], ks[nres:]
            bur, ks = ks[:nburied], ks[nburied:]
            fre, ks = ks[:nfresh], ks[nfresh:]
            spi = ks[:nspilled]
            if hot is not None:
                res = list(hot[sub])
            pool = res[:(len(res) + 1) // 2] + fre + spi
            if not pool:
                pool = fre = [ks[-1]]
            self.resident.append(res)
            self.buried.append(bur)
            self.fresh.append(fre)
            self.spilled.append(spi)
            c = counts[sub]
            r = np.zeros(c, dtype=dt)
            r["key"] = np.array(pool, dtype=np.int64)[rng.integers(0, len(pool), c)]
            r["t"] = rng.permutation(c).astype(np.uint32) + 5
            if rw == 3:
                r["val"] = rng.integers(M.I64_MIN, M.I64_MAX, c, dtype=np.int64)
                r["aux"] = rng.integers(0, 1 << 32, c, dtype=np.uint32)
            else:
                r["val"] = rng.integers(-(1 << 31), 1 << 31, c, dtype=np.int64)
            # buckets: nsrc contiguous pieces of uneven length (some empty)
            cut = np.sort(rng.integers(0, c + 1, nsrc - 1)) if bcap is None else \
                np.minimum(np.arange(1, nsrc) * bcap, c)
            cut = [0] + cut.tolist() + [c]
            # equal timestamps: a record repeats its predecessor's key and time (other value),
            # inside one lookup chunk of one bucket
            for i in np.flatnonzero(rng.random(c) < 0.3).tolist():
                src = max(s for s in range(nsrc) if cut[s] <= i)
                if i > cut[src] and (i - cut[src]) % M.LOOKUP_CHUNK:
                    r["key"][i], r["t"][i] = r["key"][i - 1], r["t"][i - 1]
            x = r.copy()
            for i in np.flatnonzero(rng.random(c) < 0.15).tolist():
                if i:
                    j = int(rng.integers(0, i))
                    x["key"][i], x["t"][i] = x["key"][j], x["t"][j]
            if holes and c:
                hole = rng.random(c) < 0.06
                r["t"][hole] = x["t"][hole] = M.HOLE_T
            arrival.append(x)
            near.append(r)
            cuts.append(cut)
        longest = max(cuts[s][j + 1] - cuts[s][j] for s in range(nsub) for j in range(nsrc))
        self.bcap = bcap or max(8, (longest + 7) & ~7)
        self.counts = np.zeros(nsrc * nsub, dtype=np.int32)
        bufs = []
        for recs in (arrival, near):
            buf = np.zeros(nsrc * nsub * self.bcap, dtype=dt)
            buf.view(np.uint8)[:] = 0x5A
            for sub in range(nsub):
                for src in range(nsrc):
                    piece = recs[sub][cuts[sub][src]:cuts[sub][src + 1]]
                    b = src * nsub + sub
                    buf[b * self.bcap:b * self.bcap + len(piece)] = piece
                    # a bucket count above bucket_cap is clamped by the kernels
                    self.counts[b] = len(piece) + (over if len(piece) == self.bcap else 0)
            bufs.append(buf.view(np.int64))
        self.words, self._near_words = bufs

    def for_global(self):
        """The same step with equal timestamps only next to each other in one lookup chunk."""
        other = copy.copy(self)
        other.words = self._near_words
        return other

    def for_path(self, path):
        return self.for_global() if path == "global" else self

    def state(self, cap_log2, *, fill=False, spill_log2=None):
        """The starting table at this sub-table size. fill: no tombstones, and every slot the
        resident keys leave free takes a filler key whose home slot it is (a full sub-table)."""
        n = max(len(s) + len(f) for s, f in zip(self.spilled, self.fresh)) * 2 + 16
        st = State(self.nsub, cap_log2, spill_log2 or max(4, int(n).bit_length()))
        cap = 1 << cap_log2
        for sub in range(self.nsub):
            for k in () if fill else self.buried[sub]:
                st.bury(sub, k)
            for j, k in enumerate(self.resident[sub]):
                st.seed(sub, k, [(j, j + 3, 7, 1, 0)], last=j)
            if fill:
                cand = np.arange(20 * cap + 64, dtype=np.uint64) + np.uint64(1 + sub * (20 * cap + 64))
                home, first = np.unique(_slot_hash_np(cand) & np.uint64(cap - 1), return_index=True)
                assert len(home) == cap
                for h, i in zip(home.tolist(), first.tolist()):
                    if st.keys[sub * cap + h] == M.EMPTY_KEY:
                        st.keys[sub * cap + h] = int(cand[i])
            for k in self.spilled[sub]:
                M.set_insert(st.spill, k)
        return st


def run_lookup(path, dev, inp, st, *, spill_any=1, host_cap=None, tbits=20, skip=None, skip_mask=0):
    """One lookup through `path` (lds / global: gpu_session_lookup + gpu_sort_pairs; fused0 /
    fused1: gpu_session_lookup_sort with pair 0 / 1). Returns what it wrote, as host data."""
    m = load()
    st.upload(dev)
    total = inp.nsrc * inp.nsub * inp.bcap
    host_cap = total if host_cap is None else host_cap
    recs, counts = _dev(inp.words, dev), _dev(inp.counts, dev)
    host = _filled(3 * host_cap + 96, dev)
    heads = _filled(total + 8, dev)
    sk_out, vals_out = _filled(2 * total + 8, dev), _filled(total + 8, dev)
    c, s = st.ctr, _stream(dev)
    common = (recs.data_ptr(), counts.data_ptr(), inp.nsrc, inp.nsub, inp.bcap, st.cap_log2,
              st.keys_g.data_ptr(), st.spill_g.data_ptr(), len(st.spill) - 1, spill_any)
    tail = (c[0:1].data_ptr(), host.data_ptr(), c[2:3].data_ptr(), host_cap, c[3:4].data_ptr(),
            tbits, s)
    launched = True
    if path in ("lds", "global"):
        assert (st.cap_log2 > 12) == (path == "global")
        sk_in, vals_in = _filled(total + 8, dev), _filled(total + 8, dev)
        m.gpu_session_lookup(*common, sk_in.data_ptr(), vals_in.data_ptr(), *tail,
                             rec_words=inp.rw)
        n = int(c[0])
        if n:
            nbits = tbits + st.nslots.bit_length()
            need = m.gpu_sort_pairs_temp_bytes(n, 0, nbits)
            tmp = torch.empty(need, dtype=torch.uint8, device=dev)
            m.gpu_sort_pairs(tmp.data_ptr(), need, sk_in.data_ptr(), sk_out.data_ptr(),
                             vals_in.data_ptr(), vals_out.data_ptr(), n, 0, nbits, s)
        sk, vals = sk_out.cpu().numpy(), vals_out.cpu().numpy()
    else:
        pair = int(path == "fused1")
        launched = m.gpu_session_lookup_sort(
            *common, sk_out.data_ptr(), vals_out.data_ptr(), *tail,
            skip.data_ptr() if skip is not None else 0, skip_mask, heads.data_ptr(),
            c[10:11].data_ptr(), pair, rec_words=inp.rw)
        raw = sk_out.cpu().numpy()
        if pair:
            sk, vals = raw[0::2], raw[1::2]
        else:
            sk, vals = raw, vals_out.cpu().numpy()
    keys1, _, _, spill1 = st.download()
    ctr = c.cpu().tolist()
    hostw = host.cpu().numpy()
    return dict(path=path, launched=launched, n_out=ctr[0], n_host=ctr[2], n_ins=ctr[3],
                n_heads=ctr[10], sk=sk, vals=vals, heads=heads.cpu().numpy(), keys=keys1,
                spill=spill1, host=hostw[:3 * host_cap].view(REC24), guard=hostw[3 * host_cap:],
                host_cap=host_cap, tbits=tbits, ctr=ctr)


def _rec_tuples(r, rw):
    aux = r["aux"].tolist() if rw == 3 else [0] * len(r)
    return list(zip(r["key"].tolist(), r["val"].tolist(), r["t"].tolist(), aux))


def check_lookup(out, inp, st0, *, spill_any=1, full=False):
    """Everything section a of the test plan asserts for one path's output."""
    nsub, cap_log2, tbits = inp.nsub, st0.cap_log2, out["tbits"]
    fused = out["path"].startswith("fused")
    keys0, keys1 = st0.keys, out["keys"]
    where0 = M.check_table(keys0, nsub, cap_log2)
    where1 = M.check_table(keys1, nsub, cap_log2)
    spill0 = {k for k in st0.spill if k not in (M.EMPTY_KEY, M.TOMB_KEY)}
    want_seq, want_host, new_kept, to_set, n_clamped, spilled_seen = {}, Counter(), set(), set(), 0, 0
    for sub in range(nsub):
        pieces = []
        for src in range(inp.nsrc):
            b = src * nsub + sub
            n = min(int(inp.counts[b]), inp.bcap)
            pieces.append(inp.words.view(REC24 if inp.rw == 3 else REC16)[b * inp.bcap:b * inp.bcap + n])
        arr = np.concatenate(pieces)
        n_clamped += len(arr)
        by_key = {}
        for r in _rec_tuples(arr, inp.rw):
            if r[2] != M.HOLE_T:
                by_key.setdefault(r[0], []).append(r)
        for key, recs in by_key.items():
            if (sub, key) in where0:
                host = False
            elif spill_any and key in spill0:
                host, spilled_seen = True, spilled_seen + 1
            elif full:
                host = True
                to_set.add(key)
            else:
                host = False
                new_kept.add((sub, key))
            if host:
                want_host.update(recs)
            else:  # (ts, arrival) order: the sort is stable
                want_seq[(sub, key)] = sorted(((r[2], r[1]) for r in recs), key=lambda x: x[0])
    kept = sum(len(v) for v in want_seq.values())

    # -- output records: sorted by (slot, ts), one contiguous segment per key, values in place.
    # The radix sort orders the whole array. The fused kernel sorts each sub-table in its own
    # workgroup, which takes its output range with an atomic: the sub-tables' ranges follow each
    # other in any order (the merge goes by the segment list), each sorted in itself.
    n_out = out["n_out"]
    sk, vals = out["sk"][:n_out], out["vals"][:n_out]
    if fused:
        assert n_out == kept             # no holes, no diverted records
        assert np.all(out["sk"][n_out:] == FILL) and np.all(out["vals"][n_out:] == FILL)
    else:
        assert n_out == n_clamped        # holes and diverted records are sentinels, sorted last
        assert int((sk != SENT).sum()) == kept and np.all(sk[kept:] == SENT)
        sk, vals = sk[:kept], vals[:kept]
    slots, ts = sk >> tbits, sk & ((1 << tbits) - 1)
    subs = slots >> cap_log2
    if fused:
        same = subs[1:] == subs[:-1]
        assert np.all(np.diff(sk)[same] >= 0)
        starts = subs[np.r_[True, ~same]] if kept else subs
        assert len(set(starts.tolist())) == len(starts), "a sub-table's range is not contiguous"
    else:
        assert np.all(np.diff(sk) >= 0)
    got_seq, segs = {}, set()
    bounds = [0] + (np.flatnonzero(np.diff(slots)) + 1).tolist() + [kept] if kept else [0]
    for a, b in zip(bounds, bounds[1:]):
        slot = int(slots[a])
        key = keys1[slot]
        assert (slot >> cap_log2, key) not in got_seq, "a key's segment is not contiguous"
        got_seq[(slot >> cap_log2, key)] = list(zip(ts[a:b].tolist(), vals[a:b].tolist()))
        assert where1[(slot >> cap_log2, key)] == slot
        segs.add(a | (b - a) << 32)
    assert got_seq == want_seq
    if fused:
        assert out["n_heads"] == len(want_seq)
        heads = out["heads"][:out["n_heads"]].tolist()
        assert len(set(heads)) == len(heads) and set(heads) == segs
        assert np.all(out["heads"][out["n_heads"]:] == FILL)

    # -- the table: new keys counted, nothing else touched
    assert set(where1) == set(where0) | new_kept
    assert out["n_ins"] == len(new_kept)
    new_tombs = 0
    for i, (a, b) in enumerate(zip(keys0, keys1)):
        if a == b:
            continue
        assert a in (M.EMPTY_KEY, M.TOMB_KEY), f"slot {i} held {a}, now {b}"
        if b == M.TOMB_KEY:
            new_tombs += 1
        else:
            assert (i >> cap_log2, b) in new_kept
    # (the fused kernel claims a slot for a key it then finds in the spill set, and frees it
    # again as a tombstone; the unfused one asks the set first)
    if fused and not full and M.TOMB_KEY not in keys0:
        assert new_tombs == spilled_seen
    else:
        assert new_tombs <= (spilled_seen if fused else 0)

    # -- records of spilled keys (and of keys a full sub-table turned away) go to the host
    assert out["n_host"] == sum(want_host.values())
    assert np.all(out["guard"] == FILL), "written past host_cap"
    got_host = Counter(_rec_tuples(out["host"][:min(out["n_host"], out["host_cap"])], 3))
    if out["n_host"] <= out["host_cap"]:
        assert got_host == want_host
    else:
        assert not got_host - want_host
    M.check_set(out["spill"], spill0 | to_set)
    if not to_set:
        assert out["spill"] == st0.spill
    return kept


# (nsub, nsrc, LDS cap_log2, records of sub-table 0): every count meets several geometries
_GEOM = [(1, 1, 6), (3, 2, 3), (3, 64, 12), (1, 2, 1), (3, 1, 12), (1, 64, 6)]
_SHAPES = [g + (c,) for i, c in enumerate((0, 1, 63, 64, 65, 1023, 1024, 1025))
           for g in (_GEOM[i % 6], _GEOM[(i + 2) % 6], _GEOM[(i + 3) % 6])]
_SHAPES += [(1, 1, 6, 8192 + 77),      # two chunks of the global lookup kernel
            (3, 1, 12, 8192 + 5000)]


def _mix_for(cap_log2, count):
    """Key categories that fit the sub-table (fresh + spilled keys never exceed its free slots)."""
    if cap_log2 == 1:
        return dict(nres=1, nfresh=1)
    if cap_log2 == 3:
        return dict(nres=2, nburied=1, nfresh=2, nspilled=1)
    if cap_log2 == 6 or count < 200:
        return dict(nres=10, nburied=4, nfresh=12, nspilled=5)
    return dict(nres=300, nburied=50, nfresh=500, nspilled=40)


def _four_paths(dev, inp, cap_log2, **kw):
    kept = None
    for path, cl in (("lds", cap_log2), ("global", 13), ("fused0", cap_log2), ("fused1", cap_log2)):
        st0, x = inp.state(cl), inp.for_path(path)
        out = run_lookup(path, dev, x, inp.state(cl), **kw)
        assert out["launched"]
        k = check_lookup(out, x, st0, spill_any=kw.get("spill_any", 1))
        if path != "global":             # (where the ties differ, its records carry other keys)
            assert kept in (None, k)
            kept = k
    return kept


@pytest.mark.parametrize("rw", [2, 3])
@pytest.mark.parametrize("nsub,nsrc,cap_log2,count", _SHAPES)
def test_lookup_paths_agree(gpu_device, nsub, nsrc, cap_log2, count, rw):
    """The LDS lookup + radix sort, the global lookup + radix sort and the fused lookup-sort
    (two arrays / pairs) on the same buckets: resident, fresh and spilled keys, tombstones to
    reuse, holes and equal timestamps. Sub-table 0 holds `count` records, the others fewer."""
    counts = [count, count // 2, min(count, 1)][:nsub]
    inp = LookupInput(1000 * count + 10 * cap_log2 + rw, nsub, nsrc, counts, rw,
                      **_mix_for(cap_log2, count))
    kept = _four_paths(gpu_device, inp, cap_log2)
    assert kept > 0 or count < 2


def _lds_max(cap_log2):
    """The most records (a multiple of 8) the fused kernel stages for this sub-table size."""
    m = (LDS_BUDGET // 10) & ~7
    while M.lookup_sort_lds(cap_log2, m + 8) <= LDS_BUDGET:
        m += 8
    while M.lookup_sort_lds(cap_log2, m) > LDS_BUDGET:
        m -= 8
    return m


@pytest.mark.parametrize("rw", [2, 3])
@pytest.mark.parametrize("cap_log2,nsrc", [(6, 1), (12, 2)])
def test_lookup_lds_maximum(gpu_device, cap_log2, nsrc, rw):
    """As many records as the fused kernel's LDS holds (the largest workgroup): 15,960 for 64
    slots in one bucket, 15,152 for 4,096 slots in two."""
    m = _lds_max(cap_log2)
    assert m == {6: 15960, 12: 15152}[cap_log2] and m % (8 * nsrc) == 0
    inp = LookupInput(7 + rw, 1, nsrc, [m], rw, bcap=m // nsrc, **_mix_for(cap_log2, m))
    assert inp.bcap * nsrc == m
    assert _four_paths(gpu_device, inp, cap_log2) > m // 2


def _keys_with_home(home, mask, n, start=1):
    out, k = [], start
    while len(out) < n:
        if M.slot_hash(k) & mask == home:
            out.append(k)
        k += 1
    return out


@pytest.mark.parametrize("rw", [2, 3])
@pytest.mark.parametrize("count", [1025, 15960])
def test_lookup_one_hot_key(gpu_device, count, rw):
    """Every record of the sub-table belongs to one key, with many equal timestamps: the ranking
    walks the whole segment for every record (the largest m: 15,960 records)."""
    hot = [[_keys_with_home(5, 63, 1)[0]]]
    inp = LookupInput(3 + rw, 1, 1, [count], rw, hot=hot, bcap=(count + 7) & ~7, holes=False)
    assert _four_paths(gpu_device, inp, 6) == count


@pytest.mark.parametrize("rw", [2, 3])
@pytest.mark.parametrize("k", [0, 7, 31])
def test_lookup_two_hot_keys_share_a_cursor_word(gpu_device, k, rw):
    """Two hot keys on the adjacent slots 2k and 2k + 1: their u16 cursors are the two halves
    of one 32-bit word."""
    a = _keys_with_home(2 * k, 63, 1)[0]
    b = _keys_with_home(2 * k + 1, 63, 1)[0]
    inp = LookupInput(5 + k + rw, 1, 2, [3000], rw, hot=[[a, b]])
    st = inp.state(6)
    assert sorted(i for i, x in enumerate(st.keys) if x != M.EMPTY_KEY) == [2 * k, 2 * k + 1]
    assert _four_paths(gpu_device, inp, 6) > 2500


@pytest.mark.parametrize("rw", [2, 3])
def test_lookup_bucket_counts_are_clamped(gpu_device, rw):
    """Bucket counts above bucket_cap (an overflowed partition): only bucket_cap records are
    read from each such bucket."""
    inp = LookupInput(21 + rw, 3, 2, [128, 128, 128], rw, bcap=64, over=1000, **_mix_for(6, 128))
    assert int(inp.counts.max()) == 1064
    _four_paths(gpu_device, inp, 6)


@pytest.mark.parametrize("rw", [2, 3])
def test_lookup_spill_set_not_consulted(gpu_device, rw):
    """spill_any = 0: keys that sit in the spill set are inserted and folded like any other."""
    inp = LookupInput(31 + rw, 3, 2, [300, 150, 1], rw, **_mix_for(6, 300))
    assert any(inp.spilled)
    for path, cl in (("lds", 6), ("global", 13), ("fused0", 6), ("fused1", 6)):
        out = run_lookup(path, gpu_device, inp.for_path(path), inp.state(cl), spill_any=0)
        assert out["n_host"] == 0
        check_lookup(out, inp.for_path(path), inp.state(cl), spill_any=0)


@pytest.mark.parametrize("rw", [2, 3])
def test_lookup_spilled_keys_leave_tombstones(gpu_device, rw):
    """A table without tombstones: the unfused lookups leave none, the fused one leaves exactly
    one per spilled key that received records (the slot it claimed before asking the set)."""
    inp = LookupInput(35 + rw, 3, 2, [300, 150, 1], rw, nres=10, nfresh=12, nspilled=5)
    assert M.TOMB_KEY not in inp.state(6).keys
    for path, cl in (("lds", 6), ("global", 13), ("fused0", 6), ("fused1", 6)):
        out = run_lookup(path, gpu_device, inp.for_path(path), inp.state(cl))
        check_lookup(out, inp.for_path(path), inp.state(cl))
        assert out["n_host"] > 0
        assert (M.TOMB_KEY in out["keys"]) == path.startswith("fused")


@pytest.mark.parametrize("rw", [2, 3])
@pytest.mark.parametrize("cap_log2", [1, 3, 6])
def test_lookup_full_sub_table(gpu_device, cap_log2, rw):
    """No free slot and no tombstone: keys new to the table land in the spill set and their
    records in host_recs; resident keys still fold. All four paths: the global kernel meets the
    same buckets with its 8,192-slot sub-tables filled."""
    mix = _mix_for(cap_log2, 500)
    mix.pop("nspilled", None)
    inp = LookupInput(41 + rw, 3, 2, [500, 250, 9], rw, **mix)
    for path, cl in (("lds", cap_log2), ("global", 13), ("fused0", cap_log2), ("fused1", cap_log2)):
        st0, x = inp.state(cl, fill=True, spill_log2=8), inp.for_path(path)
        assert M.EMPTY_KEY not in st0.keys and M.TOMB_KEY not in st0.keys
        out = run_lookup(path, gpu_device, x, inp.state(cl, fill=True, spill_log2=8))
        kept = check_lookup(out, x, st0, full=True)
        assert kept > 0 and out["n_host"] > 0 and out["n_ins"] == 0


@pytest.mark.parametrize("rw", [2, 3])
def test_lookup_host_buffer_overflow(gpu_device, rw):
    """More diverted records than host_cap: n_host is exact, nothing is written past the cap."""
    inp = LookupInput(51 + rw, 3, 2, [600, 300, 1], rw, **_mix_for(6, 600))
    for path, cl in (("lds", 6), ("global", 13), ("fused0", 6), ("fused1", 6)):
        out = run_lookup(path, gpu_device, inp.for_path(path), inp.state(cl), host_cap=16)
        assert out["n_host"] > 16
        check_lookup(out, inp.for_path(path), inp.state(cl))


@pytest.mark.parametrize("pair", [0, 1])
@pytest.mark.parametrize("word,masked", [(3, True), (5, True), (6, False)])
def test_lookup_sort_skip_word(gpu_device, pair, word, masked):
    """A non-zero word of the reduced vector under skip_mask: the fused kernel leaves every
    output and counter untouched. A non-zero word outside the mask changes nothing."""
    inp = LookupInput(61, 3, 2, [300, 150, 1], 2, **_mix_for(6, 300))
    skip = torch.zeros(32, dtype=torch.int64, device=gpu_device)
    skip[word] = -1
    st0 = inp.state(6)
    out = run_lookup(f"fused{pair}", gpu_device, inp, inp.state(6), skip=skip,
                     skip_mask=1 << 3 | 1 << 4 | 1 << 5 | 1 << 7)
    assert out["launched"]
    if not masked:
        check_lookup(out, inp, st0)
        return
    assert out["ctr"] == [0] * 16
    assert out["keys"] == st0.keys and out["spill"] == st0.spill
    for name in ("sk", "vals", "heads", "guard"):
        assert np.all(out[name] == FILL), name
    assert np.all(out["host"].view(np.int64) == FILL)


@pytest.mark.parametrize("why,nsrc,cap_log2,bcap,launches", [
    ("nsrc > 64", 65, 6, 8, False),
    ("cap_log2 = 13", 1, 13, 64, False),
    ("nsrc * bcap > 65535", 2, 6, 32768, False),
    ("LDS: the largest bcap that fits", 1, 6, 15960, True),
    ("LDS: 8 records more", 1, 6, 15968, False),
])
def test_lookup_sort_launcher_refuses(gpu_device, why, nsrc, cap_log2, bcap, launches):
    """gpu_session_lookup_sort returns False and launches nothing when the step cannot be staged
    in LDS (the operator then takes the lookup + radix sort path)."""
    assert (M.lookup_sort_lds(6, 15960) <= LDS_BUDGET < M.lookup_sort_lds(6, 15968))
    inp = LookupInput(71, 1, nsrc, [40], 3, bcap=bcap, nres=3, nfresh=3)
    st0 = inp.state(cap_log2)
    out = run_lookup("fused1", gpu_device, inp, inp.state(cap_log2))
    assert out["launched"] == launches, why
    if launches:
        check_lookup(out, inp, st0)
        return
    assert out["ctr"] == [0] * 16 and out["keys"] == st0.keys
    assert np.all(out["sk"] == FILL) and np.all(out["heads"] == FILL)


# =================================================================================================
# b. Merge
# =================================================================================================
MERGES = ["scan", "heads0", "heads1"]
GAP = 10


def run_merge(kernel, dev, segs, pre=None, *, gap=GAP, lateness=0, wm=M.I64_MIN, tbase=1000,
              tbits=20, agg=K.AGG_SUM_I64, cap_log2=7, nsub=2, ovf_cap=64, seed=0, tail=True):
    """Merge key segments [(slot, [(ts, value bits), ...])] (slots ascending, records in ts
    order) into a table that holds `pre` = {slot: (sessions, last)}, with gpu_session_merge
    (`scan`: segment heads found by scanning the keys; `tail`: sentinels after them) or
    gpu_session_merge_heads (`heads0` two arrays, `heads1` interleaved pairs; the segment list
    shuffled). Compares everything the merge writes with the model."""
    m, pre = load(), pre or {}
    rng = np.random.default_rng(seed)
    st = State(nsub, cap_log2)
    for slot in set(pre) | {s for s, _ in segs}:
        st.keys[slot] = 100_000 + 7 * slot
        sessions, last = pre.get(slot, ((), M.I64_MIN))
        for j, (s, e, a, c, f) in enumerate(sessions):
            st.sess[slot, (slot + j) % M.K_SESS] = (s, e, a, c | f << 32)
        st.meta[slot] = (M.sess_due(sessions, lateness), last)
    st.upload(dev)
    assert [s for s, _ in segs] == sorted({s for s, _ in segs})
    sk = [slot << tbits | (t - tbase) for slot, recs in segs for t, _ in recs]
    assert all(0 <= t - tbase < 1 << tbits for _, recs in segs for t, _ in recs)
    vals = [v for _, recs in segs for _, v in recs]
    n = len(sk)
    ntail = 5 if kernel == "scan" and tail else 0
    sk_t = torch.tensor(sk + [SENT] * ntail + [FILL] * 4, dtype=torch.int64, device=dev)
    vals_t = torch.tensor(vals + [0] * ntail + [FILL] * 4, dtype=torch.int64, device=dev)
    c = st.ctr
    c[0] = n + ntail
    long_heads = torch.zeros(n + 8, dtype=torch.int32, device=dev)
    ovf_slots = _filled(2 * len(segs) + 8, dev)
    ovf_rows = _filled(5 * ovf_cap + 32, dev)
    args = (tbits, gap, lateness, wm, tbase, agg, cap_log2, st.nslots, st.sess_g.data_ptr(),
            st.due_ptr, st.last_ptr, st.late.data_ptr(), st.keys_g.data_ptr(),
            ovf_slots.data_ptr(), c[4:5].data_ptr(), ovf_rows.data_ptr(), c[5:6].data_ptr(),
            ovf_cap, _stream(dev))
    if kernel == "scan":
        m.gpu_session_merge(sk_t.data_ptr(), vals_t.data_ptr(), c[0:1].data_ptr(),
                            long_heads.data_ptr(), c[1:2].data_ptr(), n + ntail, *args)
    else:
        pos, heads = 0, []
        for _, recs in segs:
            heads.append(pos | len(recs) << 32)
            pos += len(recs)
        heads = [heads[i] for i in rng.permutation(len(heads))]
        heads_t = torch.tensor(heads + [FILL], dtype=torch.int64, device=dev)
        c[10] = len(heads)
        pair = int(kernel == "heads1")
        if pair:
            sk_t = torch.stack([sk_t, vals_t], dim=1).contiguous().view(-1)
        m.gpu_session_merge_heads(sk_t.data_ptr(), vals_t.data_ptr(), c[0:1].data_ptr(),
                                  heads_t.data_ptr(), c[10:11].data_ptr(), len(heads),
                                  long_heads.data_ptr(), c[1:2].data_ptr(), *args, pair)
    keys1, sess1, meta1, _ = st.download()
    ctr = c.cpu().tolist()

    # ---- the model
    want_sess, want_meta = st.sess.copy(), st.meta.copy()
    late, ovf_pairs, ovf_runs, touched = 0, Counter(), Counter(), set()
    for slot, recs in segs:
        sessions, last = pre.get(slot, ((), M.I64_MIN))
        r = M.fold_key(sessions, last, recs, gap, lateness, wm, agg)
        touched.add(slot)
        assert slot_sessions(sess1[slot]) == sorted(r["sessions"]), f"slot {slot}"
        assert (int(meta1[slot, 0]), int(meta1[slot, 1])) == (r["due"], r["last"]), f"slot {slot}"
        late += r["late"]
        if r["ovf"]:
            ovf_pairs[(slot, st.keys[slot])] += 1
            ovf_runs.update((slot,) + run for run in r["ovf"])
    rest = [i for i in range(st.nslots) if i not in touched]
    assert np.array_equal(sess1[rest], want_sess[rest]) and np.array_equal(meta1[rest], want_meta[rest])
    assert keys1 == st.keys
    assert int(st.late.cpu()[0]) == late
    assert ctr[1] == sum(len(recs) > M.LONG_SEG for _, recs in segs)   # queued for the wave kernel
    assert ctr[4] == sum(ovf_pairs.values())
    os_ = ovf_slots.cpu().numpy()
    assert Counter(zip(os_[0:2 * ctr[4]:2].tolist(), os_[1:2 * ctr[4]:2].tolist())) == ovf_pairs
    assert np.all(os_[2 * ctr[4]:] == FILL)
    assert ctr[5] == sum(ovf_runs.values())
    orow = ovf_rows.cpu().numpy()
    assert np.all(orow[5 * ovf_cap:] == FILL), "written past ovf_cap"
    w = min(ctr[5], ovf_cap)
    got = Counter(zip(*(orow[j * ovf_cap:j * ovf_cap + w].tolist() for j in range(5))))
    if ctr[5] <= ovf_cap:
        assert got == ovf_runs
    else:
        assert not got - ovf_runs
    return dict(late=late, n_ovf=ctr[4], n_ovf_runs=ctr[5],
                rows={s: slot_sessions(sess1[s]) for s in touched})


def _segment(rng, length, t0=2000, p_split=None, vals=None):
    """`length` records from t0 on: steps of 0 (equal timestamps), 1, GAP (still one run) and,
    with probability p_split, GAP + 1 or more (a new run)."""
    p = 2.0 / length if p_split is None else p_split
    steps = np.where(rng.random(length) < p, rng.choice([GAP + 1, GAP + 7], length),
                     rng.choice([0, 1, 1, GAP], length))
    ts = t0 + np.cumsum(steps)
    v = rng.integers(-1000, 1000, length) if vals is None else vals
    return [(int(t), int(x)) for t, x in zip(ts, v)]


@pytest.mark.parametrize("kernel", MERGES)
@pytest.mark.parametrize("place", ["first", "middle", "last"])
@pytest.mark.parametrize("length", [1, 2, 63, 64, 65, 96, 97, 128, 129, 200, 1500])
def test_merge_segment_lengths(gpu_device, length, place, kernel):
    """One key segment of `length` records first, in the middle or last in the array (the
    segment then ends at n), among short segments and one other long one: 96 records is the last
    length the thread-per-key walk takes, 97 the first for the wave kernel."""
    rng = np.random.default_rng(length)
    others = [(s, _segment(rng, int(n))) for s, n in
              zip((20, 30, 40, 140, 150, 160), (1, 3, 2, 5, 130, 4))]
    slot = {"first": 3, "middle": 77, "last": 250}[place]
    segs = sorted(others + [(slot, _segment(rng, length))])
    pre = {30: ([(1990, 2001, 5, 2, 0)], 1991), slot: ([(1500, 1510, -3, 1, 1)], 1500)}
    run_merge(kernel, gpu_device, segs, pre, wm=1400, lateness=500, seed=length,
              tail=place != "last")


@pytest.mark.parametrize("kernel", MERGES)
@pytest.mark.parametrize("step", [GAP, GAP + 1])
@pytest.mark.parametrize("length,at", [(n, at) for n in (96, 97, 200) for at in
                                       ((62, 63), (63, 64), (64, 65), (95, 96), (96, 97), (127, 128))
                                       if at[1] < n])
def test_merge_gap_boundaries(gpu_device, length, at, step, kernel):
    """Records one millisecond apart except between the pair `at`: a step of exactly `gap`
    keeps one run (which, at 200 records, spans three 64-record chunks of the wave kernel), a step
    of gap + 1 splits it there -- at the chunk edges just as anywhere else. 96 records take the
    serial walk, 97 and 200 the wave kernel. (In the wave kernel the lanes' split at
    ts > prev + gap is backed by lane 0, which joins a run that starts at or before the pending
    run's end: were the lanes to split at exactly `gap` too, lane 0 would join the halves again
    and the sessions would be the same. What must hold, and is asserted, is the sessions.)"""
    ts = [3000 + i + (step - 1 if i >= at[1] else 0) for i in range(length)]
    seg = [(t, i + 1) for i, t in enumerate(ts)]
    r = run_merge(kernel, gpu_device, [(9, [(2500, 1)]), (10, seg), (11, [(2500, 1)])])
    a = at[1]
    total = length * (length + 1) // 2
    if step == GAP:
        assert r["rows"][10] == [(3000, ts[-1] + GAP, total, length, 0)]
    else:
        assert r["rows"][10] == [(3000, ts[a - 1] + GAP, a * (a + 1) // 2, a, 0),
                                 (ts[a], ts[-1] + GAP, total - a * (a + 1) // 2, length - a, 0)]


@pytest.mark.parametrize("kernel", MERGES)
@pytest.mark.parametrize("length", [5, 150])
def test_merge_into_resident_sessions(gpu_device, length, kernel):
    """Runs that meet sessions already in the slot: one bridges two sessions into one, one
    re-opens a fired session (flags 3), one is late and dropped while a later run of the same
    key is kept -- through the serial walk (5 records) and the wave kernel (150)."""
    pre = {
        # [2000,2010) and [2030,2040): records 2010..2030 bridge them
        5: ([(2000, 2010, 100, 3, 0), (2030, 2040, 50, 2, 0)], 2030),
        # fired [3000,3010): a record at 3005 re-opens it
        6: ([(3000, 3010, 7, 1, 1), (2000, 2005, 1, 1, 1)], 3000),
        # wm 5000, lateness 100: a run ending before 4900 is late, one at 6000 is kept
        7: ([(5990, 6001, 9, 4, 0)], 5991),
    }
    n = length
    bridge = [(2010 + (20 * i) // max(n - 1, 1), i) for i in range(n)]
    assert all(b[0] - a[0] <= GAP for a, b in zip(bridge, bridge[1:]))
    reopen = [(3005 + min(i, 3), 2) for i in range(n)]
    mixed = [(4000 + min(i, 5), 1) for i in range(n - 1)] + [(6000, 5)]
    r = run_merge(kernel, gpu_device, [(5, bridge), (6, reopen), (7, mixed)], pre,
                  wm=5000, lateness=100)
    assert r["rows"][5] == [(2000, 2040, 150 + n * (n - 1) // 2, 5 + n, 0)]
    assert r["rows"][6] == [(2000, 2005, 1, 1, 1), (3000, 3008 + GAP, 7 + 2 * n, 1 + n, 3)]
    assert r["rows"][7] == [(5990, 6010, 14, 5, 0)] and r["late"] == n - 1


@pytest.mark.parametrize("kernel", MERGES)
@pytest.mark.parametrize("length", [4, 120])
@pytest.mark.parametrize("ovf_cap", [64, 2])
def test_merge_overflow(gpu_device, ovf_cap, length, kernel):
    """Four resident sessions and a disjoint fifth run: it overflows, and so does every later
    run of that key (even one that would have merged). With ovf_cap 2 the three keys' overflow
    runs outnumber the buffer: the count is exact and nothing is written past the cap."""
    four = [(1000 + 100 * j, 1010 + 100 * j, j, 1, 0) for j in range(4)]
    pre = {s: (four, 1300) for s in (40, 41, 42)}
    inside = [(1105, 3)] * (length - 3)            # merges into [1100, 1110)
    seg = inside + [(1500, 1), (1600, 2), (1700, 4)]
    late_then = [(1205, 1), (1250, 8), (1305, 9)]  # 1250 overflows; 1305 would have merged
    r = run_merge(kernel, gpu_device, [(40, seg), (41, late_then), (42, [(1800, 1)] * length)],
                  pre, ovf_cap=ovf_cap)
    assert r["n_ovf"] == 3 and r["n_ovf_runs"] == 3 + 2 + 1
    assert (1100, 1115, 1 + 3 * (length - 3), length - 2, 0) in r["rows"][40]
    assert (1300, 1310, 3, 1, 0) in r["rows"][41]


@pytest.mark.parametrize("kernel", MERGES)
@pytest.mark.parametrize("tbits,tbase", [(20, 7), (32, 1_700_000_000_000), (32, -5_000_000_000)])
def test_merge_time_bits_and_base(gpu_device, tbits, tbase, kernel):
    """Sort keys of 20 and 32 time bits over a non-zero time base (relative times up to the
    last representable one); wm = I64_MIN: nothing is late."""
    rng = np.random.default_rng(tbits)
    top = tbase + (1 << tbits) - 1
    segs = [(3, _segment(rng, 40, t0=tbase)), (4, _segment(rng, 300, t0=tbase + 5)),
            (200, [(tbase, 1), (top - GAP, 2), (top, 3)]),
            (255, [(top - 1, 1)] * 100 + [(top, -1)] * 30)]
    pre = {3: ([(tbase - 50, tbase - 40, 1, 1, 1)], tbase - 50)}
    r = run_merge(kernel, gpu_device, segs, pre, tbits=tbits, tbase=tbase, lateness=5)
    assert r["late"] == 0
    assert r["rows"][200] == [(tbase, tbase + GAP, 1, 1, 0), (top - GAP, top + GAP, 5, 2, 0)]
    assert r["rows"][255] == [(top - 1, top + GAP, 70, 130, 0)]


def _f(x):
    return M.f64_bits(x)


@pytest.mark.parametrize("kernel", MERGES)
@pytest.mark.parametrize("agg", [K.AGG_SUM_I64, K.AGG_MIN_I64, K.AGG_MAX_I64, K.AGG_COUNT,
                                 K.AGG_SUM_F64, K.AGG_MIN_F64, K.AGG_MAX_F64, K.AGG_AVG_F64])
def test_merge_aggregates(gpu_device, agg, kernel):
    """Every aggregate through the serial walk (segments of 3, 50 and 96 records) and the wave
    scan (97, 200 and 700), into slots that hold sessions. Float values are integer-valued
    doubles below 2^20, so every partial sum is exact whatever the order of the combines; the
    accumulators are compared bit for bit. Zeros of both signs are left out of the float min/max:
    agg_combine keeps the second operand when neither compares less, so -0.0 against +0.0 would
    depend on the order in which the wave scan and the serial walk combine."""
    rng = np.random.default_rng(agg)
    is_f = agg in K.AGG_IS_F64

    def val(x):
        return _f(float(x)) if is_f else int(x)

    segs, pre = [], {}
    for slot, n in zip((2, 9, 17, 64, 65, 200), (3, 50, 96, 97, 200, 700)):
        xs = rng.integers(-(1 << 19), 1 << 19, n)
        xs[xs == 0] = 1
        segs.append((slot, _segment(rng, n, vals=[val(x) for x in xs])))
        t0 = segs[-1][1][0][0]
        pre[slot] = ([(t0 - 5, t0 + 1, val(-7 if slot % 2 else 600_000), 2, 0)], t0 - 5)
    run_merge(kernel, gpu_device, segs, pre, agg=agg)


# =================================================================================================
# c. Fire
# =================================================================================================
def _fire_state(agg, wm, lateness, nsub, cap_log2, seed):
    """A table whose slots hold every kind of session a fire meets, relative to wm."""
    rng = np.random.default_rng(seed)
    is_f = agg in K.AGG_IS_F64
    st = State(nsub, cap_log2)
    cap = 1 << cap_log2
    kinds = [
        (wm + 1 - 40, wm + 1, 0),            # end - 1 == wm: fires
        (wm + 2 - 40, wm + 2, 0),            # end - 1 == wm + 1: not yet
        (wm - 90, wm - 50, 1),               # fired, unmodified, inside the lateness: stays
        (wm - 90, wm - 50, 3),               # fired and re-opened: fires again
        (wm - 900, wm - lateness + 1, 1),    # end - 1 + lateness == wm: dropped
        (wm - 900, wm - lateness + 2, 1),    # one ms inside the lateness: stays
        (wm - 2000, wm - 1500, 0),           # unfired and past cleanup: fires and leaves
        (wm + 500, wm + 600, 0),             # open
    ]
    model = {}
    for sub in range(nsub):
        for n, key in enumerate(_rand_keys(rng, int(cap * 0.6))):
            # the first keys hold one kind each, so every boundary is met; the others a mix
            pick = [n] if n < len(kinds) else rng.permutation(len(kinds))[:int(rng.integers(0, 5))]
            sessions = []
            for q in sorted(pick):
                s, e, f = kinds[q]
                cnt = int(rng.integers(1, 9))
                tot = cnt * int(rng.integers(-50, 50))       # AVG: sum / cnt is exact
                acc = M.f64_bits(float(tot)) if is_f else tot
                sessions.append((s, e, acc, cnt, f))
            sessions = _disjoint(sessions)   # (some kinds overlap: a key keeps one of them)
            st.seed(sub, key, sessions, last=0, lateness=lateness, first_pos=int(rng.integers(0, 4)))
            model[key] = sessions
    return st, model


def _disjoint(sessions):
    """Keep sessions that do not touch an earlier one (the table's invariant)."""
    out = []
    for s in sorted(sessions):
        if all(s[0] > o[1] or s[1] < o[0] for o in out):
            out.append(s)
    return out


@pytest.mark.parametrize("agg", [K.AGG_SUM_I64, K.AGG_COUNT, K.AGG_MAX_F64, K.AGG_AVG_F64])
@pytest.mark.parametrize("prog", ["plain", "map+filter"])
@pytest.mark.parametrize("out_cap", [4096, 40])
def test_fire(gpu_device, native, out_cap, prog, agg):
    """Fire a 3 x 128-slot table (384 slots: not a multiple of the 256-lane block) at wm: due and
    not-due slots, sessions at end - 1 == wm and wm + 1, fired sessions inside and past the
    lateness, a map (result * 2) and a filter (count >= 2), and an out_cap below the row count
    (exact count, nothing past the cap)."""
    wm, lateness = 10_000, 300
    st, model = _fire_state(agg, wm, lateness, 3, 7, seed=agg)
    st.upload(gpu_device)
    mapped = prog != "plain"
    mp = E.compile_expr(E.var(E.VAR_RESULT) * 2.0) if mapped else E.EMPTY
    fp = E.compile_expr(E.var(E.VAR_COUNT) >= 2) if mapped else E.EMPTY
    cols = [_filled(out_cap + 16, gpu_device) for _ in range(5)]
    ocnt = _filled(out_cap + 16, gpu_device, torch.int32)
    ov = cols[3].view(torch.float64)
    native.gpu_session_fire(GAP, lateness, wm, agg, 7, st.nslots, st.keys_g.data_ptr(),
                            st.sess_g.data_ptr(), st.due_ptr, *mp.as_args(), *fp.as_args(),
                            cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(),
                            ov.data_ptr(), cols[4].data_ptr(), ocnt.data_ptr(),
                            st.ctr[6:7].data_ptr(), out_cap, _stream(gpu_device))
    keys1, sess1, meta1, _ = st.download()
    n = int(st.ctr[6])
    want_rows, want_state = Counter(), {}
    for key, sessions in model.items():
        due0 = M.sess_due(sessions, lateness)
        if due0 > wm:                                  # not due: the slot is not touched
            want_state[key] = (sorted(sessions), due0, 0)
            continue
        fired, keep, due = M.fire_key(sessions, wm, lateness)
        want_state[key] = (sorted(keep), due, 0)
        for s, e, acc, cnt in fired:
            v = M.agg_result(agg, acc, cnt)
            if not mapped or cnt >= 2:
                want_rows[(key, s, e, v * 2.0 if mapped else v, acc, cnt)] += 1
    assert n == sum(want_rows.values()) and (n > out_cap) == (out_cap == 40)
    w = min(n, out_cap)
    h = [c.cpu().numpy() for c in cols]
    got = Counter(zip(h[0][:w].tolist(), h[1][:w].tolist(), h[2][:w].tolist(),
                      h[3][:w].view(np.float64).tolist(), h[4][:w].tolist(),
                      ocnt.cpu().numpy()[:w].tolist()))
    if n <= out_cap:
        assert got == want_rows
    else:
        assert not got - want_rows
    for c in h:
        assert np.all(c[out_cap:] == FILL), "written past out_cap"
    assert np.all(ocnt.cpu().numpy()[out_cap:] == 0x11223344)
    assert keys1 == st.keys
    assert table_rows(keys1, sess1, meta1) == want_state
    kinds = Counter(f for v in model.values() for *_, f in v)
    assert kinds[0] and kinds[1] and kinds[3]
    ends = {e for v in model.values() for _, e, *_ in v}
    for e in (wm + 1, wm + 2, wm - 50, wm - lateness + 1, wm - lateness + 2, wm - 1500, wm + 600):
        assert e in ends, f"no session ends at {e}"
    assert {(wm - 50, 1), (wm - 50, 3)} <= {(e, f) for v in model.values() for _, e, _, _, f in v}


# =================================================================================================
# d. Evict and rehash
# =================================================================================================
def _evict_state(nsub, cap_log2, seed):
    """Slots that are idle (last < 5000) or not, with 0..4 live sessions, and tombstones."""
    rng = np.random.default_rng(seed)
    st = State(nsub, cap_log2, spill_log2=(nsub << cap_log2).bit_length() + 1)
    model = {}
    for sub in range(nsub):
        keys = _rand_keys(rng, int((1 << cap_log2) * 0.7))
        for i, key in enumerate(keys):
            if i % 9 == 0:
                st.bury(sub, key)
                continue
            ns = int(rng.integers(0, 5))
            sessions = [(1000 * j + int(rng.integers(0, 100)), 1000 * j + 500, int(rng.integers(-9, 9)),
                         int(rng.integers(1, 5)), int(rng.choice([0, 1, 3]))) for j in range(ns)]
            last = int(rng.choice([100, 4999, 5000, 9000]))
            st.seed(sub, key, sessions, last=last, first_pos=int(rng.integers(0, 4)))
            model[key] = (sorted(sessions), M.sess_due(sessions, 0), last)
    return st, model


def _run_evict(native, dev, st, *, idle_before=M.I64_MIN, slots=None, row_cap):
    st.upload(dev)
    rows = torch.zeros((6, row_cap + 16), dtype=torch.int64, device=dev)
    rows[:, row_cap:] = FILL
    rows[4, :row_cap] = 0                                   # cnt pre-zeroed, as the operator does
    sl = torch.tensor(slots, dtype=torch.int64, device=dev) if slots is not None else None
    native.gpu_session_evict(st.nslots, st.cap_log2, st.keys_g.data_ptr(), st.sess_g.data_ptr(),
                             st.due_ptr, st.last_ptr, idle_before,
                             sl.data_ptr() if sl is not None else 0, len(slots or ()),
                             st.spill_g.data_ptr(), len(st.spill) - 1,
                             *(rows[j].data_ptr() for j in range(6)), st.ctr[7:8].data_ptr(),
                             row_cap, st.ctr[8:9].data_ptr(), _stream(dev))
    keys1, sess1, meta1, spill1 = st.download()
    return keys1, sess1, meta1, spill1, rows.cpu().numpy(), st.ctr.cpu().tolist()


def _check_evict(st, model, chosen, res, row_cap):
    """chosen: the keys the eviction must consider. Every one of them without a live session is
    freed; the others are spilled -- all of them if the rows fit, else exactly those whose rows
    were written, the rest staying resident with their state intact."""
    keys1, sess1, meta1, spill1, rows, ctr = res
    assert np.all(rows[:, row_cap:] == FILL), "written past row_cap"
    need = sum(len(model[k][0]) for k in chosen)
    assert ctr[7] == need
    written = rows[:, :row_cap][:, rows[4, :row_cap] != 0]
    got = {}
    for k, s, e, a, c, f in zip(*written.tolist()):
        got.setdefault(k, []).append((s, e, a, c, f))
    got = {k: sorted(v) for k, v in got.items()}
    after = table_rows(keys1, sess1, meta1)
    freed = {k for k in chosen if not model[k][0]}
    if need <= row_cap:
        assert set(got) == set(chosen) - freed
    else:
        assert set(got) < set(chosen) - freed       # some rows did not fit: holes in the staging
    for k, v in got.items():
        assert v == model[k][0]                      # whole keys, never part of one
    gone = set(got) | freed
    assert ctr[8] == len(gone)
    assert after == {k: v for k, v in model.items() if k not in gone}
    M.check_table(keys1, st.nsub, st.cap_log2)
    M.check_set(spill1, set(got))
    for i, (a, b) in enumerate(zip(st.keys, keys1)):
        if a in gone:
            assert b == M.TOMB_KEY and not sess1[i][:, 3].any()
            assert (int(meta1[i, 0]), int(meta1[i, 1])) == (M.I64_MAX, M.I64_MIN)
        else:
            assert a == b
    return got, freed


@pytest.mark.parametrize("nsub,cap_log2", [(3, 6), (3, 9)])
@pytest.mark.parametrize("mode", ["idle", "listed"])
@pytest.mark.parametrize("room", ["fits", "short"])
def test_evict(gpu_device, native, room, mode, nsub, cap_log2):
    """Idle eviction (last < idle_before) and listed-slot eviction of 192- and 1,536-slot tables
    (the second makes the 1,024-lane block loop iterate), with staging rows for everything and
    with a third of them (skipped keys leave holes and stay resident)."""
    st, model = _evict_state(nsub, cap_log2, seed=cap_log2)
    if mode == "idle":
        chosen = [k for k, v in model.items() if v[2] < 5000]
        kw = dict(idle_before=5000)
    else:
        rng = np.random.default_rng(1)
        live = [i for i, k in enumerate(st.keys) if k not in (M.EMPTY_KEY, M.TOMB_KEY)]
        slots = [live[i] for i in rng.permutation(len(live))[:len(live) // 2]]
        tomb = st.keys.index(M.TOMB_KEY)
        empty = st.keys.index(M.EMPTY_KEY)
        chosen = [st.keys[i] for i in slots]
        kw = dict(slots=slots + [tomb, empty])          # dead slots in the list are passed over
    need = sum(len(model[k][0]) for k in chosen)
    assert need > 40 and any(not model[k][0] for k in chosen)
    row_cap = need if room == "fits" else need // 3
    res = _run_evict(native, gpu_device, st, row_cap=row_cap, **kw)
    got, freed = _check_evict(st, model, chosen, res, row_cap)
    assert freed and got


def test_rehash_drops_tombstones(gpu_device, native):
    """gpu_session_rehash of a table with tombstones: the same keys with the same sessions, due
    and last; no tombstone; every key reachable from its home slot; `inserted` = live keys."""
    st, model = _evict_state(3, 9, seed=4)
    st.upload(gpu_device)
    new = State(3, 9).upload(gpu_device)
    native.gpu_session_rehash(st.nslots, 9, st.keys_g.data_ptr(), st.sess_g.data_ptr(),
                              st.due_ptr, st.last_ptr, new.keys_g.data_ptr(),
                              new.sess_g.data_ptr(), new.due_ptr, new.last_ptr,
                              new.ctr[9:10].data_ptr(), _stream(gpu_device))
    keys1, sess1, meta1, _ = new.download()
    assert M.TOMB_KEY in st.keys and M.TOMB_KEY not in keys1
    where = M.check_table(keys1, 3, 9)
    assert {(s, k) for s in range(3) for k in st.keys[s << 9:(s + 1) << 9]
            if k not in (M.EMPTY_KEY, M.TOMB_KEY)} == set(where)
    assert table_rows(keys1, sess1, meta1) == model
    assert int(new.ctr[9]) == len(model)
    for i, k in enumerate(keys1):
        if k == M.EMPTY_KEY:
            assert not sess1[i].any() and tuple(meta1[i]) == (M.I64_MAX, M.I64_MIN)
    old = st.download()
    assert old[0] == st.keys and np.array_equal(old[1], st.sess)   # the old table is only read


# =================================================================================================
# e. Spill-set kernels
# =================================================================================================
class DevSet:
    def __init__(self, native, dev, log2):
        self.m, self.dev, self.size = native, dev, 1 << log2
        self.t = torch.full((self.size,), M.EMPTY_KEY, dtype=torch.int64, device=dev)

    def _keys(self, keys):
        return torch.tensor(list(keys), dtype=torch.int64, device=self.dev)

    def insert(self, keys):
        k = self._keys(keys)
        self.m.gpu_set_insert(self.t.data_ptr(), self.size - 1, k.data_ptr(), len(k), _stream(self.dev))

    def erase(self, keys):
        k = self._keys(keys)
        self.m.gpu_set_erase(self.t.data_ptr(), self.size - 1, k.data_ptr(), len(k), _stream(self.dev))

    def probe(self, keys):
        k = self._keys(keys)
        hit = torch.full((len(k) + 8,), 7, dtype=torch.uint8, device=self.dev)
        n_hit = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self.m.gpu_set_probe(self.t.data_ptr(), self.size - 1, k.data_ptr(), len(k),
                             hit.data_ptr(), n_hit.data_ptr(), _stream(self.dev))
        h = hit.cpu().tolist()
        assert h[len(k):] == [7] * 8
        return h[:len(k)], int(n_hit)

    def list(self):
        return self.t.cpu().tolist()


@pytest.mark.parametrize("log2", [4, 12])
def test_spill_set_kernels(gpu_device, native, log2):
    """Insert (with duplicates in one batch), probe, erase, probe behind the tombstones,
    re-insert and rehash of 16- and 4,096-entry sets kept at most half full, against a Python set."""
    rng = np.random.default_rng(log2)
    ds, ref = DevSet(native, gpu_device, log2), set()
    half = (1 << log2) // 2
    universe = _rand_keys(rng, 2 * half + 300)
    first = universe[:half]
    ds.insert(first + first[:half // 2] + first[:3] * 5)       # duplicates in one batch
    ref.update(first)
    M.check_set(ds.list(), ref)
    probe = [universe[i] for i in rng.permutation(len(universe))[:2 * half + 300 - 1]]
    assert len(probe) % 256
    hits, n = ds.probe(probe)
    assert hits == [int(k in ref) for k in probe] and n == sum(hits)
    assert ds.probe([]) == ([], 0)                              # n = 0: nothing is launched
    # erase every other key: their entries become tombstones, the keys behind stay reachable
    gone = first[::2]
    ds.erase(gone + [universe[-1]])                             # (and a key that is not there)
    ref.difference_update(gone)
    tab = ds.list()
    assert tab.count(M.TOMB_KEY) == len(gone)
    M.check_set(tab, ref)
    hits, n = ds.probe(probe)
    assert hits == [int(k in ref) for k in probe] and n == sum(hits) == sum(k in ref for k in probe)
    # an erased key comes back once, and a kept key is not entered twice
    again = gone[:max(1, len(gone) // 4)]
    ds.insert(again + first[1:2])
    ref.update(again)
    M.check_set(ds.list(), ref)
    # rehash into a set twice the size: live keys only
    big = DevSet(native, gpu_device, log2 + 1)
    native.gpu_set_rehash(ds.t.data_ptr(), ds.size, big.t.data_ptr(), big.size - 1,
                          _stream(gpu_device))
    tab = big.list()
    assert M.TOMB_KEY not in tab
    M.check_set(tab, ref)
    hits, n = big.probe(probe)
    assert hits == [int(k in ref) for k in probe] and n == sum(hits)
