"""Window-join kernels (csrc/join_hip.hip, twins csrc/join_cpu.cpp) and the engine operator
(runtime/join_window_operator.py). Every comparison is exact: bit patterns and multisets."""
from __future__ import annotations

import functools
from collections import Counter

import numpy as np
import pytest
import torch

from mxstream.ops import kernels as K
from mxstream.runtime.join_window_operator import KeyedJoinWindowOperator

NAN = 0x7FF8000000000000
SPECIAL = np.array([0x7FF8000000000001, 0xFFF8000000000000, NAN], dtype=np.uint64).view(np.float64)
SPECIAL = np.concatenate([SPECIAL, [-0.0, 0.0, np.inf, -np.inf, 2.0 ** 53, -2.0 ** 53]])


def _canon(bits: np.ndarray) -> np.ndarray:
    """What comes back for a stored f64 bit pattern: itself, every NaN canonical."""
    v = bits.view(np.float64)
    return np.where(np.isnan(v), np.int64(NAN), bits.view(np.int64))


def _values(rng, n: int) -> np.ndarray:
    v = rng.standard_normal(n)
    hit = rng.random(n) < 0.2
    v[hit] = rng.choice(SPECIAL, int(hit.sum()))
    return v


class Side:
    def __init__(self, keys, lens, vals):
        self.keys_l, self.lens = [int(k) for k in keys], [int(x) for x in lens]
        self.vals = np.ascontiguousarray(vals, dtype=np.float64)
        assert self.vals.size == sum(self.lens)
        starts = np.concatenate([[0], np.cumsum(self.lens)[:-1]]) if self.lens else []
        self.keys = torch.tensor(self.keys_l, dtype=torch.int64)
        self.heads = torch.tensor(np.asarray(starts, dtype=np.int64))
        self.total = int(self.vals.size)
        self.ord = K.f64_order_bits(torch.from_numpy(self.vals.view(np.int64).copy()))

    def to(self, dev):
        c = object.__new__(Side)
        c.__dict__.update(self.__dict__)
        c.keys, c.heads, c.ord = self.keys.to(dev), self.heads.to(dev), self.ord.to(dev)
        return c


def _plan(l: Side, r: Side, **kw):
    return K.join_plan(l.keys, l.heads, l.total, r.keys, r.heads, r.total, **kw)


def _expand(jp, l: Side, r: Side, p0: int, p1: int) -> np.ndarray:
    k, a, b = K.join_expand(jp, l.ord, r.ord, p0, p1)
    return np.stack([k.cpu().numpy(), a.cpu().numpy(), b.cpu().numpy()])


def _brute(l: Side, r: Side) -> np.ndarray:
    """The nested loop, in Python: for every left key that the right side has, left-major."""
    lb, rb = _canon(l.vals), _canon(r.vals)
    rpos = {k: j for j, k in enumerate(r.keys_l)}
    rows = []
    for i, key in enumerate(l.keys_l):
        j = rpos.get(key)
        if j is None:
            continue
        l0, r0 = int(l.heads[i]), int(r.heads[j])
        for a in range(l.lens[i]):
            for b in range(r.lens[j]):
                rows.append((key, int(lb[l0 + a]), int(rb[r0 + b])))
    return np.array(rows, dtype=np.int64).reshape(-1, 3).T


def _interleaved(rng, nkeys: int, max_len: int):
    """Keys only left, only right and common; the first and the last left segment unmatched,
    runs of unmatched left segments between matched ones."""
    kind = rng.integers(0, 3, nkeys)          # 0 = left only, 1 = right only, 2 = common
    kind[:2], kind[-2:] = [0, 1], [1, 0]      # ends: left-only outermost, right-only next
    kind[10:14], kind[14], kind[9] = 0, 2, 2  # a run of unmatched lefts between two matches
    lk = [k for k in range(nkeys) if kind[k] != 1]
    rk = [k for k in range(nkeys) if kind[k] != 0]
    ll, rl = rng.integers(1, max_len + 1, len(lk)), rng.integers(1, max_len + 1, len(rk))
    sides = []
    for keys, lens in ((lk, ll), (rk, rl)):
        i = keys.index(9)                     # key 9 holds every special value on both sides
        lens[i] = SPECIAL.size
        vals = _values(rng, int(lens.sum()))
        vals[int(lens[:i].sum()):int(lens[:i + 1].sum())] = SPECIAL
        sides.append(Side(keys, lens, vals))
    return tuple(sides)


# ---- 2. twin vs brute force ------------------------------------------------------------------
def test_twin_equals_the_nested_loop():
    rng = np.random.default_rng(7)
    l, r = _interleaved(rng, 60, 6)
    jp = _plan(l, r)
    match = jp.match.tolist()
    assert match[0] == -1 and match[-1] == -1 and -1 in match[1:-1]
    assert any(match[i] == match[i + 1] == match[i + 2] == -1 and match[i + 3] >= 0
               for i in range(1, len(match) - 3))
    assert set(r.keys_l) - set(l.keys_l) and any(m >= 0 for m in match)
    want = _brute(l, r)
    assert jp.pairs == want.shape[1] > 0
    lens_r = dict(zip(r.keys_l, r.lens))
    cnt = [n * lens_r.get(k, 0) for k, n in zip(l.keys_l, l.lens)]
    assert jp.cnt.tolist() == cnt
    assert jp.pair_off.tolist() == [sum(cnt[:i]) for i in range(len(cnt) + 1)]
    assert jp.matched == sum(1 for c in cnt if c)
    got = _expand(jp, l, r, 0, jp.pairs)
    assert np.array_equal(got, want)
    # every special value went through, NaNs canonical, -0.0 and 0.0 apart
    seen = set(got[1].tolist()) | set(got[2].tolist())
    for v in _canon(SPECIAL.copy()).tolist():
        assert v in seen
    assert 0x7FF8000000000001 not in seen


# ---- 3. chunking -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _chunk_case():
    """pair_off hits 100,003 exactly (a 1 x 100,003 key first), followed by a run of unmatched
    left segments; later chunk borders fall inside segments."""
    rng = np.random.default_rng(11)
    lk = [0, 1, 2, 3, 4] + list(range(10, 400))
    ll = [1, 1, 2, 3, 1] + rng.integers(1, 60, 390).tolist()
    rk = [0] + list(range(10, 400, 2)) + [401]
    rl = [100_003] + rng.integers(1, 80, 195).tolist() + [4]
    l = Side(lk, ll, _values(rng, sum(ll)))
    r = Side(rk, rl, _values(rng, sum(rl)))
    jp = _plan(l, r)
    return l, r, jp, _expand(jp, l, r, 0, jp.pairs)


def test_chunked_expand_equals_one_launch():
    l, r, jp, full = _chunk_case()
    off = jp.pair_off.tolist()
    assert off[1] == off[2] == off[5] == 100_003 and jp.pairs > 250_000
    assert np.array_equal(full, _brute(l, r))
    parts = [_expand(jp, l, r, p, min(p + 100_003, jp.pairs)) for p in range(0, jp.pairs, 100_003)]
    assert len(parts) >= 3 and np.array_equal(np.concatenate(parts, axis=1), full)
    inner = next(i for i in range(5, len(off) - 1) if off[i + 1] - off[i] > 2)
    for p0, p1 in [(off[inner] + 1, off[inner] + 2),         # inside a segment, one pair
                   (off[inner] + 1, off[inner + 1] + 5),     # out of it into the next
                   (100_003, 100_003 + 4097),                # a boundary in an unmatched run
                   (100_002, 100_004), (0, 1), (jp.pairs - 1, jp.pairs), (7, 7)]:
        assert np.array_equal(_expand(jp, l, r, p0, p1), full[:, p0:p1]), (p0, p1)


def test_no_common_key_is_zero_pairs():
    rng = np.random.default_rng(3)
    l = Side([1, 3, 5], [2, 2, 2], _values(rng, 6))
    r = Side([0, 2, 4, 6], [1, 1, 1, 1], _values(rng, 4))
    jp = _plan(l, r)
    assert jp.pairs == 0 and jp.matched == 0 and jp.pair_off.tolist() == [0, 0, 0, 0]
    assert _expand(jp, l, r, 0, 0).shape == (3, 0)
    empty = Side([], [], np.zeros(0))
    for a, b in ((empty, r), (l, empty), (empty, empty)):
        assert _plan(a, b).pairs == 0


# ---- 4. 64-bit offsets -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _hot_case():
    """One key of 70,000 x 70,000 pairs (4.9e9 > 2**32) among small ones."""
    rng = np.random.default_rng(5)
    lk, ll = [1, 2, 3, 4, 5], [2, 1, 70_000, 3, 2]
    rk, rl = [1, 3, 4, 6], [3, 70_000, 2, 1]
    return (Side(lk, ll, rng.standard_normal(sum(ll))), Side(rk, rl, rng.standard_normal(sum(rl))))


def _hot_ranges(P: int):
    return [(0, 1000), (2 ** 32 - 500, 2 ** 32 + 500), (P - 1000, P)]


def _hot_expected(l: Side, r: Side, p0: int, p1: int) -> np.ndarray:
    cnt = [6, 0, 70_000 * 70_000, 6, 0]
    off = [sum(cnt[:i]) for i in range(6)]
    rj = {0: 0, 2: 1, 3: 2}
    lb, rb = _canon(l.vals), _canon(r.vals)
    rows = []
    for p in range(p0, p1):
        i = max(i for i in range(5) if off[i] <= p and cnt[i])
        q, nr = p - off[i], r.lens[rj[i]]
        rows.append((l.keys_l[i], int(lb[int(l.heads[i]) + q // nr]),
                     int(rb[int(r.heads[rj[i]]) + q % nr])))
    return np.array(rows, dtype=np.int64).T


def test_offsets_beyond_32_bits():
    l, r = _hot_case()
    jp = _plan(l, r)
    P = 6 + 70_000 * 70_000 + 6
    assert jp.pairs == P > 2 ** 32
    assert jp.pair_off.tolist() == [0, 6, 6, 6 + 70_000 ** 2, P, P]
    for p0, p1 in _hot_ranges(P):
        assert np.array_equal(_expand(jp, l, r, p0, p1), _hot_expected(l, r, p0, p1)), (p0, p1)


def test_firing_of_2_62_pairs_is_refused():
    one, zero = torch.tensor([1]), torch.tensor([0])
    with pytest.raises(OverflowError):
        K.join_plan(one, zero, 2 ** 31, one, zero, 2 ** 31, validate=False)
    keys = torch.arange(5)
    heads = torch.arange(5) * 2 ** 30
    with pytest.raises(OverflowError):  # no single key reaches it, their sum does
        K.join_plan(keys, heads, 5 * 2 ** 30, keys, heads, 5 * 2 ** 30, validate=False)
    assert K.join_plan(one, zero, 2 ** 31, one, zero, 2 ** 31 - 1, validate=False).pairs == \
        2 ** 31 * (2 ** 31 - 1)


# ---- 5. engine vs oracle ---------------------------------------------------------------------
def _stream(n: int, nkeys: int, seed: int, key_base: int = 0, hot: bool = False):
    """Per side: keys, timestamps (mostly ascending, 400 ms of disorder, every 97th element nine
    seconds old: late when it arrives, unless the step has just begun) and values, in arrival order."""
    rng = np.random.default_rng(seed)
    keys = rng.integers(0, nkeys, n)
    if hot:
        keys[rng.random(n) < 0.03] = 3
    ts = np.arange(n) * (24_000 // n + 1) + rng.integers(0, 400, n)
    ts[::97] -= 9000
    if key_base:  # sparse ids: no dense key range, the gather maps them first
        keys = (keys + 1) * key_base
    return keys, ts.astype(np.int64), _values(rng, n)


def _oracle(sides, steps: int, size: int, slide: int, bound: int):
    """Rows per window start and the number of dropped late elements, from the events alone:
    an element joins every window that contains it and has not fired when it arrives."""
    members = [{}, {}]  # side -> {(start, key): [value bits in arrival order]}
    wm, late = -(2 ** 63), 0
    n = len(sides[0][0])
    cuts = [n * i // steps for i in range(steps + 1)]
    for st in range(steps):
        seen = []
        for sd, (k, t, v) in enumerate(sides):
            sl = slice(cuts[st], cuts[st + 1])
            bits = _canon(v[sl].copy())
            for key, ts, b in zip(k[sl].tolist(), t[sl].tolist(), bits.tolist()):
                last = ts - ts % slide
                if last + size - 1 <= wm:
                    late += 1
                    continue
                s = last
                while s > ts - size:
                    if s + size - 1 > wm:
                        members[sd].setdefault((s, key), []).append(b)
                    s -= slide
            seen.append(int(t[sl].max()))
        wm = max(wm, max(seen) - bound)
    rows = {}
    for (s, key), lv in members[0].items():
        for a in lv:
            for b in members[1].get((s, key), []):
                rows.setdefault(s, Counter())[(key, a, b)] += 1
    return rows, late


def _run_engine(sides, steps: int, size: int, slide: int, bound: int, dev="cpu", chunk=1 << 24,
                restore_at=None, other=None, raw=False):
    op = KeyedJoinWindowOperator(size=size, slide=slide, device=dev, pair_chunk=chunk)
    n = len(sides[0][0])
    cuts = [n * i // steps for i in range(steps + 1)]
    fired, wm = [], -(2 ** 63)
    for st in range(steps):
        seen = []
        for sd, (k, t, v) in enumerate(sides):
            sl = slice(cuts[st], cuts[st + 1])
            assert op.process(sd, torch.from_numpy(k[sl]).to(dev), torch.from_numpy(t[sl]).to(dev),
                              torch.from_numpy(v[sl].view(np.int64).copy()).to(dev)) == []
            seen.append(int(t[sl].max()))
        if st == restore_at:
            snap = op.snapshot_state()
            if other is not None:
                with pytest.raises(ValueError):
                    KeyedJoinWindowOperator(device=dev, **other).restore_state(snap.columns, snap.meta)
            op = KeyedJoinWindowOperator(size=size, slide=slide, device=dev, pair_chunk=chunk)
            op.restore_state(snap.columns, snap.meta)
        wm = max(wm, max(seen) - bound)
        fired += op.advance_watermark(wm)
    fired += op.advance_watermark(2 ** 63 - 1)
    for s, e, k, a, b in fired:
        assert e == s + size and k.device.type == torch.device(dev).type
        assert 0 < k.numel() <= chunk
    if raw:
        return fired, op
    rows = {}
    for s, e, k, a, b in fired:
        rows.setdefault(s, Counter()).update(zip(k.tolist(), a.tolist(), b.tolist()))
    return rows, op


def _sorted_rows(fired) -> dict:
    """Per window start: the fired rows as one [3, n] array in sorted row order."""
    by = {}
    for s, _e, k, a, b in fired:
        by.setdefault(s, []).append(np.stack([k.cpu().numpy(), a.cpu().numpy(), b.cpu().numpy()]))
    out = {}
    for s, parts in by.items():
        rows = np.concatenate(parts, axis=1)
        out[s] = rows[:, np.lexsort(rows[::-1])]
    return out


@pytest.mark.parametrize("size,slide", [(4000, 4000), (6000, 2000)])
@pytest.mark.parametrize("key_base", [0, 1 << 40], ids=["ranked", "mapped"])
def test_engine_equals_oracle(size, slide, key_base):
    sides = [_stream(3000, 37, 21, key_base), _stream(3000, 41, 22, key_base)]
    want, late = _oracle(sides, 8, size, slide, 500)
    assert late > 20 and len(want) >= 4
    calls = Counter()
    gather = {}
    from mxstream.runtime.list_window_operator import KeyedListWindowOperator as LW
    for name in ("_gather_ranked", "_gather_dense", "_gather_mapped"):
        gather[name] = getattr(LW, name)
    try:
        for name, f in gather.items():
            setattr(LW, name, lambda self, *a, _f=f, _n=name: (calls.update([_n]), _f(self, *a))[1])
        got, op = _run_engine(sides, 8, size, slide, 500, chunk=1000)
    finally:
        for name, f in gather.items():
            setattr(LW, name, f)
    assert got == want
    assert op.metrics.num_late_records_dropped == late
    assert op.metrics.num_records_in == 6000 - late
    assert op.pairs_out == sum(sum(c.values()) for c in want.values())
    if key_base:
        assert calls["_gather_mapped"] and not calls["_gather_ranked"]
    else:
        assert calls["_gather_ranked"] and not calls["_gather_mapped"]


def test_window_with_one_side_only_emits_nothing_and_purges():
    op = KeyedJoinWindowOperator(size=1000, device="cpu")
    one = lambda k, t: (torch.tensor([k]), torch.tensor([t]), torch.tensor([0]))  # noqa: E731
    op.process(0, *one(1, 100))
    assert op.advance_watermark(1500) == [] and not op.arenas[0].panes
    op.process(0, *one(1, 2100))
    op.process(1, *one(2, 2200))           # another key
    op.process(1, *one(1, 100))            # late on the right
    assert op.advance_watermark(3500) == []
    assert op.metrics.num_late_records_dropped == 1 and not op.arenas[1].panes
    op.process(0, *one(1, 4100))
    op.process(1, *one(1, 4200))
    (row,) = op.advance_watermark(5000)
    assert row[:2] == (4000, 5000) and row[2].tolist() == [1]


# ---- 6. snapshot / restore ---------------------------------------------------------------------
def test_snapshot_restore_mid_window():
    sides = [_stream(2000, 19, 31), _stream(2000, 23, 32)]
    want, _ = _run_engine(sides, 8, 6000, 2000, 500)
    got, op = _run_engine(sides, 8, 6000, 2000, 500, restore_at=3,
                          other={"size": 6000, "slide": 3000})
    assert got == want and sum(op.arenas[0].panes.values()) == 0
    _run_engine(sides, 8, 6000, 2000, 500, restore_at=3, other={"size": 4000, "slide": 2000})


# ---- 12. validation ----------------------------------------------------------------------------
def test_validation_errors():
    with pytest.raises(ValueError):
        KeyedJoinWindowOperator(size=1000, device="cpu", pair_chunk=0)
    with pytest.raises(ValueError):
        KeyedJoinWindowOperator(size=1000, device="cpu").process(2, *[torch.zeros(1, dtype=torch.int64)] * 3)
    rng = np.random.default_rng(1)
    l = Side([1, 2], [2, 2], _values(rng, 4))
    r = Side([2, 3], [1, 3], _values(rng, 4))
    jp = _plan(l, r)
    good = (l.keys, l.heads, l.total, r.keys, r.heads, r.total)
    for i, bad in [(0, l.keys.to(torch.int32)), (1, l.heads.to(torch.float64)),
                   (3, torch.tensor([2, 0, 3, 0])[::2]), (4, r.heads.to(torch.int32))]:
        args = list(good)
        args[i] = bad
        with pytest.raises((TypeError, ValueError)):
            K.join_plan(*args)
    for args in [(l.keys, l.heads[:1], l.total, r.keys, r.heads, r.total),    # one start missing
                 (l.keys, l.heads, 2, r.keys, r.heads, r.total),               # a start past total
                 (l.keys.flip(0), l.heads, l.total, r.keys, r.heads, r.total),  # keys descend
                 (l.keys, l.heads, l.total, r.keys, r.heads.flip(0), r.total),
                 (l.keys, l.heads, -1, r.keys, r.heads, r.total)]:
        with pytest.raises(ValueError):
            K.join_plan(*args)
    with pytest.raises(TypeError):
        K.join_expand(jp, l.ord.to(torch.float64), r.ord, 0, jp.pairs)
    with pytest.raises(ValueError):
        K.join_expand(jp, l.ord[:2], r.ord, 0, jp.pairs)
    with pytest.raises(ValueError):
        K.join_expand(jp, torch.cat([l.ord, l.ord])[::2], r.ord, 0, jp.pairs)
    for p0, p1 in [(-1, 1), (1, 0), (0, jp.pairs + 1)]:
        with pytest.raises(ValueError):
            K.join_expand(jp, l.ord, r.ord, p0, p1)


# ---- 13. GPU: kernels equal the twin, array for array -------------------------------------------
@functools.lru_cache(maxsize=None)
def _regime_case():
    """One input for every regime of the kernels (see the test below)."""
    rng = np.random.default_rng(13)
    n = 70_000
    lk = np.arange(n, dtype=np.int64) * 2
    ll = rng.integers(1, 4, n)
    keep = np.arange(n) % 3 != 1                    # every third left key is missing on the right
    keep[0] = keep[-1] = False                      # first and last left segment unmatched
    rk_common = lk[keep]
    rl_common = rng.integers(1, 4, rk_common.size)
    # key 4 (the first matched one): 2 x 2048 = 4096 pairs, so the next segment starts exactly
    # on a tile border; then the hot key, a 1 x 5000, a 5000 x 1 and a 1000 x 1000 key
    assert keep[2] and rk_common[0] == 4
    ll[2], rl_common[0] = 2, 2048
    for key, nl, nr in [(3000, 3000, 2500), (60_000, 1, 5000), (90_000, 5000, 1),
                        (120_000, 1000, 1000)]:
        i = key // 2
        assert keep[i]
        ll[i] = nl
        rl_common[np.searchsorted(rk_common, key)] = nr
    extra = np.arange(1, 2 * n, 14, dtype=np.int64)  # right-only keys in between (odd)
    rk = np.concatenate([rk_common, extra])
    rl = np.concatenate([rl_common, rng.integers(1, 4, extra.size)])
    order = np.argsort(rk)
    rk, rl = rk[order], rl[order]
    l = Side(lk, ll, _values(rng, int(ll.sum())))
    r = Side(rk, rl, _values(rng, int(rl.sum())))
    jp = _plan(l, r)
    return l, r, jp, _expand(jp, l, r, 0, jp.pairs)


def _plan_arrays(jp):
    kl, m = jp.lkeys.numel(), jp.matched
    plan = jp.plan.cpu().view(5, kl + 1)
    return ([jp.match.cpu(), jp.cnt.cpu(), jp.pair_off.cpu(), plan[0, :m + 1]]
            + [plan[c, :m] for c in range(1, 5)])


@pytest.mark.gpu
def test_gpu_kernels_equal_the_twin(gpu_device):
    l, r, jp, want = _regime_case()
    tile = 4096
    off = jp.pair_off.tolist()
    assert jp.lkeys.numel() == 70_000 > 65_536
    assert jp.match[0] == -1 and jp.match[-1] == -1 and off[3] == tile  # a border on a tile border
    assert jp.pairs % tile and jp.pairs > 2048 * tile                   # a tail; the tile loop runs
    assert 3000 * 2500 in jp.cnt.tolist() and jp.matched < 50_000
    gl, gr = l.to(gpu_device), r.to(gpu_device)
    gp = _plan(gl, gr)
    assert (gp.pairs, gp.matched) == (jp.pairs, jp.matched)
    for a, b in zip(_plan_arrays(gp), _plan_arrays(jp)):
        assert torch.equal(a, b)
    got = _expand(gp, gl, gr, 0, gp.pairs)
    assert np.array_equal(got, want)
    parts = [K.join_expand(gp, gl.ord, gr.ord, p, min(p + 100_003, gp.pairs))
             for p in range(0, gp.pairs, 100_003)]
    for c in range(3):
        assert np.array_equal(torch.cat([p[c] for p in parts]).cpu().numpy(), want[c])
    # offsets beyond 32 bits
    hl, hr = _hot_case()
    hp = _plan(hl, hr)
    ghl, ghr = hl.to(gpu_device), hr.to(gpu_device)
    ghp = _plan(ghl, ghr)
    assert ghp.pairs == hp.pairs and torch.equal(ghp.pair_off.cpu(), hp.pair_off)
    for p0, p1 in _hot_ranges(hp.pairs):
        assert np.array_equal(_expand(ghp, ghl, ghr, p0, p1), _expand(hp, hl, hr, p0, p1)), (p0, p1)


# ---- 14. GPU operator equals CPU operator ------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("size,slide", [(4000, 4000), (6000, 2000)])
def test_gpu_operator_equals_cpu_operator(gpu_device, size, slide):
    sides = [_stream(40_000, 2000, 41, hot=True), _stream(40_000, 2500, 42, hot=True)]
    want, cpu = _run_engine(sides, 8, size, slide, 500, chunk=100_000, raw=True)
    got, gpu = _run_engine(sides, 8, size, slide, 500, dev=gpu_device, chunk=100_000, raw=True)
    want, got = _sorted_rows(want), _sorted_rows(got)
    assert sorted(got) == sorted(want) and len(want) >= 4
    for s in want:
        assert np.array_equal(got[s], want[s]), s
    assert gpu.metrics.num_late_records_dropped == cpu.metrics.num_late_records_dropped > 0
    assert gpu.pairs_out == cpu.pairs_out > 10 ** 5


# ---- 15. GPU: the scan's tile seams and its carry round ----------------------------------------
def _unit_plan(matched: np.ndarray, dev):
    """Left segments of one element each (keys 0 .. n - 1); the right side has the keys that
    `matched` marks, two elements each, and one key beyond the left side's."""
    n = matched.size
    rk = np.concatenate([np.nonzero(matched)[0], [n + 5]]).astype(np.int64)
    ar = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev)
    return K.join_plan(ar(np.arange(n)), ar(np.arange(n)), n, ar(rk), ar(np.arange(rk.size) * 2),
                       2 * rk.size)


@pytest.mark.gpu
@pytest.mark.parametrize("ends", [False, True], ids=["ends-empty", "ends-matched"])
@pytest.mark.parametrize("n", [1, 4095, 4096, 4097])
def test_gpu_scan_tile_seams_equal_the_twin(gpu_device, n, ends):
    matched = np.arange(n) % 3 == 1
    matched[0] = matched[-1] = ends
    want, got = _unit_plan(matched, "cpu"), _unit_plan(matched, gpu_device)
    m = int(matched.sum())
    assert (got.pairs, got.matched) == (want.pairs, want.matched) == (2 * m, m)
    for a, b in zip(_plan_arrays(got), _plan_arrays(want)):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_gpu_scan_carry_round_equals_the_twin(gpu_device):
    """4096 * 1024 + 1 left segments are 1025 scan tiles: the one workgroup that scans the tile
    totals takes 1024 of them per round, so the last tile's offsets come from the carry."""
    n = 4096 * 1024 + 1
    matched = np.arange(n) % 2 == 0
    want, got = _unit_plan(matched, "cpu"), _unit_plan(matched, gpu_device)
    assert (got.pairs, got.matched) == (want.pairs, want.matched) == (n + 1, (n + 1) // 2)
    for a, b in zip(_plan_arrays(got), _plan_arrays(want)):
        assert torch.equal(a, b)


# ---- 16. GPU: the expand's tile seams ------------------------------------------------------------
_SEAM_RANGES = [(0, 4097), (0, 1), (0, 2), (1, 2), (1, 3), (4095, 4096), (4095, 4097),
                (4096, 4097), (4097, 4098), (1, 4098), (4111, 8208), (4097, 8194), (0, 8208)]


@functools.lru_cache(maxsize=None)
def _seam_case():
    """A segment of exactly one expand tile (64 x 64 = 4096 pairs), then one of 1 pair, one of
    3 x 5 and another of 4096: P = 8208."""
    rng = np.random.default_rng(16)
    l = Side([0, 1, 2, 3], [64, 1, 3, 64], _values(rng, 132))
    r = Side([0, 1, 2, 3], [64, 1, 5, 64], _values(rng, 134))
    return l, r


@pytest.mark.gpu
def test_gpu_expand_tile_seams_equal_the_twin(gpu_device):
    l, r = _seam_case()
    jp = _plan(l, r)
    assert jp.pair_off.tolist() == [0, 4096, 4097, 4112, 8208]
    gl, gr = l.to(gpu_device), r.to(gpu_device)
    gp = _plan(gl, gr)
    for p0, p1 in _SEAM_RANGES:  # lengths 1, 2 and 4097, even and odd starts, whole tiles
        assert np.array_equal(_expand(gp, gl, gr, p0, p1), _expand(jp, l, r, p0, p1)), (p0, p1)
