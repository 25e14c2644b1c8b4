"""Top-N windows: the N largest keys per window, cut on the device.

One rule for every layer (docs/DESIGN.md "Top-N windows"): each fired row has a 64-bit order
word (signed raw accumulator, count, or the mapped double in Double.compare order; inverted
for `smallest`); the threshold T is the window's N-th largest word (0 when the window has
<= N rows); the candidates are all rows with word >= T -- every tie at T included -- and the
host orders them by (word descending, key ascending) and cuts to N. All comparisons are exact.

 1. the C++ twin of ``topn_select`` against numpy, candidates as sets of row indices;
 2. ``KeyedWindowOperator(top_n=...)`` against a plain per-(window, key) oracle;
 3. rejected option combinations and ``WindowTopN`` arguments;
 4. the API job natively (C++ twin) against the host operators, and the shapes the planner
    must leave alone;
 5. the gfx950 kernels against the twin, and the operator on the GPU against the CPU.
"""
from collections import Counter

import numpy as np
import pytest
import torch

from mxstream.ops import expr as E
from mxstream.ops import kernels as K
from mxstream.runtime.window_operator import KeyedWindowOperator

B = 256  # csrc/mxs_kernels.h kTopnBlock: rows of one workgroup tile of the select / compaction
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
U64 = np.uint64


# ---- the rule, in numpy -------------------------------------------------------------------------
def _order_words(vals, raw, cnt, source, smallest):
    if source == "raw":
        o = raw.view(U64) ^ U64(1 << 63)
    elif source == "count":
        o = cnt.astype(U64)
    else:
        b = vals.view(U64).copy()
        b[np.isnan(vals)] = U64(0x7FF8000000000000)
        o = np.where(b >> U64(63) != 0, ~b, b | U64(1 << 63))
    return ~o if smallest else o


def _candidates(o, bounds, n):
    """Per window, the set of row indices with order word >= the window's n-th largest."""
    out, lo = [], 0
    for hi in bounds:
        w = o[lo:hi]
        T = U64(0) if len(w) <= n else np.sort(w)[len(w) - n]
        out.append({lo + int(i) for i in np.nonzero(w >= T)[0]})
        lo = hi
    return out


# ---- kernel cases (shared by the twin test and the GPU test) ---------------------------------
def _case(name, *, raw=None, vals=None, cnt=None, bounds=None, n, source="raw", smallest=False,
          key32=False):
    rows = len(raw if raw is not None else vals)
    raw = np.zeros(rows, np.int64) if raw is None else np.asarray(raw, np.int64)
    vals = raw.astype(np.float64) if vals is None else np.asarray(vals, np.float64)
    cnt = np.ones(rows, np.int32) if cnt is None else np.asarray(cnt, np.int32)
    return dict(name=name, raw=raw, vals=vals, cnt=cnt, n=n, source=source, smallest=smallest,
                key32=key32, bounds=[rows] if bounds is None else list(bounds))


def _kernel_cases():
    rng = np.random.default_rng(11)
    cases = []
    for n0 in (1, 10):
        for rows in sorted({0, 1, n0 - 1, n0, n0 + 1, B - 1, B, B + 1, 5 * B + 3}):
            # few distinct values: ties everywhere, also at the threshold
            cases.append(_case(f"rows{rows}-N{n0}", raw=rng.integers(-40, 40, rows), n=n0))
            cases.append(_case(f"rows{rows}-N{n0}-distinct", raw=rng.permutation(rows) - 7, n=n0))
    for rows in (1, 10, B + 1, 5 * B + 3):
        for n in (rows, rows + 5):
            cases.append(_case(f"rows{rows}-N{n}-all-pass", raw=rng.integers(-9, 9, rows), n=n))
    cases.append(_case("all-equal", raw=np.full(3 * B + 5, 42), n=10))
    straddle = np.concatenate([np.arange(100, 105), np.full(20, 77), rng.integers(0, 70, 400)])
    cases.append(_case("ties-straddle-N", raw=rng.permutation(straddle), n=10))
    low = (np.int64(0x0123456789ABCD00) + rng.integers(0, 256, 2 * B + 9)).astype(np.int64)
    cases.append(_case("low-byte-only", raw=low, n=10))
    high = (rng.integers(0, 256, 2 * B + 9).astype(U64) << U64(56)).view(np.int64)
    cases.append(_case("high-byte-only", raw=high, n=10))
    # one deciding byte at each of the 8 positions
    mixed = np.array([(int(b) << (8 * p)) for p in range(8) for b in rng.integers(1, 256, 40)],
                     dtype=U64).view(np.int64)
    cases.append(_case("every-byte-decides", raw=rng.permutation(mixed), n=25))
    ext = np.array([I64_MIN, I64_MAX, -1, 0, 1, I64_MIN + 1, I64_MAX - 1, -1, 0], np.int64)
    for n in (1, 3, 5):
        cases.append(_case(f"int64-extremes-N{n}", raw=ext, n=n))
        cases.append(_case(f"int64-extremes-N{n}-smallest", raw=ext, n=n, smallest=True))
    nan2 = np.array([0x7FF8000000000001], U64).view(np.float64)[0]  # a second NaN payload
    dbl = np.array([-0.0, 0.0, np.inf, -np.inf, np.nan, nan2, 1.5, -1.5, 5e-324, -5e-324, 0.0, -0.0])
    for n in (1, 2, 3, 5, 8):
        cases.append(_case(f"doubles-N{n}", vals=dbl, n=n, source="value"))
        cases.append(_case(f"doubles-N{n}-smallest", vals=dbl, n=n, source="value", smallest=True))
    cases.append(_case("doubles-random", vals=rng.normal(size=3 * B + 1).round(1), n=10, source="value"))
    cases.append(_case("smallest", raw=rng.integers(-500, 500, 4 * B + 3), n=10, smallest=True))
    cases.append(_case("count-source", cnt=rng.integers(1, 30, 2 * B + 3), raw=np.zeros(2 * B + 3),
                       n=10, source="count"))
    cases.append(_case("three-windows-empty-middle", raw=rng.integers(0, 60, 700), n=10,
                       bounds=[300, 300, 700]))
    cases.append(_case("three-windows-small-first", raw=rng.integers(0, 60, 2 * B + 40), n=10,
                       bounds=[4, B + 4, 2 * B + 40]))
    cases.append(_case("key32-null-raw-cnt", vals=rng.integers(0, 50, 2 * B + 7).astype(np.float64) / 4,
                       n=10, source="value", key32=True, bounds=[B + 1, B + 1, 2 * B + 7]))
    return cases


KERNEL_CASES = _kernel_cases()
assert len({c["name"] for c in KERNEL_CASES}) == len(KERNEL_CASES)


def _run_select(c, device):
    """topn_select on `device`: (per-window sorted candidate row indices, bounds, columns)."""
    rows = len(c["raw"])
    dev = torch.device(device)
    # key = row index, so a candidate names its row (capacity >= 1: the columns are never null)
    cap = max(rows, 1)
    keys = torch.arange(cap, dtype=torch.int32 if c["key32"] else torch.int64)

    def col(a, dtype):
        t = torch.zeros(cap, dtype=dtype)
        t[:rows] = torch.from_numpy(np.ascontiguousarray(a))
        return t.to(dev)

    vals = col(c["vals"], torch.float64)
    raw = None if c["key32"] else col(c["raw"], torch.int64)
    cnt = None if c["key32"] else col(c["cnt"], torch.int32)
    bounds = torch.tensor(c["bounds"], dtype=torch.int32).to(dev)
    ok, ov, orw, oc, ob = K.topn_select(keys.to(dev), vals, raw, cnt, bounds, n=c["n"],
                                        source=c["source"], smallest=c["smallest"])
    ob = ob.cpu().numpy().tolist()
    ok, ov = ok.cpu().numpy().astype(np.int64), ov.cpu().numpy()
    per_win, lo = [], 0
    for hi in ob:
        idx = np.sort(ok[lo:hi])
        per_win.append(idx.tolist())
        lo = hi
    total = ob[-1] if ob else 0
    order = np.argsort(ok[:total], kind="stable") if total else np.zeros(0, np.int64)
    cols = {"keys": ok[:total][order], "vals": ov[:total].view(np.int64)[order]}
    if orw is not None:
        cols["raw"] = orw.cpu().numpy()[:total][order]
        cols["cnt"] = oc.cpu().numpy()[:total][order]
    return per_win, ob, cols


@pytest.mark.parametrize("c", KERNEL_CASES, ids=[c["name"] for c in KERNEL_CASES])
def test_twin_equals_numpy(c):
    o = _order_words(c["vals"], c["raw"], c["cnt"], c["source"], c["smallest"])
    want = _candidates(o, c["bounds"], c["n"])
    per_win, ob, cols = _run_select(c, "cpu")
    assert [set(w) for w in per_win] == want
    assert all(len(w) == len(s) for w, s in zip(per_win, want))  # no row twice
    assert ob == np.cumsum([len(s) for s in want]).tolist()
    lo = 0
    for hi, s in zip(c["bounds"], want):  # >= min(rows, N) candidates per window
        assert len(s) >= min(hi - lo, c["n"])
        lo = hi
    # every column followed its row
    idx = cols["keys"]
    assert np.array_equal(cols["vals"], c["vals"].view(np.int64)[idx])
    if not c["key32"]:
        assert np.array_equal(cols["raw"], c["raw"][idx])
        assert np.array_equal(cols["cnt"], c["cnt"][idx])


def test_twin_exact_count_without_boundary_ties():
    c = _case("distinct", raw=np.random.default_rng(3).permutation(5 * B + 3), n=10,
              bounds=[7, B + 100, 5 * B + 3])
    per_win, ob, _ = _run_select(c, "cpu")
    assert [len(w) for w in per_win] == [7, 10, 10] and ob == [7, 17, 27]


# ---- 2. the operator against a plain oracle ---------------------------------------------------
NK = 300           # keys: more rows per window than one select tile
OP_N = 10
MAP = E.compile_expr(E.var(E.VAR_RESULT) * 8.0 / 1024)


def _op_events(kind: str, panes: int = 7, pane_ms: int = 1000):
    """Every key once per pane. 'distinct': per-(window, key) aggregates differ between keys
    (a fixed permutation times 1000 dominates the per-pane noise); 'ties': four values only."""
    rng = np.random.default_rng(5)
    base = rng.permutation(NK).astype(np.int64)
    k, t, v = [], [], []
    for p in range(panes):
        keys = rng.permutation(NK).astype(np.int64)
        k.append(keys)
        t.append(p * pane_ms + np.sort(rng.integers(0, pane_ms, NK)))
        v.append(base[keys] * 1000 + (keys * 7 + p * 13) % 100 if kind == "distinct" else keys % 4)
    return np.concatenate(k), np.concatenate(t).astype(np.int64), np.concatenate(v).astype(np.int64)


def _oracle_windows(k, t, v, size, slide, what):
    """{window start: {key: value}} of the plain aggregate: 'sum' (int), 'avg' (float, v / 4
    averaged) or 'map' (sum * 8 / 1024)."""
    res = {}
    for s in range(int(t.min()) // slide * slide - size + slide, int(t.max()) + 1, slide):
        sel = (t >= s) & (t < s + size)
        if not sel.any():
            continue
        sums = np.zeros(NK, np.int64)
        np.add.at(sums, k[sel], v[sel])
        cnts = np.bincount(k[sel], minlength=NK)
        row = {}
        for key in np.nonzero(cnts)[0].tolist():
            if what == "sum":
                row[key] = int(sums[key])
            elif what == "avg":
                row[key] = float(sums[key]) / 4 / int(cnts[key])
            else:
                row[key] = float(sums[key]) * 8.0 / 1024
        res[s] = row
    return res


def _word(x, smallest=False):
    if isinstance(x, int):
        o = x + (1 << 63)
    else:
        o = int(_order_words(np.array([x], np.float64), None, None, "value", False)[0])
    return (1 << 64) - 1 - o if smallest else o


def _cut(row: dict, n: int, smallest=False):
    """Section 1 over one window's {key: value}: (candidates as a set of keys, the final rows)."""
    words = {key: _word(x, smallest) for key, x in row.items()}
    srt = sorted(words.values(), reverse=True)
    T = 0 if len(srt) <= n else srt[n - 1]
    cand = {key for key, o in words.items() if o >= T}
    final = sorted(row.items(), key=lambda kv: (-words[kv[0]], kv[0]))[:n]
    return cand, final


def _run_op(device, k, t, v, *, size, slide, what, top_n=None, pipeline=None, emit="full",
            smallest=False, steps=3):
    agg = K.AGG_AVG_F64 if what == "avg" else K.AGG_SUM_I64
    kw = {} if top_n is None else {"top_n": top_n, "top_order": "smallest" if smallest else "largest"}
    op = KeyedWindowOperator(size=size, slide=slide, agg=agg, device=device, max_keys=1024,
                             batch_capacity=4096, pipeline=pipeline, emit=emit,
                             dense_keys=emit == "key_value",
                             map_prog=MAP if what == "map" else E.EMPTY, **kw)
    dev = op.device
    vv = (v.astype(np.float64) / 4).view(np.int64) if what == "avg" else v
    fired = []
    for sl in np.array_split(np.arange(len(k)), steps):
        fired += op.process(torch.from_numpy(k[sl]).to(dev), torch.from_numpy(t[sl]).to(dev),
                            torch.from_numpy(vv[sl]).to(dev))
    fired += op.finish()
    out = {}
    for fr in fired:
        assert fr.window_start not in out and not fr.refire
        if what == "sum" and fr.raw is not None:
            vals = fr.raw.astype(np.int64).tolist()
        elif what == "sum":
            vals = [int(x) for x in fr.values.tolist()]  # key_value rows: the sum as a double
        else:
            vals = fr.values.tolist()
        assert (fr.raw is None) == (emit == "key_value")
        out[fr.window_start] = dict(zip(fr.keys.astype(np.int64).tolist(), vals))
        assert len(out[fr.window_start]) == len(fr.keys)
    return op, out


OP_SHAPES = [(2000, 2000), (3000, 1000)]   # tumbling; sliding (3 panes a window)
OP_MODES = [dict(), dict(pipeline="stream"), dict(emit="key_value"),
            dict(pipeline="stream", emit="key_value")]
_mode_id = lambda m: "-".join(f"{a}={b}" for a, b in m.items()) or "plain"  # noqa: E731


def _check_op(device, size, slide, what, mode, kind, smallest=False):
    k, t, v = _op_events(kind)
    # 2 steps over 7 panes: a step makes several sliding windows due at once (fire_many)
    op, got = _run_op(device, k, t, v, size=size, slide=slide, what=what, top_n=OP_N,
                      smallest=smallest, steps=2, **mode)
    want = _oracle_windows(k, t, v, size, slide, what)
    assert sorted(got) == sorted(want) and len(want) >= 4
    rows_in = rows_out = 0
    for s, row in want.items():
        cand, final = _cut(row, OP_N, smallest)
        assert set(got[s]) == cand, s
        assert _cut(got[s], OP_N, smallest)[1] == final, s
        if kind == "distinct":
            assert len(got[s]) == min(len(row), OP_N)
        rows_in += len(row)
        rows_out += len(cand)
    assert op.metrics.num_records_out == rows_out
    assert op.metrics.extra["topn_rows_in"] == rows_in and rows_in >= NK * len(want) > rows_out
    return got


@pytest.mark.parametrize("mode", OP_MODES, ids=_mode_id)
@pytest.mark.parametrize("what", ["sum", "avg", "map"])
@pytest.mark.parametrize("size,slide", OP_SHAPES)
def test_operator_distinct_values_equal_oracle(size, slide, what, mode):
    _check_op("cpu", size, slide, what, mode, "distinct")


@pytest.mark.parametrize("mode", OP_MODES, ids=_mode_id)
@pytest.mark.parametrize("what", ["sum", "avg", "map"])
@pytest.mark.parametrize("size,slide", OP_SHAPES)
def test_operator_boundary_ties_equal_oracle(size, slide, what, mode):
    got = _check_op("cpu", size, slide, what, mode, "ties")
    assert any(len(r) > OP_N for r in got.values())  # ties at the threshold all left the step


@pytest.mark.parametrize("size,slide", OP_SHAPES)
def test_operator_smallest(size, slide):
    _check_op("cpu", size, slide, "sum", {}, "distinct", smallest=True)
    _check_op("cpu", size, slide, "map", dict(emit="key_value"), "ties", smallest=True)


def test_operator_count_aggregate_ranks_by_count():
    rng = np.random.default_rng(2)
    k = rng.integers(0, 40, 3000).astype(np.int64)
    t = np.sort(rng.integers(0, 4000, 3000)).astype(np.int64)
    op = KeyedWindowOperator(size=2000, agg=K.AGG_COUNT, device="cpu", max_keys=256, top_n=5)
    fired = op.process(torch.from_numpy(k), torch.from_numpy(t), torch.zeros(3000, dtype=torch.int64))
    fired += op.finish()
    assert len(fired) == 2
    for fr in fired:
        sel = (t >= fr.window_start) & (t < fr.window_end)
        cnts = np.bincount(k[sel], minlength=40)
        T = np.sort(cnts)[-5]
        assert dict(zip(fr.keys.tolist(), fr.counts.tolist())) == \
            {int(i): int(c) for i, c in enumerate(cnts) if c >= T and c > 0}


@pytest.mark.parametrize("mode", OP_MODES, ids=_mode_id)
@pytest.mark.parametrize("size,slide", OP_SHAPES)
def test_operator_without_top_n_is_unchanged(size, slide, mode):
    k, t, v = _op_events("ties")
    op, got = _run_op("cpu", k, t, v, size=size, slide=slide, what="sum", steps=2, **mode)
    assert got == _oracle_windows(k, t, v, size, slide, "sum")
    assert "topn_rows_in" not in op.metrics.extra
    assert op.metrics.num_records_out == sum(len(r) for r in got.values())


# ---- 3. validation ------------------------------------------------------------------------------
@pytest.mark.parametrize("bad,word", [
    (dict(lateness=500), "lateness"), (dict(spill=True), "spill"),
    (dict(side_output_late=True), "side_output_late"),
    (dict(_vector={"dim": 4}), "vector"),
])
def test_operator_rejects_top_n_combinations(bad, word):
    with pytest.raises(ValueError, match=word):
        KeyedWindowOperator(size=1000, device="cpu", max_keys=64, top_n=3, **bad)
    KeyedWindowOperator(size=1000, device="cpu", max_keys=64, **bad)  # fine without top_n


def test_operator_rejects_top_n_on_several_ranks():
    from mxstream.parallel.comm import run_loopback

    def build(comm):
        with pytest.raises(ValueError, match="world"):
            KeyedWindowOperator(size=1000, device="cpu", max_keys=64, comm=comm, top_n=3)
        return True

    assert run_loopback(2, build) == [True, True]


@pytest.mark.parametrize("kw", [dict(top_n=0), dict(top_n=-1), dict(top_n=True), dict(top_n=2.0),
                                dict(top_n=3, top_order="biggest")])
def test_operator_rejects_bad_top_n(kw):
    with pytest.raises(ValueError, match="top_n|top_order"):
        KeyedWindowOperator(size=1000, device="cpu", max_keys=64, **kw)


def test_topn_select_validates_operands():
    keys = torch.arange(8, dtype=torch.int64)
    vals = torch.zeros(8, dtype=torch.float64)
    b = torch.tensor([8], dtype=torch.int32)
    for n in (0, -3, True, 1.5):
        with pytest.raises(ValueError, match="n must be"):
            K.topn_select(keys, vals, None, None, b, n=n)
    with pytest.raises(ValueError, match="raw"):
        K.topn_select(keys, vals, None, None, b, n=1, source="raw")
    with pytest.raises(ValueError, match="count"):
        K.topn_select(keys, vals, None, None, b, n=1, source="count")
    with pytest.raises(ValueError, match="source"):
        K.topn_select(keys, vals, None, None, b, n=1, source="best")
    with pytest.raises(TypeError):
        K.topn_select(keys, vals.float(), None, None, b, n=1)
    with pytest.raises(TypeError):
        K.topn_select(keys, vals, None, None, b.long(), n=1)
    with pytest.raises(ValueError, match="raw"):
        K.topn_select(keys, vals, torch.zeros(4, dtype=torch.int64), None, b, n=1)


@pytest.mark.parametrize("args,kw", [
    ((1, 0), {}), ((1, -2), {}), ((1, True), {}), ((1, 2.0), {}), ((-1, 3), {}), ((1.0, 3), {}),
    ((True, 3), {}), ((1, 3), dict(tie_field=-1)), ((1, 3), dict(tie_field=1)),
    ((0, 3), {}), ((1, 3), dict(tie_field="0")),
])
def test_window_topn_rejects_bad_arguments(args, kw):
    from mxstream.api.aggregations import WindowTopN

    with pytest.raises(ValueError, match="WindowTopN"):
        WindowTopN(*args, **kw)


def test_window_topn_host_rule():
    from mxstream.api.aggregations import WindowTopN
    from mxstream.api.functions import Collector

    rows = [("b", 5), ("a", 5), ("c", 9), ("d", 5), ("e", 1), ("a", 9)]
    fn = WindowTopN(1, 3)
    assert fn.native == ("topn", 1, 3, True, 0)
    assert fn.rank(rows) == [("a", 9), ("c", 9), ("a", 5)]
    assert WindowTopN(1, 2, largest=False).rank(rows) == [("e", 1), ("a", 5)]
    assert WindowTopN(1, 10).rank(rows[:2]) == [("a", 5), ("b", 5)]
    # equal value and equal tie field: arrival order
    assert WindowTopN(1, 2).rank([("a", 1, "x"), ("a", 1, "y")]) == [("a", 1, "x"), ("a", 1, "y")]
    nan = float("nan")
    dbl = [("a", 0.0), ("b", -0.0), ("c", nan), ("d", float("inf")), ("e", -1.0)]
    assert [k for k, _ in WindowTopN(1, 5).rank(dbl)] == ["c", "d", "a", "b", "e"]
    col = Collector()
    fn.process(None, None, rows, col)
    assert col.items == fn.rank(rows)


# ---- 4. the API job -----------------------------------------------------------------------------
def _lines():
    """"<ms> <host> <bytes>" lines, 11 hosts over 15 s; in [4000, 6000) h1 and h2 are made to
    tie for third place behind h0 and h3 (each host's first line there carries its total)."""
    out, seen = [], set()
    for i in range(600):
        ts, h = i * 25, f"h{(i * 7) % 11}"
        b = (i * 37) % 101 + 1
        if 4000 <= ts < 6000:
            b = 0 if h in seen else {"h0": 900, "h3": 800, "h1": 50, "h2": 50}.get(h, 1)
            seen.add(h)
        out.append(f"{ts} {h} {b}")
    return out


def _topn_job(native, *, slide=None, epilogue=False, key_late=0, all_late=0, all_size=None,
              second_consumer=False, comm=None, fn=None, wide_map=False):
    from mxstream.api import java as J
    from mxstream.api.aggregations import WindowTopN
    from mxstream.api.environment import StreamExecutionEnvironment
    from mxstream.api.time import Time, TimeCharacteristic
    from mxstream.api.tuples import Tuple2, Tuple3
    from mxstream.api.watermarks import BoundedOutOfOrdernessTimestampExtractor
    from mxstream.runtime.executor import ManualClock

    class Ext(BoundedOutOfOrdernessTimestampExtractor):
        def __init__(self):
            super().__init__(Time.milliseconds(500))

        def extractTimestamp(self, element):  # noqa: N802
            return J.parse_long(J.get(J.split(element, " "), 0))

    out = []
    env = StreamExecutionEnvironment(4, clock=ManualClock(0)).set_output(out.append)
    env.config.native = native
    env.config.device = "cpu"
    env._comm = comm
    env.set_stream_time_characteristic(TimeCharacteristic.EventTime)
    ks = (env.from_collection(_lines()).assign_timestamps_and_watermarks(Ext())
          .map(lambda s: Tuple2(J.get(J.split(s, " "), 1), J.parse_long(J.get(J.split(s, " "), 2))))
          .key_by(0))
    size = 2000
    w = ks.time_window(Time.milliseconds(size)) if slide is None else \
        ks.time_window(Time.milliseconds(size), Time.milliseconds(slide))
    if key_late:
        w = w.allowed_lateness(Time.milliseconds(key_late))
    s = w.sum(1)
    if second_consumer:
        s.map(lambda t: Tuple2("all:" + t.f0, t.f1)).print()
    if epilogue:
        s = s.map(lambda t: Tuple2(t.f0, t.f1 * 8.0 / 1024)).filter(lambda t: t.f1 > 0.25)
    if wide_map:
        s = s.map(lambda t: Tuple3(t.f0, t.f1 * 8.0 / 1024, t.f1 * 2.0))
    aw = s.time_window_all(Time.milliseconds(all_size or slide or size))
    if all_late:
        aw = aw.allowed_lateness(Time.milliseconds(all_late))
    aw.process(fn or WindowTopN(1, 3)).print()
    graph = env.get_stream_graph()
    env.execute("topn")
    topn_nodes = [t for t in graph if (getattr(t, "meta", None) or {}).get("kind") == "window"
                  and t.meta["stream"].keyed is None]
    keyed_nodes = [t for t in graph if (getattr(t, "meta", None) or {}).get("kind") == "window"
                   and t.meta["stream"].keyed is not None]
    assert len(topn_nodes) == 1 and len(keyed_nodes) == 1
    lowered = bool(topn_nodes[0].meta.get("fused"))
    assert lowered == ("top_n" in keyed_nodes[0].meta)
    return out, lowered


@pytest.fixture
def engine_top_n(monkeypatch):
    """The top_n each engine operator was built with (None: a plain operator)."""
    built = []
    init = KeyedWindowOperator.__init__

    def spy(self, *a, **kw):
        init(self, *a, **kw)
        built.append(kw.get("top_n"))

    monkeypatch.setattr(KeyedWindowOperator, "__init__", spy)
    return built


@pytest.mark.parametrize("epilogue", [False, True], ids=["sum", "sum-map-filter"])
@pytest.mark.parametrize("slide", [None, 1000, 500], ids=["tumbling", "slide1000", "slide500"])
def test_api_job_native_equals_host(slide, epilogue, engine_top_n):
    host, lowered = _topn_job("off", slide=slide, epilogue=epilogue)
    assert not lowered and not engine_top_n
    got, lowered = _topn_job("auto", slide=slide, epilogue=epilogue)
    assert lowered and engine_top_n and all(n == 3 for n in engine_top_n)
    assert got == host  # same lines, same order
    nwin = len({ts // (slide or 2000) for ts in range(0, 15000, 25)}) + (2000 // (slide or 2000) - 1)
    assert len(host) == 3 * nwin and all(ln.startswith("1> (h") for ln in host)


def test_api_job_tie_for_third_place_settled_by_key():
    host, _ = _topn_job("off")
    got, lowered = _topn_job("auto")
    assert lowered and got == host
    # window [4000, 6000): h0, h3, then h1 == h2 tie -> the smaller key
    sums = Counter()
    for ln in _lines():
        ts, h, b = ln.split()
        if 4000 <= int(ts) < 6000:
            sums[h] += int(b)
    assert sums["h1"] == sums["h2"] < sums["h3"] < sums["h0"]
    want = [f"1> ({h},{sums[h]})" for h in ("h0", "h3", "h1")]
    assert got[6:9] == want


def test_api_job_smallest_and_other_fields():
    from mxstream.api.aggregations import WindowTopN

    fn = WindowTopN(1, 4, largest=False)
    host, _ = _topn_job("off", fn=fn)
    got, lowered = _topn_job("auto", fn=WindowTopN(1, 4, largest=False))
    assert lowered and got == host and len(host) == 4 * 8


@pytest.mark.parametrize("kw", [
    dict(key_late=1000), dict(all_late=1000), dict(all_size=4000), dict(slide=1000, all_size=2000),
    dict(second_consumer=True),
], ids=["keyed-lateness", "all-lateness", "all-size-2x", "all-size-not-slide", "second-consumer"])
def test_api_job_not_lowered_still_correct(kw, engine_top_n):
    host, _ = _topn_job("off", **kw)
    got, lowered = _topn_job("auto", **kw)
    assert not lowered and not any(engine_top_n)
    assert Counter(got) == Counter(host) and len(host) >= 12
    top = lambda lines: [ln for ln in lines if "all:" not in ln]  # noqa: E731
    assert top(got) == top(host)


def test_api_job_field_mismatch_not_lowered(engine_top_n):
    from mxstream.api.aggregations import WindowTopN

    # a map the fire kernel cannot take (two computed columns) stays between the windows; the
    # ranked field is then not the operator's order word
    host, _ = _topn_job("off", fn=WindowTopN(2, 3), wide_map=True)
    got, lowered = _topn_job("auto", fn=WindowTopN(2, 3), wide_map=True)
    assert not lowered and not any(engine_top_n) and got == host and len(host) == 24


def test_api_job_two_loopback_ranks_not_lowered(engine_top_n):
    from mxstream.parallel.comm import run_loopback

    host, _ = _topn_job("off")

    def rank_job(comm):
        return _topn_job("auto", comm=comm)

    res = run_loopback(2, rank_job)
    assert not any(lowered for _, lowered in res) and not any(engine_top_n)
    assert [ln for out, _ in res for ln in out] == host  # the all-window runs on rank 0


def test_bench_config10_device_cut_equals_host_cut():
    """bench_configs --config 10: both variants name the same winners; with the cut only the
    candidates cross to the host (N rows a firing: random sums do not tie at this size)."""
    from mxstream.models.bench_configs import config10

    kw = dict(steps=26, warmup=1, batch=1 << 14, keys=2000, device="cpu")
    full, cut = config10(**kw), config10(top_n=10, **kw)
    assert full["firings_measured"] == cut["firings_measured"] >= 2
    assert full["top_checksum"] == cut["top_checksum"] != 0
    assert full["d2h_rows_per_firing"] > 1000 and cut["d2h_rows_per_firing"] == 10
    assert cut["d2h_bytes_per_firing"] == 280 and cut["value"] > 0 and full["value"] > 0


# ---- 5. GPU -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def twin_results():
    return {c["name"]: _run_select(c, "cpu") for c in KERNEL_CASES}


@pytest.mark.gpu
@pytest.mark.parametrize("c", KERNEL_CASES, ids=[c["name"] for c in KERNEL_CASES])
def test_gpu_kernel_equals_twin(c, gpu_device, twin_results):
    per_win, ob, cols = _run_select(c, gpu_device)
    t_win, t_ob, t_cols = twin_results[c["name"]]
    assert ob == t_ob and per_win == t_win
    assert sorted(cols) == sorted(t_cols)
    for name in cols:
        assert np.array_equal(cols[name], t_cols[name]), name


@pytest.mark.gpu
@pytest.mark.parametrize("source,smallest", [("raw", False), ("value", True)])
def test_gpu_kernel_grid_stride_70k_rows(gpu_device, source, smallest):
    rng = np.random.default_rng(17)
    rows = 70_000
    c = _case("70k", raw=rng.integers(-(1 << 40), 1 << 40, rows),
              vals=rng.normal(size=rows) * 1e6, n=10, source=source, smallest=smallest,
              bounds=[30_011, 30_500, rows])
    c["raw"][rng.integers(0, rows, 2000)] = (1 << 40) + 5   # a tie that straddles the threshold
    c["vals"][rng.integers(0, rows, 2000)] = -1e9 if smallest else 1e9
    g = _run_select(c, gpu_device)
    t = _run_select(c, "cpu")
    assert g[1] == t[1] and g[0] == t[0] and g[1][-1] > 30
    for name in t[2]:
        assert np.array_equal(g[2][name], t[2][name]), name


@pytest.mark.gpu
@pytest.mark.parametrize("mode", OP_MODES, ids=_mode_id)
@pytest.mark.parametrize("what,kind", [("sum", "distinct"), ("avg", "ties"), ("map", "ties")])
@pytest.mark.parametrize("size,slide", OP_SHAPES)
def test_gpu_operator_equals_cpu(gpu_device, size, slide, what, kind, mode):
    k, t, v = _op_events(kind)
    g_op, g = _run_op(gpu_device, k, t, v, size=size, slide=slide, what=what, top_n=OP_N, steps=2,
                      **mode)
    c_op, c = _run_op("cpu", k, t, v, size=size, slide=slide, what=what, top_n=OP_N, steps=2,
                      **mode)
    assert sorted(g) == sorted(c) and len(c) >= 4
    for s in c:  # row for row after the host ordering (candidates, then the cut)
        assert sorted(g[s].items()) == sorted(c[s].items()), s
        assert _cut(g[s], OP_N)[1] == _cut(c[s], OP_N)[1]
    assert g_op.metrics.num_records_out == c_op.metrics.num_records_out
    assert g_op.metrics.extra["topn_rows_in"] == c_op.metrics.extra["topn_rows_in"]
