"""Planner: rewrites recognised keyed-window shapes onto native operators.

A window transformation runs natively (runtime/native_ops.py -> C++ twin or gfx950 kernels)
when all of the following are provable at plan time; otherwise the exact host WindowOperator
runs:
  * assigner: tumbling/sliding, event or processing time, default trigger, no evictor;
  * key: keyBy(<int field>);
  * function: ``sum/min/max(pos)``, a builtin aggregate (api/aggregations.py), a ``process``
    function with a ``native`` descriptor (the median, ``WindowQuantiles``,
    ``WindowDistinctCount``), or a reduce
    lambda whose trace is "field pos = a.pos + b.pos, every other field = a's" (Flink's
    ``reduce((a, b) -> new TupleN(a.f0, .., a.fk + b.fk, ..))``, BandwidthMonitor.java:37);
  * keep-first fields other than the key are dead: the only consumer is a map whose traced
    output reads just the key and the aggregate (BandwidthMonitorWithEventTime.java:48-53),
    or the tuple has no such fields.

A window join (api/joins.py) whose function is a projection -- a tuple of the key and one value
field of each side -- over tumbling / sliding event-time windows with both keys given as field
positions is lowered onto NativeJoinOp (``_lower_join``); any other join, and every co-group,
keeps the host plan (tagged union -> keyed window -> co-group function). An interval join with
positional keys and such a projection is lowered onto NativeIntervalJoinOp
(``_lower_interval_join``); any other keeps the tagged union -> keyed IntervalJoinOp.
``a.connect(b).key_by(p, q).process(LookupLatest(..))`` with positional keys is lowered onto
NativeLookupOp (``_lower_connect``); every other connected function keeps the host operators.
``a.key_by(p).connect(b.broadcast(..)).process(RuleSetAlert(..))`` is lowered onto
NativeRuleSetOp (``_lower_broadcast_connect``); every other broadcast function keeps
BroadcastProcessOp.
``key_by(p).process(CountWithTimeout(..))`` is lowered onto NativeTimeoutOp and
``key_by(p).process(SustainedAlert(..))`` onto NativeSustainOp and
``key_by(p).process(BurstAlert(..))`` with ``times <= 16`` onto NativeBurstOp and
``key_by(p).process(StateMachineAlert(..))`` with at most 16 states onto NativeStateMachineOp
and ``key_by(p).process(CounterRate(..))`` onto NativeCounterRateOp
(``_lower_keyed_process``), each of the last four also under ``EventTimeOrdered(..)``, with the
device reorder buffer in front; every other keyed process function keeps KeyedProcessOp.

A ``window_all(..).process(WindowTopN(..))`` right behind such a window is folded into it
(``_lower_topn``): the keyed operator cuts each firing to its top-N candidates on the device.
"""
from __future__ import annotations

import math

from ..ops import expr as E
from ..runtime.executor import Transformation
from . import windowing as W


class _Probe:
    """Records which tuple fields a traced function touches."""

    def __init__(self, arity: int):
        self.used: set[int] = set()
        self.arity = arity

    def row(self):
        probe = self

        class Row(tuple):
            def __getitem__(self, i):
                probe.used.add(int(i))
                return E.var(int(i))

            def __getattr__(self, name):
                if name.startswith("f") and name[1:].isdigit():
                    return self[int(name[1:])]
                raise AttributeError(name)

        return Row([None] * self.arity)


def trace_fieldwise_reduce(fn, arity: int) -> int | None:
    """Return the summed field index if `fn(a, b)` is a field-wise sum of one field keeping
    a's other fields, else None."""
    from .functions import ReduceFunction

    call = fn.reduce if isinstance(fn, ReduceFunction) else fn

    class Row(tuple):
        def __getattr__(self, name):
            if name.startswith("f") and name[1:].isdigit():
                return self[int(name[1:])]
            raise AttributeError(name)

    a = Row([E.var(100 + i) for i in range(arity)])
    b = Row([E.var(200 + i) for i in range(arity)])
    try:
        out = call(a, b)
    except Exception:
        return None
    if not isinstance(out, tuple) or len(out) != arity:
        return None
    summed = None
    for i, f in enumerate(out):
        if not isinstance(f, E.Expr):
            return None
        if f.op == "var" and f.value == 100 + i:
            continue
        if f.op == "+" and {a_.value for a_ in f.args if a_.op == "var"} == {100 + i, 200 + i} \
                and all(a_.op == "var" for a_ in f.args):
            if summed is not None:
                return None
            summed = i
            continue
        return None
    return summed


def trace_avg_aggregate(fn, arity: int) -> int | None:
    """Recognise a user AggregateFunction computing the average of one numeric field with a
    (count, sum) accumulator (ComputeCpuAvg.java:31-58): `add` traced symbolically must be
    "count + 1, sum + value.f<p>" (in either accumulator order), and `get_result` / `merge`
    checked on concrete accumulators (get_result branches on count == 0, which no trace
    expresses). Returns p, or None."""
    from .functions import AggregateFunction

    if not isinstance(fn, AggregateFunction):
        return None
    try:
        acc0 = fn.create_accumulator()
        if not isinstance(acc0, tuple) or len(acc0) != 2 or any(x != 0 for x in acc0):
            return None

        class Row(tuple):
            def __getattr__(self, name):
                if name.startswith("f") and name[1:].isdigit():
                    return self[int(name[1:])]
                raise AttributeError(name)

        out = fn.add(Row([E.var(i) for i in range(arity)]), Row([E.var(100), E.var(101)]))
        if not isinstance(out, tuple) or len(out) != 2:
            return None
        cnt_i = sum_i = field = None
        for i, f in enumerate(out):
            if not isinstance(f, E.Expr) or f.op != "+" or len(f.args) != 2:
                return None
            a, b = f.args
            names = {x.value for x in (a, b) if x.op == "var"}
            consts = [x.value for x in (a, b) if x.op == "const"]
            if names == {100 + i} and consts == [1.0]:
                cnt_i = i
            elif len(names) == 2 and 100 + i in names and all(x.op == "var" for x in (a, b)):
                sum_i, field = i, (names - {100 + i}).pop()
            else:
                return None
        if cnt_i is None or sum_i is None or not 0 <= field < arity:
            return None
        T = type(acc0)

        def mk(c, sm):
            v = [0, 0]
            v[cnt_i], v[sum_i] = c, sm
            return T(v)
        for c, sm in ((0, 0.0), (3, 6.0), (7, 10.5), (2, -3.0), (5, 1e300)):
            want = 0.0 if c == 0 else sm / c
            if fn.get_result(mk(c, sm)) != want:
                return None
        m = fn.merge(mk(2, 1.5), mk(3, 4.0))
        if tuple(m) != tuple(mk(5, 5.5)):
            return None
        return field
    except Exception:
        return None


def _consumers(sinks):
    from ..runtime.executor import Executor

    nodes = Executor._topo(sinks)
    ch = {n.id: [] for n in nodes}
    for n in nodes:
        for p in n.parents:
            ch[p.id].append(n)
    return nodes, ch


def _dead_fields_ok(t: Transformation, children, key_pos: int, val_pos: int, arity: int) -> bool:
    keep = set(range(arity)) - {key_pos, val_pos}
    if not keep:
        return True
    kids = children.get(t.id, [])
    if len(kids) != 1:
        return False
    c = kids[0]
    meta = getattr(c, "meta", None) or {}
    if meta.get("kind") != "map":
        return False
    probe = _Probe(arity)
    try:
        from .functions import MapFunction

        fn = meta["fn"]
        (fn.map if isinstance(fn, MapFunction) else fn)(probe.row())
    except Exception:
        return False
    return not (probe.used & keep)


def _defer_safe(env, nodes) -> bool:
    """A pass's delay of the device ingest's output changes nothing the job can observe: no
    checkpoints (a deferred batch would sit between two passes), and every operator is a
    map / filter / timestamp assigner / rolling aggregate / event-time window / sink -- none
    reads the processing-time clock."""
    if env.checkpoint_config.is_checkpointing_enabled():
        return False
    for n in nodes:
        if n.kind in ("source", "sink", "union", "side"):
            continue
        meta = getattr(n, "meta", None) or {}
        kind = meta.get("kind")
        if kind in ("map", "filter", "timestamps", "rolling"):
            continue
        if kind == "window" and meta["stream"].assigner.is_event_time():
            continue
        return False
    return True


def _lower_text(env, sinks) -> None:
    """Columnar text ingest: source(text) -> [timestamps] -> map(parse) -> [filter] becomes one
    TextParseOp fed by raw line batches, when the map (and extractor / filter) trace
    (api/textplan.py). The filter node stays in the graph as a pass-through."""
    from ..runtime.columnar import PassThroughOp, TextParseOp
    from . import textplan as T

    nodes, children = _consumers(sinks)
    defer = _defer_safe(env, nodes) and getattr(env.config, "ingest_defer", True)
    for t in nodes:
        meta = getattr(t, "meta", None) or {}
        if meta.get("kind") != "map" or meta.get("columnar") or len(t.parents) != 1:
            continue
        parent, ts_node = t.parents[0], None
        pmeta = getattr(parent, "meta", None) or {}
        if pmeta.get("kind") == "timestamps" and len(parent.parents) == 1:
            ts_node, parent = parent, parent.parents[0]
            pmeta = getattr(parent, "meta", None) or {}
        if parent.kind != "source" or not pmeta.get("text"):
            continue
        if len(children[parent.id]) != 1 or (ts_node is not None and len(children[ts_node.id]) != 1):
            continue
        try:
            spec = T.trace_text_map(meta["fn"])
            ts_spec, bound = None, 0
            if ts_node is not None:
                a = ts_node.meta["assigner"]
                ts_spec = T.trace_extractor(a)
                bound = a.get_max_out_of_orderness_in_millis()
        except T.TraceError:
            continue
        filt, fnode = None, None
        kids = children[t.id]
        if len(kids) == 1 and (getattr(kids[0], "meta", None) or {}).get("kind") == "filter" \
                and (kids[0].parallelism or env.parallelism) == (t.parallelism or env.parallelism):
            try:
                filt = T.trace_tuple_filter(kids[0].meta["fn"], tuple(k for _, k in spec.fields))
                fnode = kids[0]
            except T.TraceError:
                filt = None
        mode = getattr(env.config, "text_ingest", "auto")
        dev = str(env.config.device)
        ingest_dev = dev if (mode == "device" or (mode == "auto" and dev.startswith("cuda"))) \
            else None
        # The device ingest's dictionary is shared with the keyed native operators downstream
        # (names of fired keys, Java hashes of key groups at G > 1).
        shared: dict = {}
        t.factory = (lambda spec=spec, ts_spec=ts_spec, bound=bound, filt=filt, d=ingest_dev,
                     sh=shared, df=defer: TextParseOp(spec, ts_spec=ts_spec, bound=bound,
                                                      filter_prog=filt, device=d, shared=sh,
                                                      defer=df))
        t.parents = [parent]
        if fnode is not None:
            fnode.factory = PassThroughOp
            fnode.meta = dict(fnode.meta, fused=True)
        src_factory = parent.factory

        def columnar_source(f=src_factory, ring=ingest_dev is not None, dev=ingest_dev):
            s = f()
            s.columnar = True
            if ring and hasattr(type(s), "ring"):
                s.ring = True  # file -> pinned ring slots (C++ reader) -> device ingest
                s.ring_device = dev
            return s

        parent.factory = columnar_source
        t.meta = dict(meta, columnar=True, text_spec=spec,
                      device_ingest=shared if ingest_dev is not None else None,
                      event_ts=ts_spec is not None)


def plan(env, sinks):
    if env.config.native == "off":
        return sinks
    _lower_text(env, sinks)
    nodes, children = _consumers(sinks)
    for t in nodes:
        meta = getattr(t, "meta", None) or {}
        if meta.get("kind") == "rolling" and meta["agg"] in ("sum", "min", "max") \
                and meta["key_pos"] is not None:
            _install_native_rolling(env, t, meta)
            continue
        if meta.get("kind") == "rolling" and meta["agg"] in ("maxBy", "minBy") \
                and meta["key_pos"] is not None:
            # (a key selector that is not a position keeps the host RollingReduceOp)
            _install_native_rolling_by(env, t, meta)
            continue
        if meta.get("kind") == "join":
            _lower_join(env, t, meta)
            continue
        if meta.get("kind") == "interval_join":
            _lower_interval_join(env, t, meta)
            continue
        if meta.get("kind") == "connect":
            _lower_connect(env, t, meta)
            continue
        if meta.get("kind") == "broadcast_connect":
            _lower_broadcast_connect(env, t, meta)
            continue
        if meta.get("kind") == "keyed_process":
            _lower_keyed_process(env, t, meta)
            continue
        if meta.get("kind") != "window":
            continue
        ws = meta["stream"]
        spec = meta["spec"]
        a = ws.assigner
        if type(a) is W.GlobalWindows:
            _lower_count_window(env, t, ws, spec, meta, children)
            continue
        session = type(a) is W.EventTimeSessionWindows
        if session and ws._late_tag is not None:
            continue  # late side output of merging windows: host operator
        if not session and not isinstance(a, (W.TumblingEventTimeWindows,
                                              W.SlidingEventTimeWindows)):
            continue
        if ws._trigger is not None or ws._evictor is not None or ws.keyed is None:
            continue
        key_pos = ws.keyed.key_pos
        if key_pos is None:
            continue
        kind = val_pos = None
        ok_arities: set[int] = set()
        if meta.get("native_hint") and meta["native_hint"][0] in ("sum", "min", "max"):
            kind, val_pos = meta["native_hint"]
            result = "tuple"
            ok_arities = {ar for ar in range(2, 9) if ar > max(key_pos, val_pos)
                          and _dead_fields_ok(t, children, key_pos, val_pos, ar)}
        elif spec.kind == "aggregate" and spec.window_fn is None and hasattr(spec.fn, "native"):
            kind, val_pos = spec.fn.native
            result = "value"
            ok_arities = set(range(max(key_pos, val_pos) + 1, 64))
        elif spec.kind == "aggregate" and spec.window_fn is None and not session:
            # A user AggregateFunction: the (count, sum) average of one field?
            for ar in range(2, 9):
                if ar <= key_pos:
                    continue
                p = trace_avg_aggregate(spec.fn, ar)
                if p is not None and p != key_pos:
                    kind, val_pos, result = "avg", p, "value"
                    ok_arities.add(ar)
        elif spec.kind == "process" and getattr(spec.fn, "native", (None,))[0] == "median" \
                and not session:
            kind, val_pos = "median", spec.fn.native[1]
            result = "value"
            ok_arities = set(range(max(key_pos, val_pos) + 1, 64))
        elif spec.kind == "process" and getattr(spec.fn, "native", (None,))[0] == "quantiles" \
                and not session and a.is_event_time():
            # WindowQuantiles(field, qs) over tumbling / sliding event-time windows: (key,
            # x_1..x_Q) rows from the median's pane arena; anything else: host operator
            kind, val_pos = "quantiles", spec.fn.native[1]
            result = "tuple"  # NativeMedianOp builds the (key, x_1..x_Q) rows itself
            ok_arities = set(range(max(key_pos, val_pos) + 1, 64))
        elif spec.kind == "process" and getattr(spec.fn, "native", (None,))[0] == "distinct" \
                and not session and a.is_event_time():
            # WindowDistinctCount(field), the same windows as the quantiles: (key, count) rows
            # from a hash set over the median's pane arena; anything else: host operator
            kind, val_pos = "distinct", spec.fn.native[1]
            result = "tuple"  # NativeMedianOp builds the (key, count) rows itself
            ok_arities = set(range(max(key_pos, val_pos) + 1, 64))
        elif spec.kind == "reduce" and spec.window_fn is None:
            result = "tuple"
            for ar in range(2, 9):
                p = trace_fieldwise_reduce(spec.fn, ar)
                if p is None or p == key_pos or ar <= key_pos:
                    continue
                if val_pos is not None and p != val_pos:
                    continue
                if _dead_fields_ok(t, children, key_pos, p, ar):
                    kind, val_pos = "sum", p
                    ok_arities.add(ar)
        if kind is None or not ok_arities:
            continue
        _install_native(env, t, ws, spec, key_pos, val_pos, kind, result, ok_arities,
                        session=session)
        if not session and kind in ("sum", "min", "max") and result == "tuple":
            _fuse_window_epilogue(env, t, children, key_pos, val_pos, ok_arities)
        if not session and t.meta.get("native") and kind in ("sum", "min", "max", "count", "avg"):
            t.meta = dict(t.meta, reduce_kind=kind, key_pos=key_pos, val_pos=val_pos,
                          scalar=result == "value")
    _lower_topn(env, nodes, children)
    return sinks


def _lower_topn(env, nodes, children) -> None:
    """keyed window (native sum / min / max / count / avg, epilogue fused or not) ->
    ``window_all(tumbling).process(WindowTopN)``: when every all-window holds exactly one firing
    of the keyed window, the keyed operator cuts each firing to its top-N candidates on the
    device (KeyedWindowOperator top_n), ranks them with the function and emits what the
    all-window operator would have; that node becomes a pass-through. Anything else -- lateness
    or a late tag on either window, another trigger / evictor / assigner, a size that is not the
    keyed window's slide, a second consumer, more than one rank -- keeps the host operators."""
    from ..runtime.columnar import PassThroughOp

    comm = getattr(env, "_comm", None)
    if (comm.world if comm is not None else getattr(env, "world", 1)) > 1:
        return
    for t in nodes:
        meta = getattr(t, "meta", None) or {}
        if meta.get("kind") != "window" or meta.get("fused"):
            continue
        ws, spec = meta["stream"], meta["spec"]
        fn = spec.fn
        if ws.keyed is not None or type(ws.assigner) is not W.TumblingEventTimeWindows \
                or ws._trigger is not None or ws._evictor is not None or ws._lateness \
                or ws._late_tag is not None or spec.kind != "process" \
                or getattr(fn, "native", (None,))[0] != "topn" or len(t.parents) != 1:
            continue
        # up through the map / filter nodes the keyed window fused into its fire kernel
        p = t.parents[0]
        while True:
            pm = getattr(p, "meta", None) or {}
            if pm.get("fused") and pm.get("kind") in ("map", "filter") and len(p.parents) == 1 \
                    and len(children[p.id]) == 1:
                p = p.parents[0]
                continue
            break
        if pm.get("kind") != "window" or not pm.get("native") or "reduce_kind" not in pm \
                or len(children[p.id]) != 1 or pm.get("scalar") or pm.get("fused_scalar"):
            continue
        pws = pm["stream"]
        pa, a = pws.assigner, ws.assigner
        if not isinstance(pa, (W.TumblingEventTimeWindows, W.SlidingEventTimeWindows)) \
                or pws._lateness or pws._late_tag is not None:
            continue
        # one upstream firing per all-window: its rows carry window_end - 1
        if a.size != pa.slide or (pa.offset + pa.size - a.offset) % a.size:
            continue
        layout = pm.get("fused_layout")
        if layout is None:
            ok = fn.field == pm["val_pos"] and fn.tie_field == pm["key_pos"]
        else:
            want = -1 if pm.get("fused_map") else pm["val_pos"]
            ok = (max(fn.field, fn.tie_field) < len(layout) and layout[fn.field] == want
                  and layout[fn.tie_field] == pm["key_pos"] and pm["key_pos"] != pm["val_pos"])
        if not ok:
            continue
        inner, tail = p.factory, t.factory

        def factory(inner=inner, fn=fn, tail=tail):
            op = inner()
            op.top_fn, op.top_tail_factory = fn, tail
            return op

        p.factory = factory
        p.meta = dict(pm, top_n=fn.n)
        t.factory = PassThroughOp
        t.meta = dict(meta, fused=True)


def _count_window_size(ws) -> int | None:
    """n of a tumbling count window: GlobalWindows + PurgingTrigger(CountTrigger(n)), no evictor
    (KeyedStream.countWindow(n)); None for anything else (sliding count windows use an evictor)."""
    tr = ws._trigger
    if ws._evictor is not None or not isinstance(tr, W.PurgingTrigger):
        return None
    inner = tr.nested
    if type(inner) is not W.CountTrigger or not isinstance(inner.count, int) or inner.count < 1:
        return None
    return inner.count


SLIDE_MAX_PANES = 64  # csrc kSlideMaxPanes: panes of gcd(size, slide) elements per window


def _count_window_slide(ws) -> tuple[int, int] | None:
    """(size, slide) of a sliding count window: GlobalWindows + CountEvictor.of(size) (evicting
    before the function) + a bare CountTrigger(slide) (KeyedStream.countWindow(size, slide)), with
    at most SLIDE_MAX_PANES panes per window; None for anything else."""
    ev, tr = ws._evictor, ws._trigger
    if type(ev) is not W.CountEvictor or ev.after or type(tr) is not W.CountTrigger:
        return None
    size, slide = ev.max_count, tr.count
    for x in (size, slide):
        if not isinstance(x, int) or isinstance(x, bool) or not 1 <= x < (1 << 31):
            return None
    if size // math.gcd(size, slide) > SLIDE_MAX_PANES:
        return None
    return size, slide


def _lower_count_window(env, t, ws, spec, meta, children) -> None:
    """keyBy(k).countWindow(n).sum/min/max(p) | reduce(field-wise sum) | aggregate(avg) ->
    NativeCountWindowOp (segmented-scan count windows on the GPU / C++ twin); countWindow(size,
    slide) with the same functions -> the same operator in its sliding mode.

    countWindow(n).maxBy/minBy(p) (tumbling only) -> NativeCountWindowByOp: the arg-select scan
    names each window's winner and the whole winner record is emitted, so every arity above the
    key and value positions is accepted and no dead-field condition applies. These keep the host
    operators: countWindow(size, slide) with maxBy / minBy (the pane ring would need a row per
    pane), time and session windows with maxBy / minBy (pane state would need the payload row;
    plan() never lowers their hint), key selectors that are not a position, and a late tag."""
    n, slide = _count_window_size(ws), 0
    hint = meta.get("native_hint")
    if hint and hint[0] in ("maxBy", "minBy"):
        if n is None or ws.keyed is None or ws.keyed.key_pos is None \
                or ws._late_tag is not None:
            return
        from ..runtime.native_ops import NativeCountWindowByOp

        by_kind, by_pos = hint
        by_key_pos, by_key_fn = ws.keyed.key_pos, ws.keyed.key_fn
        if by_pos < 0 or by_pos == by_key_pos:
            return
        by_fallback, by_device = t.factory, env.config.device

        def by_factory():
            return NativeCountWindowByOp(count=n, key_fn=by_key_fn, key_pos=by_key_pos,
                                         val_pos=by_pos, kind=by_kind, device=by_device,
                                         fallback_factory=by_fallback)

        t.factory = by_factory
        t.meta = dict(t.meta, native=True)
        return
    if n is None:
        shape = _count_window_slide(ws)
        if shape is not None:
            n, slide = shape
    if n is None or ws.keyed is None or ws.keyed.key_pos is None or ws._late_tag is not None:
        return
    key_pos = ws.keyed.key_pos
    kind = val_pos = None
    ok: set[int] = set()
    result = "tuple"
    if meta.get("native_hint") and meta["native_hint"][0] in ("sum", "min", "max"):
        kind, val_pos = meta["native_hint"]
        ok = {ar for ar in range(2, 9) if ar > max(key_pos, val_pos)
              and _dead_fields_ok(t, children, key_pos, val_pos, ar)}
    elif spec.kind == "aggregate" and spec.window_fn is None and hasattr(spec.fn, "native"):
        kind, val_pos = spec.fn.native
        result = "value"
        ok = set(range(max(key_pos, val_pos) + 1, 64))
    elif spec.kind == "aggregate" and spec.window_fn is None:
        for ar in range(2, 9):
            if ar <= key_pos:
                continue
            p = trace_avg_aggregate(spec.fn, ar)
            if p is not None and p != key_pos:
                kind, val_pos, result = "avg", p, "value"
                ok.add(ar)
    elif spec.kind == "reduce" and spec.window_fn is None:
        for ar in range(2, 9):
            p = trace_fieldwise_reduce(spec.fn, ar)
            if p is None or p == key_pos or ar <= key_pos:
                continue
            if val_pos is not None and p != val_pos:
                continue
            if _dead_fields_ok(t, children, key_pos, p, ar):
                kind, val_pos = "sum", p
                ok.add(ar)
    if kind not in ("sum", "min", "max", "count", "avg") or not ok:
        return
    from ..runtime.native_ops import NativeCountWindowOp
    from .tuples import Tuple

    if result == "value":
        def builder(template, res, key):
            return res
    else:
        def builder(template, res, key, vp=val_pos):
            row = list(template)
            row[vp] = res
            return Tuple(row)

    fallback = t.factory
    device = env.config.device
    key_fn = ws.keyed.key_fn

    def factory():
        return NativeCountWindowOp(count=n, slide=slide, result_builder=builder, ok_arities=ok,
                                   key_fn=key_fn, key_pos=key_pos, val_pos=val_pos, kind=kind,
                                   device=device, fallback_factory=fallback)

    t.factory = factory
    t.meta = dict(t.meta, native=True)


def _expr_vars(e) -> set:
    if e.op == "var":
        return {e.value}
    return set().union(*(_expr_vars(a) for a in e.args)) if e.args else set()


def _fuse_window_epilogue(env, t, children, key_pos: int, val_pos: int, ok_arities) -> None:
    """window(reduce/sum/min/max) -> map -> [filter] (BandwidthMonitorWithEventTime.java:46-55):
    the map and filter are traced over the window's output tuple (the aggregate as
    VAR_RESULT, other fields passed through by name) and run inside the fire kernel's epilogue;
    only the rows that pass leave the device. The map / filter nodes become pass-throughs."""
    from ..runtime.columnar import PassThroughOp
    from .functions import FilterFunction, MapFunction

    par = lambda n: n.parallelism or env.parallelism  # noqa: E731
    kids = children.get(t.id, [])
    if len(kids) != 1:
        return
    m = kids[0]
    mmeta = getattr(m, "meta", None) or {}
    spec = None
    for p in t.parents:
        spec = (getattr(p, "meta", None) or {}).get("text_spec") or spec
    arity = spec.arity if spec is not None else (next(iter(ok_arities)) if len(ok_arities) == 1 else None)
    if arity is None or arity not in ok_arities or par(m) != par(t):
        return
    if mmeta.get("kind") == "filter" and not mmeta.get("fused"):
        # window -> filter (BandwidthMonitor.java:37-39): the predicate over the aggregate runs
        # in the fire kernel.
        ff = mmeta["fn"]
        try:
            row = [E.var(E.VAR_RESULT) if i == val_pos else E.FieldRef(f"f{i}") for i in range(arity)]
            r = E.trace_row_fn(ff.filter if isinstance(ff, FilterFunction) else ff, row)
        except E.TraceError:
            return
        if not isinstance(r, E.Expr) or not _expr_vars(r) <= {E.VAR_RESULT}:
            return
        inner, prog = t.factory, E.compile_expr(r)

        def ffactory(inner=inner, prog=prog):
            op = inner()
            op.filter_prog = prog
            return op

        t.factory = ffactory
        m.factory = PassThroughOp
        m.meta = dict(mmeta, fused=True)
        return
    if mmeta.get("kind") != "map" or mmeta.get("columnar"):
        return
    fn = mmeta["fn"]
    try:
        row = [E.var(E.VAR_RESULT) if i == val_pos else E.FieldRef(f"f{i}") for i in range(arity)]
        out = E.trace_row_fn(fn.map if isinstance(fn, MapFunction) else fn, row)
        from .tuples import Tuple

        comps = list(out) if isinstance(out, Tuple) else [out]
        layout, exprs = [], []
        for c in comps:
            if isinstance(c, E.FieldRef):
                layout.append(int(c.name[1:]))
            elif isinstance(c, E.Expr):
                if not _expr_vars(c) <= {E.VAR_RESULT}:
                    return
                layout.append(-1)
                exprs.append(c)
            else:
                return
        if len(exprs) > 1:
            return
        map_prog = E.compile_expr(exprs[0]) if exprs else E.EMPTY
        filt_prog, fnode = E.EMPTY, None
        mk = children.get(m.id, [])
        if len(mk) == 1 and (getattr(mk[0], "meta", None) or {}).get("kind") == "filter" \
                and par(mk[0]) == par(m):
            ff = mk[0].meta["fn"]
            row2 = [E.var(E.VAR_MAPPED) if j < 0 else E.FieldRef(f"f{j}") for j in layout]
            try:
                r2 = E.trace_row_fn(ff.filter if isinstance(ff, FilterFunction) else ff,
                                    row2 if isinstance(out, Tuple) else [E.var(E.VAR_MAPPED)])
                if not isinstance(out, Tuple):
                    r2 = ff.filter(E.var(E.VAR_MAPPED)) if isinstance(ff, FilterFunction) else ff(E.var(E.VAR_MAPPED))
                if isinstance(r2, E.Expr) and _expr_vars(r2) <= {E.VAR_MAPPED, E.VAR_RESULT}:
                    filt_prog, fnode = E.compile_expr(r2), mk[0]
            except E.TraceError:
                pass
    except E.TraceError:
        return
    inner = t.factory
    scalar = not isinstance(out, Tuple)

    def factory(inner=inner, map_prog=map_prog, filt_prog=filt_prog, layout=tuple(layout)):
        op = inner()
        op.map_prog, op.filter_prog = map_prog, filt_prog
        op.fused_layout = None if scalar else layout
        op.fused_scalar = scalar
        return op

    t.factory = factory
    t.meta = dict(t.meta, fused_layout=None if scalar else tuple(layout), fused_scalar=scalar,
                  fused_map=bool(exprs))
    m.factory = PassThroughOp
    m.meta = dict(mmeta, fused=True)
    if fnode is not None:
        fnode.factory = PassThroughOp
        fnode.meta = dict(fnode.meta, fused=True)


def _install_native(env, t, ws, spec, key_pos, val_pos, kind, result, ok_arities,
                    session: bool = False):
    from ..runtime import operators as O
    from ..runtime.native_ops import NativeSessionOp, NativeWindowOp
    from .tuples import Tuple

    fallback = t.factory
    assigner, late, tag = ws.assigner, ws._lateness, ws._late_tag
    key_fn = ws.keyed.key_fn

    if result == "value":
        def builder(template, res, key):
            return res
    else:
        def builder(template, res, key, vp=val_pos):
            row = list(template)
            row[vp] = res
            return Tuple(row)

    device = env.config.device

    from ..runtime.native_ops import NativeMedianOp

    from ..runtime.native_ops import NativeVectorWindowOp

    if session and kind in ("vsum", "vavg"):
        return  # merging windows over vectors: exact host operator
    cls = NativeSessionOp if session else (
        NativeMedianOp if kind in ("median", "quantiles", "distinct") else
        NativeVectorWindowOp if kind in ("vsum", "vavg") else NativeWindowOp)
    # Input straight from the device ingest: the operator knows its column kinds up front and
    # shares the ingest's dictionary (the G > 1 device exchange needs both before any data).
    device_input = None
    for p in t.parents:
        pm = getattr(p, "meta", None) or {}
        if pm.get("device_ingest") is not None and pm.get("text_spec") is not None:
            device_input = (tuple(k for _, k in pm["text_spec"].fields), pm["device_ingest"])

    def factory():
        op = cls(key_fn=key_fn, key_pos=key_pos, val_pos=val_pos, kind=kind,
                 assigner=assigner, lateness=late, late_tag=tag, device=device,
                 fallback_factory=fallback, result_builder=builder, ok_arities=ok_arities)
        op.device_input = device_input
        op.scalar_result = result == "value"
        if kind == "quantiles":
            op.quantiles_ppm = tuple(spec.fn.native[2])
        op.dense_budget = int(env.config.window_dense_max_keys)
        return op

    t.factory = factory
    t.meta = dict(t.meta, native=True)
    _ = O


def _install_native_rolling(env, t, meta):
    """keyBy(<int field>).sum/min/max(p) -> NativeRollingOp (ComputeCpuMax.java:26)."""
    from ..runtime.native_ops import NativeRollingOp

    fallback = t.factory
    device = env.config.device
    key_fn, key_pos, pos, kind = meta["key_fn"], meta["key_pos"], meta["pos"], meta["agg"]
    device_input, event_ts = None, True
    for p in t.parents:
        pm = getattr(p, "meta", None) or {}
        if pm.get("device_ingest") is not None and pm.get("text_spec") is not None:
            device_input = (tuple(k for _, k in pm["text_spec"].fields), pm["device_ingest"])
            event_ts = bool(pm.get("event_ts"))

    def factory():
        op = NativeRollingOp(key_fn=key_fn, key_pos=key_pos, val_pos=pos, kind=kind,
                             device=device, fallback_factory=fallback)
        op.device_input, op.event_ts = device_input, event_ts
        return op

    t.factory = factory
    t.meta = dict(t.meta, native=True)


def _install_native_rolling_by(env, t, meta):
    """keyBy(<field>).maxBy/minBy(p) -> NativeRollingByOp: the arg-select scan names the record
    that holds each key's extremum and the operator carries that record's row. Key selectors
    that are not a position keep the host operator."""
    from ..runtime.native_ops import NativeRollingByOp

    fallback = t.factory
    device = env.config.device
    key_fn, key_pos, pos, kind = meta["key_fn"], meta["key_pos"], meta["pos"], meta["agg"]
    if pos < 0 or pos == key_pos:
        return

    def factory():
        return NativeRollingByOp(key_fn=key_fn, key_pos=key_pos, val_pos=pos, kind=kind,
                                 device=device, fallback_factory=fallback)

    t.factory = factory
    t.meta = dict(t.meta, native=True)


_JOIN_RIGHT = 100  # variable ids of the right row's fields in a traced join function


def trace_join_projection(fn, key_pos, al: int, ar: int):
    """Trace `fn(left, right)` over rows of arity `al` / `ar`. Returns (layout, left value field,
    right value field) when the result is a tuple whose every field is a bare key reference (of
    either side: "k") or a bare reference to the one non-key field of its side ("l" / "r"), and
    both sides' values appear; None otherwise (arithmetic, a non-tuple result, a second value
    field of one side, a flat join function, a function that does not trace)."""
    from .joins import _is_flat_join

    if _is_flat_join(fn) or al <= key_pos[0] or ar <= key_pos[1]:
        return None
    call = fn.join if hasattr(fn, "join") else fn
    left = E.RowProxy([E.FieldRef("key") if j == key_pos[0] else E.var(j) for j in range(al)])
    right = E.RowProxy([E.FieldRef("key") if j == key_pos[1] else E.var(_JOIN_RIGHT + j)
                        for j in range(ar)])
    try:
        res = call(left, right)
    except Exception:  # noqa: BLE001 -- anything that does not trace keeps the host operators
        return None
    if not isinstance(res, tuple) or isinstance(res, E.RowProxy) or not res:
        return None
    layout, vals = [], [None, None]
    for f in res:
        if isinstance(f, E.FieldRef):
            layout.append("k")
        elif isinstance(f, E.Expr) and f.op == "var":
            side, j = divmod(int(f.value), _JOIN_RIGHT)
            if vals[side] not in (None, j):
                return None
            vals[side] = j
            layout.append("lr"[side])
        else:
            return None
    if vals[0] is None or vals[1] is None:
        return None
    return tuple(layout), vals[0], vals[1]


def _lower_join(env, t, meta) -> None:
    """``a.join(b).where(p).equal_to(q).window(w).apply(fn)`` -> NativeJoinOp when both keys are
    field positions, `w` is a tumbling / sliding event-time assigner with the default trigger,
    no evictor, lateness 0 and no late tag, one rank runs the job and `fn` traces to a
    projection (trace_join_projection). Anything else -- and every co-group -- keeps the host
    plan: tagged union -> keyed window -> the co-group function."""
    from ..runtime.native_ops import NativeJoinOp

    ws = meta["stream"]
    a = ws.assigner
    kp = meta["key_pos"]
    comm = getattr(env, "_comm", None)
    world = comm.world if comm is not None else getattr(env, "world", 1)
    if meta.get("co_group") or kp[0] is None or kp[1] is None or world > 1:
        return
    if type(a) not in (W.TumblingEventTimeWindows, W.SlidingEventTimeWindows):
        return
    if ws._trigger is not None or ws._evictor is not None or ws._lateness or \
            ws._late_tag is not None:
        return
    fn = meta["fn"]
    shape, ok = None, (set(), set())
    for side in (0, 1):
        for ar in range(2, 9):
            tr = trace_join_projection(fn, kp, ar if side == 0 else 8, 8 if side == 0 else ar)
            if tr is None:
                continue
            if shape is None:
                shape = tr
            if tr == shape:
                ok[side].add(ar)
    if shape is None or not ok[0] or not ok[1]:
        return
    layout, lval, rval = shape
    fallback = t.factory
    device = env.config.device
    assigner = a

    def factory():
        return NativeJoinOp(key_pos=kp, val_pos=(lval, rval), layout=layout,
                            ok_arities=(frozenset(ok[0]), frozenset(ok[1])), assigner=assigner,
                            device=device, fallback_factory=fallback)

    t.factory = factory
    t.meta = dict(t.meta, native=True)
    meta["columnar"]["on"] = True  # the tag operators let column batches through as they are


class _PoisonedContext:
    """The `ctx` of a traced ProcessJoinFunction: any use ends the trace."""

    def __getattr__(self, name):
        raise TypeError("ctx is not available to a traced join function")


def _as_join_fn(fn):
    """`fn` as a ``(left, right) -> value`` callable for trace_join_projection: a plain callable
    as it is; a ProcessJoinFunction when it collects exactly one value and leaves `ctx` alone."""
    from . import functions as F

    if not isinstance(fn, F.ProcessJoinFunction):
        return fn

    def call(left, right):
        col = F.Collector()
        fn.process_element(left, right, _PoisonedContext(), col)
        if len(col.items) != 1:
            raise TypeError("not exactly one collect")
        return col.items[0]

    return call


def _lower_interval_join(env, t, meta) -> None:
    """``a.interval_join(b).between(lo, hi).process(fn)`` -> NativeIntervalJoinOp when both keys
    are field positions, one rank runs the job and `fn` traces to a projection: exactly one
    collect of a tuple whose fields are bare key references or the one value field of a side.
    Anything else keeps the host plan: tagged union -> keyed IntervalJoinOp."""
    from ..runtime.native_ops import NativeIntervalJoinOp

    kp = meta["key_pos"]
    comm = getattr(env, "_comm", None)
    world = comm.world if comm is not None else getattr(env, "world", 1)
    if kp[0] is None or kp[1] is None or world > 1:
        return
    call = _as_join_fn(meta["fn"])
    shape, ok = None, (set(), set())
    for side in (0, 1):
        for ar in range(2, 9):
            tr = trace_join_projection(call, kp, ar if side == 0 else 8, 8 if side == 0 else ar)
            if tr is None:
                continue
            if shape is None:
                shape = tr
            if tr == shape:
                ok[side].add(ar)
    if shape is None or not ok[0] or not ok[1]:
        return
    layout, lval, rval = shape
    fallback = t.factory
    device = env.config.device
    lo, hi = meta["lo"], meta["hi"]

    def factory():
        return NativeIntervalJoinOp(key_pos=kp, val_pos=(lval, rval), layout=layout,
                                    ok_arities=(frozenset(ok[0]), frozenset(ok[1])), lo=lo, hi=hi,
                                    device=device, fallback_factory=fallback)

    t.factory = factory
    t.meta = dict(t.meta, native=True)
    meta["columnar"]["on"] = True  # the tag operators let column batches through as they are


def _lower_connect(env, t, meta) -> None:
    """``a.connect(b).key_by(p, q).process(fn)`` -> NativeLookupOp when `fn` is exactly a
    ``LookupLatest`` (not a subclass, whose methods may differ), both keys are field positions and
    one rank runs the job. Anything else -- co-maps, co-flat-maps, any other CoProcessFunction,
    key selectors, several ranks -- keeps the host plan: tagged union -> (keyed) host operator."""
    from ..runtime.native_ops import NativeLookupOp
    from . import functions as F

    fn, kp = meta["fn"], meta["key_pos"]
    comm = getattr(env, "_comm", None)
    world = comm.world if comm is not None else getattr(env, "world", 1)
    if meta.get("op") != "process" or type(fn) is not F.LookupLatest or kp is None \
            or kp[0] is None or kp[1] is None or world > 1:
        return
    if isinstance(fn.default, int) and abs(fn.default) > (1 << 53):
        return  # not a double: the host operator keeps the exact integer
    fallback = t.factory
    device = env.config.device
    val_pos = (fn.value_field, fn.state_field)
    arities = tuple(range(max(kp[s], val_pos[s]) + 1, 1 << 16) for s in (0, 1))

    def factory():
        return NativeLookupOp(fn=fn, key_pos=kp, val_pos=val_pos, ok_arities=arities,
                              device=device, fallback_factory=fallback)

    t.factory = factory
    t.meta = dict(t.meta, native=True)
    meta["columnar"]["on"] = True  # the tag operators let column batches through as they are


def _lower_broadcast_connect(env, t, meta) -> None:
    """``a.key_by(p).connect(b.broadcast(RuleSetAlert.DESCRIPTOR)).process(fn)`` ->
    NativeRuleSetOp when `fn` is exactly a ``RuleSetAlert`` (not a subclass, whose methods may
    differ), the first input is keyed by a field position and one rank runs the job. Anything
    else -- any other function, a key selector, the non-keyed form -- keeps the host
    BroadcastProcessOp."""
    from ..runtime.native_ops import NativeRuleSetOp
    from . import functions as F

    fn, kp = meta["fn"], meta["key_pos"]
    comm = getattr(env, "_comm", None)
    world = comm.world if comm is not None else getattr(env, "world", 1)
    if type(fn) is not F.RuleSetAlert or kp is None or world > 1:
        return
    fallback = t.factory
    device = env.config.device

    def factory():
        return NativeRuleSetOp(fn=fn, key_pos=kp, device=device, fallback_factory=fallback)

    t.factory = factory
    t.meta = dict(t.meta, native=True)
    meta["columnar"]["on"] = True  # the tag operators let column batches through as they are


def _lower_keyed_process(env, t, meta) -> None:
    """``stream.key_by(p).process(fn)`` -> NativeTimeoutOp when `fn` is exactly a
    ``CountWithTimeout``, -> NativeSustainOp when it is exactly a ``SustainedAlert``, ->
    NativeBurstOp when it is exactly a ``BurstAlert`` with ``times <= 16``, the width of the
    engine's per-key ring, and -> NativeStateMachineOp when it is exactly a
    ``StateMachineAlert`` with at most 16 states and 16 classes, what one packed function holds,
    and -> NativeCounterRateOp when it is exactly a ``CounterRate``
    (not a subclass, whose methods may differ), the key is a field position and one rank runs
    the job. Every other keyed process function, a ``BurstAlert`` with more `times`, a
    ``StateMachineAlert`` with a larger table, key selectors and several ranks keep the host
    KeyedProcessOp.

    ``EventTimeOrdered(fn)`` (exactly that class) around exactly a ``SustainedAlert``, a
    ``BurstAlert``, a ``StateMachineAlert`` or a ``CounterRate`` lowers, under the same conditions, onto the same
    operators with ``ordered=True``: the device reorder buffer in front of the rule."""
    from ..ops.kernels import BURST_MAX_TIMES, FSM_MAX_CLASSES, FSM_MAX_STATES
    from ..runtime.native_ops import (NativeBurstOp, NativeCounterRateOp, NativeStateMachineOp,
                                      NativeSustainOp, NativeTimeoutOp)
    from . import functions as F

    fn, kp = meta["fn"], meta["key_pos"]
    comm = getattr(env, "_comm", None)
    world = comm.world if comm is not None else getattr(env, "world", 1)
    kw = {}
    if type(fn) is F.EventTimeOrdered:
        # the device reorder buffer in front of the rules; any other wrapped function keeps the
        # host wrapper
        fn, kw = fn.fn, {"ordered": True}
        if type(fn) not in (F.SustainedAlert, F.BurstAlert, F.StateMachineAlert, F.CounterRate):
            return
    native = {F.CountWithTimeout: NativeTimeoutOp, F.SustainedAlert: NativeSustainOp,
              F.BurstAlert: NativeBurstOp,
              F.StateMachineAlert: NativeStateMachineOp,
              F.CounterRate: NativeCounterRateOp}.get(type(fn))
    if native is None or kp is None or world > 1:
        return
    if native is NativeBurstOp and fn.times > BURST_MAX_TIMES:
        return
    if native is NativeStateMachineOp and (len(fn.table) > FSM_MAX_STATES
                                           or len(fn.bounds) + 1 > FSM_MAX_CLASSES):
        return
    fallback = t.factory
    device = env.config.device

    def factory():
        return native(fn=fn, key_pos=kp, device=device, fallback_factory=fallback, **kw)

    t.factory = factory
    t.meta = dict(t.meta, native=True)
