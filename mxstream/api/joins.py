"""Window joins and co-groups of two streams (Flink 1.8 ``JoinedStreams`` / ``CoGroupedStreams``).

``a.join(b).where(ka).equal_to(kb).window(assigner)[.trigger(t)][.evictor(e)]
[.allowed_lateness(t)].apply(fn)`` emits ``fn(l, r)`` for every left element ``l`` and every
right element ``r`` of a (key, window) when the window fires -- left-major, each side in arrival
order, timestamped ``window.maxTimestamp()``. A key that only one side has in a window emits
nothing. ``a.co_group(b)...apply(fn(lefts, rights, out))`` is the primitive under it.

The plan is Flink's own, built from the operators that exist: both inputs are tagged with their
side (runtime/columnar.py TagSideOp), unioned (watermark = the minimum of the two inputs'), keyed
by the side's own selector, windowed by `assigner` and handed to ``WindowedStream.apply`` with a
co-group function. The window node carries ``meta = {"kind": "join", ...}``; the planner
(api/planner.py _lower_join) replaces it by the native operator where it can prove the shape.

``a.key_by(ka).interval_join(b.key_by(kb)).between(lo, hi).process(fn)`` (Flink 1.8
``KeyedStream.intervalJoin``, below) pairs elements of one key whose timestamps satisfy
``l.ts + lo <= r.ts <= l.ts + hi``, as they arrive and independent of any window.
"""
from __future__ import annotations

import inspect

from . import functions as F
from . import windowing as W
from .datastream import DataStream, WindowedStream, _field_key


def _selector(k, what: str):
    """A field position / field expression / key selector, like ``key_by``: (key fn, position)."""
    if isinstance(k, bool) or k is None:
        raise TypeError(f"{what}: a field position or a key selector is expected")
    if isinstance(k, int):
        if k < 0:
            raise ValueError(f"{what}: field position {k} is negative")
        return _field_key(k), k
    if isinstance(k, str):
        return _field_key(k), None
    if isinstance(k, F.KeySelector):
        return k.get_key, None
    if callable(k):
        return k, None
    raise TypeError(f"{what}: a field position or a key selector is expected")


def _is_flat_join(fn) -> bool:
    if isinstance(fn, F.FlatJoinFunction):
        return True
    j = getattr(fn, "join", None)
    if j is None or isinstance(fn, F.JoinFunction):
        return False
    try:
        return len(inspect.signature(j).parameters) >= 3
    except (TypeError, ValueError):
        return False


class _TwoStreams:
    """``a.join(b)`` / ``a.co_group(b)``: waits for ``where``."""

    kind = "join"

    def __init__(self, left: DataStream, right: DataStream):
        if not isinstance(right, DataStream):
            raise TypeError("the other input must be a DataStream")
        if left.env is not right.env:
            raise ValueError("both inputs must belong to one execution environment")
        self.left, self.right = left, right

    def where(self, key) -> "_Where":
        return _Where(self, *_selector(key, "where"))

    def equal_to(self, key):
        raise ValueError("equal_to() before where(): name the left input's key first")

    def window(self, assigner):
        raise ValueError("window() before where().equal_to(): name both keys first")

    equalTo = equal_to


class JoinedStreams(_TwoStreams):
    kind = "join"


class CoGroupedStreams(_TwoStreams):
    kind = "co_group"


class _Where:
    def __init__(self, streams: _TwoStreams, key_fn, key_pos):
        self.streams, self.key_fn, self.key_pos = streams, key_fn, key_pos

    def equal_to(self, key) -> "_EqualTo":
        return _EqualTo(self, *_selector(key, "equal_to"))

    def window(self, assigner):
        raise ValueError("window() before equal_to(): name the right input's key first")

    equalTo = equal_to


class _EqualTo:
    def __init__(self, where: _Where, key_fn, key_pos):
        self.where_, self.key_fn, self.key_pos = where, key_fn, key_pos

    def window(self, assigner: W.WindowAssigner) -> "_WithWindow":
        if not isinstance(assigner, W.WindowAssigner):
            raise TypeError("window(): a WindowAssigner is expected")
        return _WithWindow(self, assigner)


class _WithWindow:
    def __init__(self, eq: _EqualTo, assigner):
        self.eq, self.assigner = eq, assigner
        self._trigger = self._evictor = None
        self._lateness = None

    def trigger(self, trigger) -> "_WithWindow":
        self._trigger = trigger
        return self

    def evictor(self, evictor) -> "_WithWindow":
        self._evictor = evictor
        return self

    def allowed_lateness(self, t) -> "_WithWindow":
        self._lateness = t
        return self

    allowedLateness = allowed_lateness

    def apply(self, fn):
        from ..runtime.columnar import TagSideOp

        streams = self.eq.where_.streams
        ka, kb = self.eq.where_.key_fn, self.eq.key_fn
        if streams.kind == "join":
            cofn = _join_as_co_group(fn)
        else:
            call = fn.co_group if hasattr(fn, "co_group") else fn
            if not callable(call):
                raise TypeError("apply(): a co-group function fn(lefts, rights, out) is expected")
            cofn = _co_group_window_fn(call)
        # tag(0) / tag(1) -> union -> key_by(the side's own selector) -> window -> apply
        columnar = {"on": False}  # the planner switches the tag operators to column batches
        tagged = [s._one_input("Join(tag)", lambda i=i: TagSideOp(i, columnar["on"]))
                  for i, s in enumerate((streams.left, streams.right))]
        keyed = tagged[0].union(tagged[1]).key_by(
            lambda tv: F.call_key(ka if tv[0] == 0 else kb, tv[1]))
        ws = WindowedStream(keyed, self.assigner)
        if self._trigger is not None:
            ws.trigger(self._trigger)
        if self._evictor is not None:
            ws.evictor(self._evictor)
        if self._lateness is not None:
            ws.allowed_lateness(self._lateness)
        op = ws.apply(cofn)
        op.t.meta = {"kind": "join", "co_group": streams.kind != "join", "stream": ws, "fn": fn,
                     "key_pos": (self.eq.where_.key_pos, self.eq.key_pos),
                     "assigner": self.assigner, "columnar": columnar}
        return op


def _split(elements):
    lefts, rights = [], []
    for side, v in elements:
        (lefts if side == 0 else rights).append(v)
    return lefts, rights


def _co_group_window_fn(call):
    def co_group(key, window, elements, out):
        lefts, rights = _split(elements)
        call(lefts, rights, out)

    return co_group


def _join_as_co_group(fn):
    """The nested loop of JoinedStreams' JoinCoGroupFunction: left-major, arrival order."""
    call = fn.join if hasattr(fn, "join") else fn
    if not callable(call):
        raise TypeError("apply(): a join function fn(left, right) is expected")
    flat = _is_flat_join(fn)

    def join(key, window, elements, out):
        lefts, rights = _split(elements)
        for l in lefts:
            for r in rights:
                if flat:
                    call(l, r, out)
                else:
                    out.collect(call(l, r))

    return join


# ---- interval joins (Flink 1.8 KeyedStream.intervalJoin) ---------------------------------------

class IntervalJoin:
    """``a.interval_join(b)``: waits for ``between``. Both inputs are keyed streams of one
    environment; the join is defined in event time only."""

    def __init__(self, left, right):
        from .datastream import KeyedStream
        from .time import TimeCharacteristic

        if not isinstance(left, KeyedStream) or not isinstance(right, KeyedStream):
            raise TypeError("interval_join: both inputs must be keyed streams (key_by first)")
        if left.env is not right.env:
            raise ValueError("both inputs must belong to one execution environment")
        if left.env.time_characteristic != TimeCharacteristic.EventTime:
            raise RuntimeError("Time-bounded stream joins are only supported in event time")
        self.left, self.right = left, right

    def between(self, lower, upper) -> "IntervalJoined":
        from .time import to_ms

        return IntervalJoined(self.left, self.right, to_ms(lower), to_ms(upper))

    def process(self, fn):
        raise ValueError("process() before between(): name the bounds first")


class IntervalJoined:
    """``...between(lo, hi)[.lower_bound_exclusive()][.upper_bound_exclusive()].process(fn)``:
    `fn` is a ProcessJoinFunction, or a plain ``fn(left, right) -> value`` that collects that
    value. The plan: tag(0) / tag(1) -> union -> key_by(the side's own selector) -> the interval
    join operator (runtime/operators.py IntervalJoinOp), whose node carries
    ``meta = {"kind": "interval_join", ...}`` for the planner (_lower_interval_join)."""

    def __init__(self, left, right, lo: int, hi: int):
        self.left, self.right = left, right
        self.lo, self.hi = int(lo), int(hi)
        self._check()

    def _check(self) -> None:
        if self.lo > self.hi:
            raise ValueError("lowerBound <= upperBound must be fulfilled")

    def lower_bound_exclusive(self) -> "IntervalJoined":
        self.lo += 1
        self._check()
        return self

    def upper_bound_exclusive(self) -> "IntervalJoined":
        self.hi -= 1
        self._check()
        return self

    lowerBoundExclusive = lower_bound_exclusive
    upperBoundExclusive = upper_bound_exclusive

    def process(self, fn):
        from ..runtime import operators as O
        from ..runtime.columnar import TagSideOp

        if not isinstance(fn, F.ProcessJoinFunction) and not callable(fn):
            raise TypeError("process(): a ProcessJoinFunction or fn(left, right) is expected")
        ka, kb = self.left.key_fn, self.right.key_fn
        lo, hi = self.lo, self.hi
        columnar = {"on": False}  # the planner switches the tag operators to column batches
        tagged = [s._one_input_plain("Join(tag)", lambda i=i: TagSideOp(i, columnar["on"]))
                  for i, s in enumerate((self.left, self.right))]
        key_fn = lambda tv: F.call_key(ka if tv[0] == 0 else kb, tv[1])  # noqa: E731
        keyed = tagged[0].union(tagged[1]).key_by(key_fn)
        op = keyed._one_input("IntervalJoin", lambda: O.IntervalJoinOp(key_fn, lo, hi, fn))
        op.t.meta = {"kind": "interval_join", "fn": fn, "lo": lo, "hi": hi,
                     "key_pos": (self.left.key_pos, self.right.key_pos), "columnar": columnar}
        return op
