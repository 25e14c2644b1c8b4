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
