"""Connected streams (Flink 1.8 ``ConnectedStreams``): ``a.connect(b)`` feeds two streams of any
two types into one operator that keeps them apart -- ``map(CoMapFunction)``,
``flat_map(CoFlatMapFunction)``, ``process(CoProcessFunction)``. Keyed connected streams (both
inputs ``KeyedStream``s, or ``.key_by(k1, k2)``) share one keyed state and one timer service: what
input 2 writes for a key is what input 1 reads for it -- rules that change while the job runs.

The plan is the joins' (api/joins.py): both inputs are tagged with their side (runtime/columnar.py
TagSideOp) and unioned (watermark = the minimum of the two inputs'); keyed streams are then keyed
by the side's own selector. The operator (runtime/operators.py CoMapOp / CoFlatMapOp /
CoProcessOp) carries ``meta = {"kind": "connect", ...}``; the planner (api/planner.py
_lower_connect) replaces a keyed ``process(LookupLatest(..))`` by the native lookup operator.
"""
from __future__ import annotations

from . import functions as F
from .datastream import DataStream, KeyedStream
from .joins import _selector


class ConnectedStreams:
    def __init__(self, first: DataStream, second: DataStream, keys=None):
        if not isinstance(second, DataStream):
            raise TypeError("the other input must be a DataStream")
        if first.env is not second.env:
            raise ValueError("both inputs must belong to one execution environment")
        self.first, self.second = first, second
        self.env = first.env
        if keys is None and isinstance(first, KeyedStream) and isinstance(second, KeyedStream):
            # Flink's rule: two keyed inputs make keyed connected streams
            keys = ((first.key_fn, first.key_pos), (second.key_fn, second.key_pos))
        self._keys = keys  # ((key fn, position | None), (key fn, position | None)) | None

    @property
    def keyed(self) -> bool:
        return self._keys is not None

    def get_first_input(self) -> DataStream:
        return self.first

    def get_second_input(self) -> DataStream:
        return self.second

    def key_by(self, key1, key2) -> "ConnectedStreams":
        """Key both inputs: field positions, field expressions or key selectors."""
        return ConnectedStreams(self.first, self.second,
                                (_selector(key1, "key_by"), _selector(key2, "key_by")))

    # -- the plan ------------------------------------------------------------------------------
    def _build(self, name: str, kind: str, fn, make_op):
        from ..runtime.columnar import TagSideOp

        columnar = {"on": False}  # the planner switches the tag operators to column batches
        plain = lambda s: getattr(s, "_one_input_plain", s._one_input)  # noqa: E731
        tagged = [plain(s)("Connect(tag)", lambda i=i: TagSideOp(i, columnar["on"]))
                  for i, s in enumerate((self.first, self.second))]
        union = tagged[0].union(tagged[1])
        key_fn = key_pos = None
        if self.keyed:
            (ka, pa), (kb, pb) = self._keys
            key_fn = lambda tv: F.call_key(ka if tv[0] == 0 else kb, tv[1])  # noqa: E731
            key_pos = (pa, pb)
            union = union.key_by(key_fn)
        op = union._one_input(name, lambda: make_op(key_fn))
        op.t.meta = {"kind": "connect", "op": kind, "fn": fn, "key_pos": key_pos,
                     "columnar": columnar}
        return op

    def map(self, fn: F.CoMapFunction):
        if not (callable(getattr(fn, "map1", None)) and callable(getattr(fn, "map2", None))):
            raise TypeError("map(): a CoMapFunction with map1 / map2 is expected")
        from ..runtime import operators as O

        return self._build("Co-Map", "map", fn, lambda _k: O.CoMapOp(fn))

    def flat_map(self, fn: F.CoFlatMapFunction):
        if not (callable(getattr(fn, "flat_map1", None))
                and callable(getattr(fn, "flat_map2", None))):
            raise TypeError("flat_map(): a CoFlatMapFunction with flat_map1 / flat_map2 is "
                            "expected")
        from ..runtime import operators as O

        return self._build("Co-Flat Map", "flat_map", fn, lambda _k: O.CoFlatMapOp(fn))

    def process(self, fn: F.CoProcessFunction):
        if not isinstance(fn, F.CoProcessFunction):
            raise TypeError("process(): a CoProcessFunction is expected")
        from ..runtime import operators as O

        return self._build("Co-Process", "process", fn, lambda k: O.CoProcessOp(k, fn))

    keyBy = key_by
    flatMap = flat_map
    getFirstInput = get_first_input
    getSecondInput = get_second_input
