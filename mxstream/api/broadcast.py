"""Broadcast state (Flink 1.8): ``rules.broadcast(descriptor)`` makes a ``BroadcastStream``,
``samples[.key_by(k)].connect(broadcast_stream)`` a ``BroadcastConnectedStream`` and
``.process(fn)`` runs a ``KeyedBroadcastProcessFunction`` (keyed first input) or a
``BroadcastProcessFunction`` (non-keyed): every element of the broadcast input reaches every
parallel instance, which keeps its own copy of the declared map states; the first input reads
them. One rule set for all keys, changed while the job runs.

The plan is connect's (api/connect.py): both inputs are tagged with their side (runtime/columnar.py
TagSideOp) and unioned (watermark = the minimum of the two inputs'). The union is not keyed: the
operator (runtime/operators.py BroadcastProcessOp) keys side 0 itself with the first input's
selector. It carries ``meta = {"kind": "broadcast_connect", ...}``; the planner (api/planner.py
_lower_broadcast_connect) replaces a keyed ``process(RuleSetAlert(..))`` by the native rule-set
operator.
"""
from __future__ import annotations

from . import functions as F
from .datastream import DataStream, KeyedStream
from .state import MapStateDescriptor


class BroadcastStream:
    """A stream whose elements go to every parallel instance of the operator it is connected to,
    with the map states that operator keeps of them."""

    def __init__(self, stream: DataStream, descriptors):
        if not descriptors:
            raise ValueError("broadcast(): at least one MapStateDescriptor is expected (a "
                             "broadcast partitioner without state is not supported)")
        for d in descriptors:
            if not isinstance(d, MapStateDescriptor):
                raise TypeError("broadcast(): MapStateDescriptors are expected")
        self.stream = stream
        self.env = stream.env
        self.descriptors = tuple(descriptors)

    def get_broadcast_state_descriptors(self):
        return list(self.descriptors)

    getBroadcastStateDescriptors = get_broadcast_state_descriptors


class BroadcastConnectedStream:
    def __init__(self, first: DataStream, second: BroadcastStream):
        if first.env is not second.env:
            raise ValueError("both inputs must belong to one execution environment")
        self.first, self.second = first, second
        self.env = first.env

    @property
    def keyed(self) -> bool:
        return isinstance(self.first, KeyedStream)

    def get_first_input(self) -> DataStream:
        return self.first

    def get_second_input(self) -> BroadcastStream:
        return self.second

    def process(self, fn):
        if isinstance(fn, F.KeyedBroadcastProcessFunction):
            if not self.keyed:
                raise TypeError("A KeyedBroadcastProcessFunction can only be used on a keyed "
                                "stream.")
        elif isinstance(fn, F.BroadcastProcessFunction):
            if self.keyed:
                raise TypeError("A BroadcastProcessFunction can only be used on a non-keyed "
                                "stream.")
        else:
            raise TypeError("process(): a KeyedBroadcastProcessFunction or a "
                            "BroadcastProcessFunction is expected")
        from ..runtime import operators as O
        from ..runtime.columnar import TagSideOp

        columnar = {"on": False}  # the planner switches the tag operators to column batches
        plain = lambda s: getattr(s, "_one_input_plain", s._one_input)  # noqa: E731
        tagged = [plain(s)("Connect(tag)", lambda i=i: TagSideOp(i, columnar["on"]))
                  for i, s in enumerate((self.first, self.second.stream))]
        union = tagged[0].union(tagged[1])
        key_fn = self.first.key_fn if self.keyed else None
        descriptors = self.second.descriptors
        op = union._one_input("Co-Process-Broadcast-Keyed" if self.keyed
                              else "Co-Process-Broadcast",
                              lambda: O.BroadcastProcessOp(key_fn, fn, descriptors))
        op.t.meta = {"kind": "broadcast_connect", "fn": fn,
                     "key_pos": self.first.key_pos if self.keyed else None,
                     "columnar": columnar}
        return op

    getFirstInput = get_first_input
    getSecondInput = get_second_input
