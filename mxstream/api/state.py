"""Keyed state: descriptors + the host (heap) keyed state backend.

Flink state kinds the reference exercises through its operators (SURVEY.md F-kstate):
ValueState (rolling ``max``, ComputeCpuMax.java:26), ReducingState (window ``reduce``,
BandwidthMonitor.java:37), AggregatingState (window ``aggregate``, ComputeCpuAvg.java:31),
ListState (window ``process``, ComputeCpuMiddle.java:34); MapState completes the API.

State is partitioned by key group (``murmur(hash) % maxParallelism``) so snapshots can be
written per key group and restored at a different parallelism. The GPU-resident keyed state
for the hot aggregation paths lives in ``mxstream.runtime`` (HBM hash sub-tables); this backend
serves user functions that need arbitrary Python values.
"""
from __future__ import annotations

import copy
from typing import Any, Callable

from ..utils.hashing import key_group
from .functions import AggregateFunction, _acc_fns, call_reduce


class StateDescriptor:
    kind = "value"

    def __init__(self, name: str, type_info: Any = None, default_value: Any = None):
        self.name = name
        self.type_info = type_info
        self.default_value = default_value

    def get_name(self) -> str:
        return self.name


class ValueStateDescriptor(StateDescriptor):
    kind = "value"


class ListStateDescriptor(StateDescriptor):
    kind = "list"


class MapStateDescriptor(StateDescriptor):
    kind = "map"

    def __init__(self, name: str, key_type: Any = None, value_type: Any = None):
        super().__init__(name, (key_type, value_type))


class ReducingStateDescriptor(StateDescriptor):
    kind = "reducing"

    def __init__(self, name: str, reduce_function, type_info: Any = None):
        super().__init__(name, type_info)
        self.reduce_function = reduce_function


class AggregatingStateDescriptor(StateDescriptor):
    kind = "aggregating"

    def __init__(self, name: str, agg_function: AggregateFunction, type_info: Any = None):
        super().__init__(name, type_info)
        self.agg_function = agg_function


class StateTtlConfig:
    """Accepted for API compatibility (Flink 1.8 StateTtlConfig); TTL is enforced by the
    backend's ``expire(now)`` sweep."""

    def __init__(self, ttl_ms: int):
        self.ttl_ms = ttl_ms

    @staticmethod
    def new_builder(ttl) -> "StateTtlConfig":
        from .time import to_ms

        return StateTtlConfig(to_ms(ttl))

    def build(self) -> "StateTtlConfig":
        return self


class _StateBase:
    def __init__(self, backend: "HeapKeyedStateBackend", desc: StateDescriptor):
        self._b = backend
        self._d = desc

    def _table(self) -> dict:
        return self._b._table(self._d.name)

    def _k(self):
        return (self._b.current_key, self._b.current_namespace)

    def clear(self) -> None:
        self._table().pop(self._k(), None)


class ValueState(_StateBase):
    def value(self):
        v = self._table().get(self._k(), None)
        if v is None:
            return copy.copy(self._d.default_value)
        return v

    def update(self, value) -> None:
        if value is None:
            self.clear()
        else:
            self._table()[self._k()] = value


class ListState(_StateBase):
    def get(self) -> list:
        return self._table().get(self._k(), [])

    def add(self, value) -> None:
        self._table().setdefault(self._k(), []).append(value)

    def add_all(self, values) -> None:
        self._table().setdefault(self._k(), []).extend(values)

    def update(self, values) -> None:
        self._table()[self._k()] = list(values)

    addAll = add_all


class MapState(_StateBase):
    def _m(self) -> dict:
        return self._table().setdefault(self._k(), {})

    def get(self, key):
        return self._table().get(self._k(), {}).get(key)

    def put(self, key, value) -> None:
        self._m()[key] = value

    def put_all(self, d: dict) -> None:
        self._m().update(d)

    def remove(self, key) -> None:
        self._m().pop(key, None)

    def contains(self, key) -> bool:
        return key in self._table().get(self._k(), {})

    def keys(self):
        return list(self._table().get(self._k(), {}).keys())

    def values(self):
        return list(self._table().get(self._k(), {}).values())

    def items(self):
        return list(self._table().get(self._k(), {}).items())

    entries = items

    def is_empty(self) -> bool:
        return not self._table().get(self._k())


class ReducingState(_StateBase):
    def get(self):
        return self._table().get(self._k())

    def add(self, value) -> None:
        t = self._table()
        k = self._k()
        if k in t:
            t[k] = call_reduce(self._d.reduce_function, t[k], value)
        else:
            t[k] = value


class AggregatingState(_StateBase):
    def __init__(self, backend, desc):
        super().__init__(backend, desc)
        self._create, self._add, self._result, self._merge = _acc_fns(desc.agg_function)

    def get(self):
        t = self._table()
        k = self._k()
        if k not in t:
            return None
        return self._result(t[k])

    def get_accumulator(self):
        return self._table().get(self._k())

    def add(self, value) -> None:
        t = self._table()
        k = self._k()
        acc = t[k] if k in t else self._create()
        t[k] = self._add(value, acc)

    def merge_namespaces(self, target, sources) -> None:
        t = self._table()
        key = self._b.current_key
        acc = None
        for ns in sources:
            a = t.pop((key, ns), None)
            if a is not None:
                acc = a if acc is None else self._merge(acc, a)
        if acc is not None:
            cur = t.get((key, target))
            t[(key, target)] = acc if cur is None else self._merge(cur, acc)


class BroadcastState:
    """Broadcast state (Flink 1.8 ``BroadcastState``): a map that every parallel instance of the
    operator holds a copy of (runtime/operators.py BroadcastProcessOp). Read-write on the
    broadcast side of a (Keyed)BroadcastProcessFunction."""

    def __init__(self, entries: dict):
        self._m = entries

    def get(self, key):
        return self._m.get(key)

    def contains(self, key) -> bool:
        return key in self._m

    def immutable_entries(self):
        return tuple(self._m.items())

    def put(self, key, value) -> None:
        self._m[key] = value

    def put_all(self, d: dict) -> None:
        self._m.update(d)

    def remove(self, key) -> None:
        self._m.pop(key, None)

    def entries(self):
        return list(self._m.items())

    def clear(self) -> None:
        self._m.clear()

    putAll = put_all
    immutableEntries = immutable_entries


class ReadOnlyBroadcastState(BroadcastState):
    """The element side's view (``ReadOnlyBroadcastState``): get, contains and
    immutable_entries; a write raises TypeError."""

    def _read_only(self, *_a, **_k):
        raise TypeError("the broadcast state is read-only on the element side: it may only be "
                        "changed in process_broadcast_element")

    put = put_all = remove = entries = clear = putAll = _read_only


_STATE_CLASSES = {"value": ValueState, "list": ListState, "map": MapState,
                  "reducing": ReducingState, "aggregating": AggregatingState}


class HeapKeyedStateBackend:
    """Per-operator keyed state: tables name -> {(key, namespace): value}."""

    def __init__(self, max_parallelism: int = 128, key_hash: Callable | None = None):
        self.max_parallelism = max_parallelism
        self.current_key = None
        self.current_namespace = None
        self._tables: dict[str, dict] = {}
        self._descs: dict[str, StateDescriptor] = {}
        self._key_hash = key_hash

    def _table(self, name: str) -> dict:
        return self._tables.setdefault(name, {})

    def set_current_key(self, key) -> None:
        self.current_key = key

    def set_current_namespace(self, ns) -> None:
        self.current_namespace = ns

    def get_state(self, desc: StateDescriptor):
        prev = self._descs.get(desc.name)
        if prev is not None and prev.kind != desc.kind:
            raise ValueError(f"state '{desc.name}' registered with a different kind")
        self._descs[desc.name] = desc
        return _STATE_CLASSES[desc.kind](self, desc)

    def merge_namespaces(self, desc: StateDescriptor, target, sources) -> None:
        """Merge window namespaces (session windows) for the current key."""
        t = self._table(desc.name)
        key = self.current_key
        if desc.kind == "aggregating":
            AggregatingState(self, desc).merge_namespaces(target, sources)
            return
        acc = None
        for ns in sources:
            v = t.pop((key, ns), None)
            if v is None:
                continue
            if acc is None:
                acc = v
            elif desc.kind == "list":
                acc = acc + v
            elif desc.kind == "reducing":
                acc = call_reduce(desc.reduce_function, acc, v)
            else:
                acc = v
        if acc is not None:
            cur = t.get((key, target))
            if cur is None:
                t[(key, target)] = acc
            elif desc.kind == "list":
                t[(key, target)] = cur + acc
            elif desc.kind == "reducing":
                t[(key, target)] = call_reduce(desc.reduce_function, cur, acc)
            else:
                t[(key, target)] = acc

    def num_entries(self) -> int:
        return sum(len(t) for t in self._tables.values())

    def keys(self, name: str):
        return {k for (k, _ns) in self._tables.get(name, {})}

    # ---- snapshot / restore by key group -------------------------------------------------
    def _kg(self, key) -> int:
        if self._key_hash is not None:
            return self._key_hash(key) % self.max_parallelism
        return key_group(key, self.max_parallelism)

    def snapshot(self) -> dict[int, dict]:
        """{key_group: {state_name: {(key, ns): value}}}"""
        out: dict[int, dict] = {}
        for name, t in self._tables.items():
            for (k, ns), v in t.items():
                out.setdefault(self._kg(k), {}).setdefault(name, {})[(k, ns)] = copy.deepcopy(v)
        return out

    def restore(self, groups: dict[int, dict], kg_range: tuple[int, int] | None = None) -> None:
        for kg, tables in groups.items():
            if kg_range is not None and not (kg_range[0] <= kg <= kg_range[1]):
                continue
            for name, entries in tables.items():
                self._table(name).update(entries)
