"""User-function interfaces (Flink 1.8 ``org.apache.flink.api.common.functions`` and
``streaming.api.functions``). Every operator also accepts a plain Python callable.

Reference uses: MapFunction (Main.java:18), FilterFunction (Main.java:27), ReduceFunction
(BandwidthMonitor.java:37), AggregateFunction (ComputeCpuAvg.java:31-58), ProcessWindowFunction
(ComputeCpuMiddle.java:34-48).
"""
from __future__ import annotations

from typing import Any, Iterable


class Function:
    pass


class RuntimeContext:
    """What a RichFunction sees: subtask info + keyed state access (keyed operators only)."""

    def __init__(self, task_name: str, subtask: int, parallelism: int, max_parallelism: int,
                 state_backend=None, metric_group=None):
        self.task_name = task_name
        self.index_of_this_subtask = subtask
        self.number_of_parallel_subtasks = parallelism
        self.max_number_of_parallel_subtasks = max_parallelism
        self._state = state_backend
        self._metrics = metric_group

    def get_index_of_this_subtask(self) -> int:
        return self.index_of_this_subtask

    def get_number_of_parallel_subtasks(self) -> int:
        return self.number_of_parallel_subtasks

    def get_task_name(self) -> str:
        return self.task_name

    def _require_state(self):
        if self._state is None:
            raise RuntimeError("Keyed state is only available on a KeyedStream")
        return self._state

    def get_state(self, descriptor):
        return self._require_state().get_state(descriptor)

    def get_list_state(self, descriptor):
        return self._require_state().get_state(descriptor)

    def get_map_state(self, descriptor):
        return self._require_state().get_state(descriptor)

    def get_reducing_state(self, descriptor):
        return self._require_state().get_state(descriptor)

    def get_aggregating_state(self, descriptor):
        return self._require_state().get_state(descriptor)

    def get_metric_group(self):
        return self._metrics

    # camelCase aliases
    getState = get_state
    getListState = get_list_state
    getMapState = get_map_state
    getReducingState = get_reducing_state
    getAggregatingState = get_aggregating_state
    getIndexOfThisSubtask = get_index_of_this_subtask
    getNumberOfParallelSubtasks = get_number_of_parallel_subtasks


class RichFunction(Function):
    _runtime_context: RuntimeContext | None = None

    def open(self, parameters=None):
        pass

    def close(self):
        pass

    def get_runtime_context(self) -> RuntimeContext:
        if self._runtime_context is None:
            raise RuntimeError("runtime context not set (function not opened)")
        return self._runtime_context

    def set_runtime_context(self, ctx: RuntimeContext):
        self._runtime_context = ctx

    getRuntimeContext = get_runtime_context


class MapFunction(Function):
    def map(self, value):
        raise NotImplementedError


class RichMapFunction(RichFunction, MapFunction):
    pass


class FilterFunction(Function):
    def filter(self, value) -> bool:
        raise NotImplementedError


class RichFilterFunction(RichFunction, FilterFunction):
    pass


class FlatMapFunction(Function):
    def flat_map(self, value, out: "Collector"):
        raise NotImplementedError

    def flatMap(self, value, out):  # camelCase
        return self.flat_map(value, out)


class RichFlatMapFunction(RichFunction, FlatMapFunction):
    pass


class KeySelector(Function):
    def get_key(self, value):
        raise NotImplementedError

    def getKey(self, value):
        return self.get_key(value)


class ReduceFunction(Function):
    def reduce(self, a, b):
        raise NotImplementedError


class JoinFunction(Function):
    """join(left, right) -> value, once per pair of a (key, window) (JoinedStreams.apply)."""

    def join(self, left, right):
        raise NotImplementedError


class FlatJoinFunction(Function):
    """join(left, right, out): any number of values per pair."""

    def join(self, left, right, out: "Collector"):
        raise NotImplementedError


class CoGroupFunction(Function):
    """co_group(lefts, rights, out): both sides' elements of a (key, window), each in arrival
    order; either list may be empty (CoGroupedStreams.apply)."""

    def co_group(self, lefts, rights, out: "Collector"):
        raise NotImplementedError

    def coGroup(self, lefts, rights, out):
        return self.co_group(lefts, rights, out)


class AggregateFunction(Function):
    """createAccumulator / add / getResult / merge (ComputeCpuAvg.java:33-58)."""

    def create_accumulator(self):
        raise NotImplementedError

    def add(self, value, accumulator):
        raise NotImplementedError

    def get_result(self, accumulator):
        raise NotImplementedError

    def merge(self, a, b):
        raise NotImplementedError

    # Java names map onto the snake_case hooks
    def createAccumulator(self):
        return self.create_accumulator()

    def getResult(self, acc):
        return self.get_result(acc)


def _acc_fns(fn: AggregateFunction):
    """Resolve an AggregateFunction's hooks whether it defines Java or snake names."""

    def pick(snake, camel):
        m = getattr(type(fn), snake, None)
        base = getattr(AggregateFunction, snake)
        if m is not None and m is not base:
            return getattr(fn, snake)
        return getattr(fn, camel)

    return (pick("create_accumulator", "createAccumulator"), fn.add,
            pick("get_result", "getResult"), fn.merge)


class Collector:
    def __init__(self):
        self.items: list = []
        self.stamps: dict = {}   # item index -> timestamp, for items collected with one

    def collect(self, value):
        self.items.append(value)

    def collect_at(self, value, ts):
        """Collect `value` stamped `ts` where the operator would stamp it otherwise (a keyed
        process function's on_timer: the timer's time)."""
        self.stamps[len(self.items)] = ts
        self.items.append(value)


class ProcessWindowFunction(RichFunction):
    """process(key, context, elements, out) (ComputeCpuMiddle.java:36)."""

    class Context:
        def __init__(self, window, current_processing_time: int, current_watermark: int,
                     side_outputs=None):
            self._window = window
            self._pt = current_processing_time
            self._wm = current_watermark
            self._side = side_outputs

        def window(self):
            return self._window

        def current_processing_time(self) -> int:
            return self._pt

        def current_watermark(self) -> int:
            return self._wm

        def output(self, tag, value):
            self._side.setdefault(tag.tag_id, []).append(value)

        currentProcessingTime = current_processing_time
        currentWatermark = current_watermark

    def process(self, key, context, elements: Iterable, out: Collector):
        raise NotImplementedError


class WindowFunction(Function):
    """apply(key, window, input, out)."""

    def apply(self, key, window, inputs: Iterable, out: Collector):
        raise NotImplementedError


class ProcessFunction(RichFunction):
    class Context:
        def __init__(self, ts, timer_service, side_outputs, key=None):
            self._ts = ts
            self._timers = timer_service
            self._side = side_outputs
            self._key = key

        def timestamp(self):
            return self._ts

        def timer_service(self):
            return self._timers

        def output(self, tag, value):
            self._side.setdefault(tag.tag_id, []).append(value)

        def get_current_key(self):
            return self._key

        timerService = timer_service
        getCurrentKey = get_current_key

    def process_element(self, value, ctx, out: Collector):
        raise NotImplementedError

    def on_timer(self, timestamp: int, ctx, out: Collector):
        pass


class KeyedProcessFunction(ProcessFunction):
    pass


class ProcessJoinFunction(RichFunction):
    """process_element(left, right, ctx, out), once per pair of an interval join
    (``a.interval_join(b).between(lo, hi).process(fn)``)."""

    class Context:
        def __init__(self, left_ts: int, right_ts: int, side_outputs):
            self._left, self._right = left_ts, right_ts
            self._side = side_outputs

        def get_left_timestamp(self) -> int:
            return self._left

        def get_right_timestamp(self) -> int:
            return self._right

        def get_timestamp(self) -> int:
            """The pair's timestamp: the larger of the two elements'."""
            return max(self._left, self._right)

        def output(self, tag, value):
            self._side.setdefault(tag.tag_id, []).append(value)

        getLeftTimestamp = get_left_timestamp
        getRightTimestamp = get_right_timestamp
        getTimestamp = get_timestamp

    def process_element(self, left, right, ctx, out: Collector):
        raise NotImplementedError

    def processElement(self, left, right, ctx, out):
        return self.process_element(left, right, ctx, out)


class CoMapFunction(Function):
    """map1(value) / map2(value): one result per element of the first / second connected stream
    (``a.connect(b).map(fn)``)."""

    def map1(self, value):
        raise NotImplementedError

    def map2(self, value):
        raise NotImplementedError


class CoFlatMapFunction(Function):
    """flat_map1(value, out) / flat_map2(value, out): any number of results per element."""

    def flat_map1(self, value, out: "Collector"):
        raise NotImplementedError

    def flat_map2(self, value, out: "Collector"):
        raise NotImplementedError

    def flatMap1(self, value, out):
        return self.flat_map1(value, out)

    def flatMap2(self, value, out):
        return self.flat_map2(value, out)


class CoProcessFunction(RichFunction):
    """process_element1 / process_element2 (value, ctx, out) for the two connected streams and
    on_timer(timestamp, ctx, out); on keyed connected streams both inputs share one keyed state
    and one timer service (``a.connect(b).key_by(k1, k2).process(fn)``)."""

    class Context:
        def __init__(self, ts, timer_service, side_outputs, key=None):
            self._ts = ts
            self._timers = timer_service
            self._side = side_outputs
            self._key = key

        def timestamp(self):
            return self._ts

        def timer_service(self):
            return self._timers

        def output(self, tag, value):
            self._side.setdefault(tag.tag_id, []).append(value)

        def get_current_key(self):
            """The key of keyed connected streams (None otherwise)."""
            return self._key

        timerService = timer_service
        getCurrentKey = get_current_key

    class OnTimerContext(Context):
        def __init__(self, ts, timer_service, side_outputs, time_domain, key=None):
            super().__init__(ts, timer_service, side_outputs, key)
            self.time_domain = time_domain

        timeDomain = property(lambda self: self.time_domain)

    def process_element1(self, value, ctx, out: Collector):
        raise NotImplementedError

    def process_element2(self, value, ctx, out: Collector):
        raise NotImplementedError

    def on_timer(self, timestamp: int, ctx, out: Collector):
        pass

    def processElement1(self, value, ctx, out):
        return self.process_element1(value, ctx, out)

    def processElement2(self, value, ctx, out):
        return self.process_element2(value, ctx, out)

    def onTimer(self, timestamp, ctx, out):
        return self.on_timer(timestamp, ctx, out)


_LOOKUP_WHENS = {
    ">": lambda a, b: a > b, ">=": lambda a, b: a >= b, "<": lambda a, b: a < b,
    "<=": lambda a, b: a <= b, "==": lambda a, b: a == b, "!=": lambda a, b: a != b,
}


class LookupLatest(CoProcessFunction):
    """Keyed latest-value lookup over ``samples.connect(rules).key_by(k1, k2)``: input 2 (the
    rules) stores ``rule[state_field]`` in one ValueState per key and emits nothing; input 1 (the
    samples) reads the value ``t`` in force for its key -- the stored one, else `default`, else the
    sample is dropped -- and collects ``Tuple3(key, sample[value_field], t)`` with the sample's
    timestamp when `when` is None or ``sample[value_field] <when> t`` holds. `when` is one of
    ``">", ">=", "<", "<=", "==", "!="``; values are int or float (not bool) and compare as Java
    compares doubles: a NaN on either side is false for every operator but ``!=``, and
    ``-0.0 == 0.0``. A per-host alert threshold that changes while the job runs:

        samples.connect(rules).key_by(0, 0).process(LookupLatest(2, 1, when=">"))

    The planner runs exactly this class (not a subclass) with positional keys on the device
    lookup operator (runtime/lookup_operator.py); these methods are the exact host
    implementation used otherwise."""

    def __init__(self, value_field: int, state_field: int, when=None, default=None):
        for name, f in (("value_field", value_field), ("state_field", state_field)):
            if isinstance(f, bool) or not isinstance(f, int) or f < 0:
                raise ValueError(f"LookupLatest: {name} is a non-negative int, got {f!r}")
        if when is not None and (not isinstance(when, str) or when not in _LOOKUP_WHENS):
            raise ValueError("LookupLatest: when must be one of '>', '>=', '<', '<=', '==', '!=' "
                             f"or None, got {when!r}")
        if default is not None:
            self._number(default, "default")
        self.value_field, self.state_field = value_field, state_field
        self.when, self.default = when, default
        self.native = ("lookup", value_field, state_field, when, default)

    @staticmethod
    def _number(x, what: str):
        if isinstance(x, bool) or not isinstance(x, (int, float)):
            raise TypeError(f"LookupLatest: {what} must be an int or a float, got {x!r}")
        return x

    def open(self, parameters=None):
        from .state import ValueStateDescriptor

        self._state = self.get_runtime_context().get_state(ValueStateDescriptor("lookup-latest"))

    def process_element2(self, rule, ctx, out):
        self._state.update(self._number(rule[self.state_field], "the rule's value"))

    def process_element1(self, sample, ctx, out):
        from .tuples import Tuple3

        t = self._state.value()
        if t is None:
            t = self.default
        if t is None:
            return
        v = self._number(sample[self.value_field], "the sample's value")
        # Python compares an int with a float exactly; Java compares the two doubles
        if self.when is None or _LOOKUP_WHENS[self.when](float(v), float(t)):
            out.collect(Tuple3(ctx.get_current_key(), v, t))


_NO_BROADCAST_STATE = (
    "The requested state does not exist. Check for typos in your state descriptor, or specify "
    "the state descriptor in the datastream.broadcast(...) call if you forgot to register it.")


class _BaseBroadcastProcessFunction(RichFunction):
    """What BroadcastProcessFunction and KeyedBroadcastProcessFunction share (Flink 1.8
    ``BaseBroadcastProcessFunction``): process_element(value, ctx, out) for the first input with
    a read-only view of the broadcast state, process_broadcast_element(value, ctx, out) for the
    broadcast input, which alone may change it. The operator (runtime/operators.py
    BroadcastProcessOp) calls process_broadcast_element once per parallel instance, each with
    that instance's copy of the state."""

    class Context:
        """The broadcast side: the state is read-write."""

        _read_only = False

        def __init__(self, ts, states: dict, side_outputs, watermark, clock):
            self._ts = ts
            self._states = states        # descriptor name -> this instance's entries
            self._side = side_outputs
            self._wm, self._clock = watermark, clock

        def get_broadcast_state(self, descriptor):
            from .state import BroadcastState, ReadOnlyBroadcastState

            entries = self._states.get(getattr(descriptor, "name", None))
            if entries is None:
                raise ValueError(_NO_BROADCAST_STATE)
            return (ReadOnlyBroadcastState if self._read_only else BroadcastState)(entries)

        def timestamp(self):
            return self._ts

        def current_watermark(self):
            return self._wm()

        def current_processing_time(self):
            return self._clock()

        def output(self, tag, value):
            self._side.setdefault(tag.tag_id, []).append(value)

        getBroadcastState = get_broadcast_state
        currentWatermark = current_watermark
        currentProcessingTime = current_processing_time

    class ReadOnlyContext(Context):
        """The element side: the state is read-only."""

        _read_only = True

    def process_element(self, value, ctx, out: Collector):
        raise NotImplementedError

    def process_broadcast_element(self, value, ctx, out: Collector):
        raise NotImplementedError

    def processElement(self, value, ctx, out):
        return self.process_element(value, ctx, out)

    def processBroadcastElement(self, value, ctx, out):
        return self.process_broadcast_element(value, ctx, out)


class BroadcastProcessFunction(_BaseBroadcastProcessFunction):
    """``stream.connect(rules.broadcast(descriptor)).process(fn)`` on a non-keyed first input: no
    keyed state, no timers, no key."""


class KeyedBroadcastProcessFunction(_BaseBroadcastProcessFunction):
    """``stream.key_by(k).connect(rules.broadcast(descriptor)).process(fn)``: the element side
    also has keyed state, a timer service and the current key; the broadcast side may visit the
    keyed state of every key (``apply_to_keyed_state``); on_timer(timestamp, ctx, out) sees the
    read-only broadcast state."""

    class Context(_BaseBroadcastProcessFunction.Context):
        def __init__(self, ts, states, side_outputs, watermark, clock, apply):
            super().__init__(ts, states, side_outputs, watermark, clock)
            self._apply = apply

        def apply_to_keyed_state(self, state_descriptor, fn):
            """``fn(key, state)`` for every key of this parallel instance that has the state."""
            self._apply(state_descriptor, fn)

        applyToKeyedState = apply_to_keyed_state

    class ReadOnlyContext(_BaseBroadcastProcessFunction.ReadOnlyContext):
        def __init__(self, ts, states, side_outputs, watermark, clock, timer_service, key):
            super().__init__(ts, states, side_outputs, watermark, clock)
            self._timers, self._key = timer_service, key

        def timer_service(self):
            return self._timers

        def get_current_key(self):
            return self._key

        timerService = timer_service
        getCurrentKey = get_current_key

    class OnTimerContext(ReadOnlyContext):
        def __init__(self, ts, states, side_outputs, watermark, clock, timer_service, key,
                     time_domain):
            super().__init__(ts, states, side_outputs, watermark, clock, timer_service, key)
            self.time_domain = time_domain

        timeDomain = property(lambda self: self.time_domain)

    def on_timer(self, timestamp: int, ctx, out: Collector):
        pass

    def onTimer(self, timestamp, ctx, out):
        return self.on_timer(timestamp, ctx, out)


class RuleSetAlert(KeyedBroadcastProcessFunction):
    """A rule set that holds for every key, changed while the job runs, over
    ``samples.key_by(k).connect(rules.broadcast(RuleSetAlert.DESCRIPTOR))``. A rule
    ``(id, when, threshold)`` of the broadcast input is stored as ``id -> (when, threshold)`` in
    the broadcast state, the last rule of an id wins, ``when`` None withdraws the rule and nothing
    is emitted. A sample collects, for the rules in ascending id, ``Tuple4(key,
    sample[value_field], id, threshold)`` with the sample's timestamp where
    ``sample[value_field] <when> threshold`` holds. `when` is one of ``">", ">=", "<", "<=", "==",
    "!="``; values and thresholds are int or float (not bool) and compare as Java compares
    doubles: a NaN on either side is false for every operator but ``!=``, and ``-0.0 == 0.0``.
    Warning at 80, critical at 95, suspiciously idle below 1:

        samples.key_by(0).connect(rules.broadcast(RuleSetAlert.DESCRIPTOR)) \\
            .process(RuleSetAlert(2)).print()
        # rules:  (1, ">", 80.0)  (2, ">", 95.0)  (3, "<", 1.0)  ...  (1, None, 0) withdraws rule 1
        # (host, usage, rule id, threshold): one line per sample and rule that the sample breaks

    The planner runs exactly this class (not a subclass) with a positional key on the device
    rule-set operator (runtime/ruleset_operator.py); these methods are the exact host
    implementation used otherwise."""

    class _RuleSetDescriptor:
        """``MapStateDescriptor("rule-set")``, made at first use (api/state.py imports this
        module)."""

        def __get__(self, obj, cls):
            from .state import MapStateDescriptor

            RuleSetAlert.DESCRIPTOR = MapStateDescriptor("rule-set")
            return RuleSetAlert.DESCRIPTOR

    DESCRIPTOR = _RuleSetDescriptor()

    def __init__(self, value_field: int, id_field: int = 0, when_field: int = 1,
                 threshold_field: int = 2):
        for name, f in (("value_field", value_field), ("id_field", id_field),
                        ("when_field", when_field), ("threshold_field", threshold_field)):
            if isinstance(f, bool) or not isinstance(f, int) or f < 0:
                raise ValueError(f"RuleSetAlert: {name} is a non-negative int, got {f!r}")
        self.value_field, self.id_field = value_field, id_field
        self.when_field, self.threshold_field = when_field, threshold_field
        self.native = ("ruleset", value_field, id_field, when_field, threshold_field)

    @staticmethod
    def _number(x, what: str):
        if isinstance(x, bool) or not isinstance(x, (int, float)):
            raise TypeError(f"RuleSetAlert: {what} must be an int or a float, got {x!r}")
        return x

    def parse_rule(self, rule):
        """``(id, when, threshold)`` of a broadcast element, validated."""
        rid, when = rule[self.id_field], rule[self.when_field]
        if isinstance(rid, bool) or not isinstance(rid, int):
            raise TypeError(f"RuleSetAlert: the rule id must be an int, got {rid!r}")
        if when is not None and (not isinstance(when, str) or when not in _LOOKUP_WHENS):
            raise ValueError("RuleSetAlert: when must be one of '>', '>=', '<', '<=', '==', '!=' "
                             f"or None, got {when!r}")
        return rid, when, self._number(rule[self.threshold_field], "the rule's threshold")

    def process_broadcast_element(self, rule, ctx, out):
        rid, when, threshold = self.parse_rule(rule)
        state = ctx.get_broadcast_state(self.DESCRIPTOR)
        if when is None:
            state.remove(rid)
        else:
            state.put(rid, (when, threshold))

    def process_element(self, sample, ctx, out):
        from .tuples import Tuple4

        rules = ctx.get_broadcast_state(self.DESCRIPTOR).immutable_entries()
        if not rules:
            return
        v = self._number(sample[self.value_field], "the sample's value")
        key = ctx.get_current_key()
        for rid, (when, threshold) in sorted(rules, key=lambda e: e[0]):
            # Python compares an int with a float exactly; Java compares the two doubles
            if _LOOKUP_WHENS[when](float(v), float(threshold)):
                out.collect(Tuple4(key, v, rid, threshold))


class CountWithTimeout(KeyedProcessFunction):
    """Per-key element count with an event-time timeout (the ``CountWithTimeoutFunction`` of
    Flink's ProcessFunction documentation): every element adds one to its key's count, stores its
    timestamp as the key's `last` (the last arrival, not the largest timestamp) and registers an
    event-time timer at ``last + timeout``; the timer that still finds ``last + timeout`` equal to
    its own time -- no element has arrived for `timeout` -- collects
    ``Tuple3(key, count, last)`` stamped with the timer's time. The state is kept: the count is
    the key's total, and a later element arms the key again. `timeout` is a positive int
    (milliseconds) or a ``Time``. A host that has stopped reporting:

        samples.key_by(0).process(CountWithTimeout(Time.seconds(60)))

    The planner runs exactly this class (not a subclass) with a positional key on the device
    timer operator (runtime/timeout_operator.py); these methods are the exact host
    implementation used otherwise."""

    def __init__(self, timeout):
        from .time import Time

        ms = timeout.to_milliseconds() if isinstance(timeout, Time) else timeout
        if isinstance(ms, bool) or not isinstance(ms, int) or ms <= 0:
            raise ValueError("CountWithTimeout: timeout is a positive int (milliseconds) or a "
                             f"Time, got {timeout!r}")
        self.timeout = ms
        self.native = ("count_timeout", ms)

    def open(self, parameters=None):
        from .state import ValueStateDescriptor

        self._state = self.get_runtime_context().get_state(
            ValueStateDescriptor("count-with-timeout"))

    def process_element(self, value, ctx, out):
        ts = ctx.timestamp()
        if ts is None:
            raise ValueError("CountWithTimeout: a record without an event timestamp")
        cur = self._state.value()
        self._state.update(((cur[0] if cur is not None else 0) + 1, ts))
        ctx.timer_service().register_event_time_timer(ts + self.timeout)

    def on_timer(self, timestamp, ctx, out):
        from .tuples import Tuple3

        cur = self._state.value()
        if cur is not None and timestamp == cur[1] + self.timeout:
            out.collect(Tuple3(ctx.get_current_key(), cur[0], cur[1]))


class SustainedAlert(KeyedProcessFunction):
    """A condition that has held for a duration (the ``for:`` of a Prometheus alerting rule):
    ``value[field] <when> threshold`` is evaluated for every element of a key, in arrival order.
    The first element of an uninterrupted run of breaching elements stamps the run's `since`;
    the first element of the run with ``ts - since >= for_`` collects
    ``Tuple4(key, 1, since, value[field])``, once per run; the first element that does not breach
    after that collects ``Tuple4(key, 0, since, value[field])`` and closes the run. A run that
    ends before it fired leaves no trace. Output records carry their element's timestamp; there
    are no timers. `when` is one of ``">", ">=", "<", "<=", "==", "!="``; values are int or float
    (not bool) and compare as Java compares doubles (a NaN on either side is false for every
    operator but ``!=``). `for_` is an int >= 0 (milliseconds) or a ``Time``; 0 reports every
    run at its first element. A host that has been above 90 % for five minutes:

        samples.key_by(0).process(SustainedAlert(2, ">", 90.0, Time.minutes(5)))

    The planner runs exactly this class (not a subclass) with a positional key on the device
    operator (runtime/sustain_operator.py); these methods are the exact host implementation used
    otherwise."""

    def __init__(self, field: int, when: str, threshold, for_):
        from .time import Time

        if isinstance(field, bool) or not isinstance(field, int) or field < 0:
            raise ValueError(f"SustainedAlert: field is a non-negative int, got {field!r}")
        if not isinstance(when, str) or when not in _LOOKUP_WHENS:
            raise ValueError("SustainedAlert: when must be one of '>', '>=', '<', '<=', '==', "
                             f"'!=', got {when!r}")
        self._number(threshold, "threshold")
        ms = for_.to_milliseconds() if isinstance(for_, Time) else for_
        if isinstance(ms, bool) or not isinstance(ms, int) or ms < 0:
            raise ValueError("SustainedAlert: for_ is an int >= 0 (milliseconds) or a Time, "
                             f"got {for_!r}")
        self.field, self.when, self.threshold, self.for_ms = field, when, threshold, ms
        self.native = ("sustained", field, when, threshold, ms)

    @staticmethod
    def _number(x, what: str):
        if isinstance(x, bool) or not isinstance(x, (int, float)):
            raise TypeError(f"SustainedAlert: {what} must be an int or a float, got {x!r}")
        return x

    def open(self, parameters=None):
        from .state import ValueStateDescriptor

        self._state = self.get_runtime_context().get_state(
            ValueStateDescriptor("sustained-alert"))

    def process_element(self, value, ctx, out):
        from .tuples import Tuple4

        ts = ctx.timestamp()
        if ts is None:
            raise ValueError("SustainedAlert: a record without an event timestamp")
        v = self._number(value[self.field], "the element's value")
        cur = self._state.value()
        # Python compares an int with a float exactly; Java compares the two doubles
        if _LOOKUP_WHENS[self.when](float(v), float(self.threshold)):
            since, firing = cur if cur is not None else (ts, False)
            if not firing and ts - since >= self.for_ms:
                firing = True
                out.collect(Tuple4(ctx.get_current_key(), 1, since, v))
            self._state.update((since, firing))
        else:
            if cur is not None and cur[1]:
                out.collect(Tuple4(ctx.get_current_key(), 0, cur[0], v))
            self._state.clear()


class BurstAlert(KeyedProcessFunction):
    """N breaches within T (the ``times(N).within(T)`` of a CEP pattern, fail2ban's ``maxretry`` /
    ``findtime``, a flapping host): ``value[field] <when> threshold`` is evaluated for every
    element of a key, in arrival order, and the timestamps of the key's `times` most recent
    breaching elements are kept. An element is dense when `times` of them are held and the
    oldest lies at most `within` before the element's timestamp (a negative difference, disorder,
    is dense). The first dense breach collects ``Tuple4(key, 1, since, value[field])`` with
    `since` the oldest held breach, once per burst; the first element after that which is not
    dense, breaching or not, collects ``Tuple4(key, 0, since, value[field])`` and ends the burst.
    Output records carry their element's timestamp. There are no timers: a burst that simply
    stops resolves at the key's next element, whenever that arrives (``CountWithTimeout``
    reports silence). `when`, the values and the comparison are ``SustainedAlert``'s; `times` is
    an int >= 2; `within` is an int >= 0 (milliseconds) or a ``Time``, below 2**62. Five errors
    within ten seconds:

        events.key_by(0).process(BurstAlert(2, ">=", 500, 5, Time.seconds(10)))

    The planner runs exactly this class (not a subclass) with a positional key and
    ``times <= 16`` on the device operator (runtime/burst_operator.py); these methods are the
    exact host implementation used otherwise."""

    def __init__(self, field: int, when: str, threshold, times: int, within):
        from .time import Time

        if isinstance(field, bool) or not isinstance(field, int) or field < 0:
            raise ValueError(f"BurstAlert: field is a non-negative int, got {field!r}")
        if not isinstance(when, str) or when not in _LOOKUP_WHENS:
            raise ValueError("BurstAlert: when must be one of '>', '>=', '<', '<=', '==', "
                             f"'!=', got {when!r}")
        self._number(threshold, "threshold")
        if isinstance(times, bool) or not isinstance(times, int) or times < 2:
            raise ValueError(f"BurstAlert: times is an int >= 2, got {times!r}")
        ms = within.to_milliseconds() if isinstance(within, Time) else within
        if isinstance(ms, bool) or not isinstance(ms, int) or not 0 <= ms < 1 << 62:
            raise ValueError("BurstAlert: within is an int >= 0 (milliseconds) or a Time, below "
                             f"2**62, got {within!r}")
        self.field, self.when, self.threshold = field, when, threshold
        self.times, self.within_ms = times, ms
        self.native = ("burst", field, when, threshold, times, ms)

    @staticmethod
    def _number(x, what: str):
        if isinstance(x, bool) or not isinstance(x, (int, float)):
            raise TypeError(f"BurstAlert: {what} must be an int or a float, got {x!r}")
        return x

    def open(self, parameters=None):
        from .state import ValueStateDescriptor

        self._state = self.get_runtime_context().get_state(ValueStateDescriptor("burst-alert"))

    def process_element(self, value, ctx, out):
        from .tuples import Tuple4

        ts = ctx.timestamp()
        if ts is None:
            raise ValueError("BurstAlert: a record without an event timestamp")
        v = self._number(value[self.field], "the element's value")
        recent, since, firing = self._state.value() or ((), None, False)
        # Python compares an int with a float exactly; Java compares the two doubles
        breach = _LOOKUP_WHENS[self.when](float(v), float(self.threshold))
        if breach:
            recent = (recent + (ts,))[-self.times:]
        dense = len(recent) == self.times and ts - recent[0] <= self.within_ms
        if breach and dense and not firing:
            firing, since = True, recent[0]
            out.collect(Tuple4(ctx.get_current_key(), 1, since, v))
        elif not dense and firing:
            out.collect(Tuple4(ctx.get_current_key(), 0, since, v))
            firing, since = False, None
        if recent:
            self._state.update((recent, since, firing))


class StateMachineAlert(KeyedProcessFunction):
    """A finite state machine per key, stepped by every element (Flink's StateMachineExample; a
    warning / critical / ok severity reported once per change; hysteresis; "three breaches in a
    row"): ``value[field]`` falls into class ``c`` = the number of `bounds` ``b`` with
    ``value >= b``, and the key moves ``to = table[from][c]``. A key enters `initial` at its
    first element, which then steps it like any other. Every reported pair ``(from, to)``
    collects ``Tuple5(key, from, to, since, value[field])``, `since` being the timestamp at which
    the key entered `from` (``ts - since`` is how long it stayed). Elements are taken in arrival
    order, output records carry their element's timestamp, and there are no timers. Values are
    int or float (not bool) and compare as Java compares doubles: a NaN is class 0 and
    ``-0.0 >= 0.0`` holds. `bounds` holds 1 to 15 finite ints or floats, strictly ascending;
    `table` has one row per state and one entry per class (``len(bounds) + 1``), each a state;
    `report` is ``"change"`` (every pair with ``from != to``) or an iterable of ``(from, to)``
    pairs, self-loops allowed, possibly empty. An integer event type ``e`` in ``[0, C)`` is its
    own class with ``bounds = [1, 2, .., C - 1]``. On above 90, off only below 80:

        samples.key_by(0).process(StateMachineAlert(2, [80.0, 90.0], [[0, 0, 1], [0, 1, 1]]))

    The planner runs exactly this class (not a subclass) with a positional key and at most 16
    states on the device operator (runtime/fsm_operator.py); these methods are the exact host
    implementation used otherwise."""

    def __init__(self, field: int, bounds, table, initial: int = 0, report="change"):
        import math

        def is_int(x):
            return isinstance(x, int) and not isinstance(x, bool)

        if not is_int(field) or field < 0:
            raise ValueError(f"StateMachineAlert: field is a non-negative int, got {field!r}")
        try:
            bounds = tuple(bounds)
        except TypeError:
            raise TypeError(f"StateMachineAlert: bounds is a sequence of numbers, got {bounds!r}") \
                from None
        for b in bounds:
            self._number(b, "a bound")
        if not 1 <= len(bounds) <= 15:
            raise ValueError(f"StateMachineAlert: 1 to 15 bounds, got {len(bounds)}")
        try:
            cuts = tuple(float(b) for b in bounds)
        except OverflowError:
            raise ValueError("StateMachineAlert: the bounds must be finite") from None
        if not all(math.isfinite(c) for c in cuts) or any(a >= b for a, b in zip(cuts, cuts[1:])):
            raise ValueError("StateMachineAlert: the bounds must be finite and strictly "
                             f"ascending, got {bounds!r}")
        try:
            table = tuple(tuple(row) for row in table)
        except TypeError:
            raise TypeError("StateMachineAlert: table is a sequence of rows of states, got "
                            f"{table!r}") from None
        states, classes = len(table), len(cuts) + 1
        if states < 1:
            raise ValueError("StateMachineAlert: the table needs at least one state")
        for s, row in enumerate(table):
            if len(row) != classes:
                raise ValueError(f"StateMachineAlert: table[{s}] needs one entry per class "
                                 f"({classes}), got {len(row)}")
            for to in row:
                if not is_int(to) or not 0 <= to < states:
                    raise ValueError(f"StateMachineAlert: table[{s}] holds {to!r}, no state in "
                                     f"[0, {states})")
        if not is_int(initial) or not 0 <= initial < states:
            raise ValueError(f"StateMachineAlert: initial is a state in [0, {states}), got "
                             f"{initial!r}")
        if isinstance(report, str):
            if report != "change":
                raise ValueError("StateMachineAlert: report is 'change' or an iterable of "
                                 f"(from, to) pairs, got {report!r}")
            pairs = {(a, b) for a in range(states) for b in range(states) if a != b}
        else:
            try:
                pairs = {tuple(p) for p in report}
            except TypeError:
                raise TypeError("StateMachineAlert: report is 'change' or an iterable of "
                                f"(from, to) pairs, got {report!r}") from None
            for p in pairs:
                if len(p) != 2 or not all(is_int(x) and 0 <= x < states for x in p):
                    raise ValueError(f"StateMachineAlert: the reported pair {p!r} is no pair of "
                                     f"states in [0, {states})")
        self.field, self.bounds, self.table, self.initial = field, cuts, table, initial
        self.report = tuple(sorted(pairs))
        self._reported = frozenset(pairs)
        # the bounds as the doubles they are compared as: 80 and 80.0 are one rule
        self.native = ("state_machine", field, cuts, table, initial, self.report)

    @staticmethod
    def _number(x, what: str):
        if isinstance(x, bool) or not isinstance(x, (int, float)):
            raise TypeError(f"StateMachineAlert: {what} must be an int or a float, got {x!r}")
        return x

    def open(self, parameters=None):
        from .state import ValueStateDescriptor

        self._state = self.get_runtime_context().get_state(
            ValueStateDescriptor("state-machine-alert"))

    def process_element(self, value, ctx, out):
        from .tuples import Tuple5

        ts = ctx.timestamp()
        if ts is None:
            raise ValueError("StateMachineAlert: a record without an event timestamp")
        v = self._number(value[self.field], "the element's value")
        since, state = self._state.value() or (ts, self.initial)
        # Python compares an int with a float exactly; Java compares the two doubles
        x = float(v)
        to = self.table[state][sum(x >= b for b in self.bounds)]
        if (state, to) in self._reported:
            out.collect(Tuple5(ctx.get_current_key(), state, to, since, v))
        if to != state:
            since = ts
        self._state.update((since, to))


class CounterRate(KeyedProcessFunction):
    """The rate and the increase of a cumulative counter (Prometheus' ``irate()`` /
    ``increase()``): interface octets, request totals and ``/proc/net/dev`` only mean something
    as the difference between two consecutive samples of a key, and restart at zero with their
    process. Per key the last accepted sample ``(ts, value[field])`` is kept; a key's first
    element is only stored. An element with ``ts <= `` the stored one (a duplicate or a
    straggler) is ignored and counted in ``out_of_order``. Any other element gives
    ``dt = ts - last_ts``, ``inc = v - last if v >= last else v`` (a smaller reading is a counter
    reset: the new reading is the increase) and becomes the stored sample; unless
    ``dt > max_gap`` (the key is re-based silently) it collects
    ``Tuple4(key, rate, inc, dt)`` with ``rate = float(inc) * per / dt``, `per` in
    milliseconds, when there is no rule or ``rate <when> threshold`` holds. A key's counter is
    all ints (Java longs: the subtraction wraps to 64 bits) or all floats (a NaN makes ``>=``
    false, so ``inc = v``); `inc` is of the counter's kind. The comparison is Java's on two
    doubles: a NaN is false for every operator but ``!=``. Output records carry their element's
    timestamp; there are no timers. `per` is an int >= 1 (milliseconds) or a ``Time``, `max_gap`
    None or such a duration below 2**62, `when` one of ``">", ">=", "<", "<=", "==", "!="`` and
    given together with `threshold`. Bytes per second from raw interface counters, and the
    hosts below 100 Mbit/s:

        samples.key_by(0).process(CounterRate(2))
        samples.key_by(0).process(CounterRate(2, per=Time.seconds(1), when="<",
                                              threshold=100e6 / 8, max_gap=Time.minutes(2)))

    The planner runs exactly this class (not a subclass) with a positional key on the device
    operator (runtime/rate_operator.py); these methods are the exact host implementation used
    otherwise."""

    def __init__(self, field: int, per=1000, when=None, threshold=None, max_gap=None):
        from .time import Time

        if isinstance(field, bool) or not isinstance(field, int) or field < 0:
            raise ValueError(f"CounterRate: field is a non-negative int, got {field!r}")
        ms = per.to_milliseconds() if isinstance(per, Time) else per
        if isinstance(ms, bool) or not isinstance(ms, int) or not 1 <= ms < 1 << 63:
            raise ValueError("CounterRate: per is an int >= 1 (milliseconds) or a Time, "
                             f"got {per!r}")
        gap = max_gap.to_milliseconds() if isinstance(max_gap, Time) else max_gap
        if gap is not None and (isinstance(gap, bool) or not isinstance(gap, int)
                                or not 1 <= gap < 1 << 62):
            raise ValueError("CounterRate: max_gap is None, an int >= 1 (milliseconds) or a "
                             f"Time, below 2**62, got {max_gap!r}")
        if when is None:
            if threshold is not None:
                raise ValueError("CounterRate: a threshold without when")
        else:
            if not isinstance(when, str) or when not in _LOOKUP_WHENS:
                raise ValueError("CounterRate: when must be one of '>', '>=', '<', '<=', '==', "
                                 f"'!=' or None, got {when!r}")
            if threshold is None:
                raise ValueError("CounterRate: when without a threshold")
            self._number(threshold, "threshold")
        self.field, self.per_ms, self.when, self.threshold = field, ms, when, threshold
        self.max_gap_ms = gap
        self.out_of_order = 0
        self.native = ("counter_rate", field, ms, when, threshold, gap)

    @staticmethod
    def _number(x, what: str):
        if isinstance(x, bool) or not isinstance(x, (int, float)):
            raise TypeError(f"CounterRate: {what} must be an int or a float, got {x!r}")
        if isinstance(x, int) and not -(1 << 63) <= x < 1 << 63:
            raise TypeError(f"CounterRate: {what} is an int beyond 64 bits, got {x!r}")
        return x

    def open(self, parameters=None):
        from .state import ValueStateDescriptor

        self._state = self.get_runtime_context().get_state(ValueStateDescriptor("counter-rate"))

    def process_element(self, value, ctx, out):
        from .tuples import Tuple4

        ts = ctx.timestamp()
        if ts is None:
            raise ValueError("CounterRate: a record without an event timestamp")
        v = self._number(value[self.field], "the element's value")
        cur = self._state.value()
        if cur is None:
            self._state.update((ts, v))
            return
        last_ts, last = cur
        if isinstance(v, float) != isinstance(last, float):
            raise TypeError("CounterRate: a key's counter is all ints or all floats, got "
                            f"{v!r} after {last!r}")
        if ts <= last_ts:
            self.out_of_order += 1
            return
        dt = ts - last_ts
        if v >= last:
            inc = v - last
            if isinstance(inc, int):
                inc = (inc + (1 << 63)) % (1 << 64) - (1 << 63)  # Java's long subtraction
        else:
            inc = v
        self._state.update((ts, v))
        if self.max_gap_ms is not None and dt > self.max_gap_ms:
            return
        rate = float(inc) * float(self.per_ms) / float(dt)
        if self.when is None or _LOOKUP_WHENS[self.when](rate, float(self.threshold)):
            out.collect(Tuple4(ctx.get_current_key(), rate, inc, dt))


class _NoTimerService:
    """What a function wrapped by EventTimeOrdered finds in place of the timer service."""

    def __getattr__(self, name):
        raise RuntimeError("EventTimeOrdered: the wrapped function may not use the timer service "
                           f"({name})")


class _StampedCollector:
    """Collects into `out` with the element's timestamp, where `out` can keep one."""

    def __init__(self, out, ts):
        self._out, self._ts = out, ts

    def collect(self, value):
        if hasattr(self._out, "collect_at"):
            self._out.collect_at(value, self._ts)
        else:
            self._out.collect(value)


class EventTimeOrdered(KeyedProcessFunction):
    """Event-time order in front of a keyed rule: the elements of a key are buffered, and when
    the watermark reaches an element's timestamp it is handed to ``fn.process_element`` -- a
    key's elements in (timestamp, arrival) order, whatever order they arrived in. An element
    whose timestamp is at or behind the watermark when it arrives is late: it is dropped and
    counted in ``late_dropped`` (there is no side output). Output records carry their element's
    timestamp, as the rules' rows do. Per key the result is `fn` applied to the key's elements
    that are not late, sorted by (timestamp, arrival). `fn` is a ``KeyedProcessFunction`` that
    does not override ``on_timer`` and does not use the timer service. A rule that must not be
    fooled by a straggler:

        samples.key_by(0).process(EventTimeOrdered(SustainedAlert(2, ">", 90.0, Time.minutes(5))))

    The planner runs exactly this class around exactly a ``SustainedAlert``, a ``BurstAlert``
    (``times <= 16``), a ``StateMachineAlert`` (at most 16 states) or a ``CounterRate`` (whose
    ``out_of_order`` then counts only equal timestamps) with a positional key on
    the device reorder buffer
    (runtime/reorder_operator.py) in front of the rule's device operator; these methods are the
    exact host implementation used otherwise."""

    def __init__(self, fn):
        if not isinstance(fn, KeyedProcessFunction) \
                or type(fn).on_timer is not ProcessFunction.on_timer:
            raise ValueError("EventTimeOrdered: fn is a KeyedProcessFunction that does not "
                             f"override on_timer, got {fn!r}")
        self.fn = fn
        self.late_dropped = 0
        if hasattr(fn, "native"):
            self.native = ("event_time_ordered",) + tuple(fn.native)

    def open(self, parameters=None):
        from .state import ValueStateDescriptor

        ctx = self.get_runtime_context()
        self.fn.set_runtime_context(ctx)
        self.fn.open(parameters)
        # (the key's next arrival number, its buffered (ts, seq, value) entries)
        self._state = ctx.get_state(ValueStateDescriptor("event-time-ordered"))

    def process_element(self, value, ctx, out):
        ts = ctx.timestamp()
        if ts is None:
            raise ValueError("EventTimeOrdered: a record without an event timestamp")
        timers = ctx.timer_service()
        if ts <= timers.current_watermark():
            self.late_dropped += 1
            return
        seq, entries = self._state.value() or (0, [])
        self._state.update((seq + 1, entries + [(ts, seq, value)]))
        timers.register_event_time_timer(ts)

    def on_timer(self, timestamp, ctx, out):
        cur = self._state.value()
        if cur is None:
            return
        seq, entries = cur
        due = sorted((e for e in entries if e[0] <= timestamp), key=lambda e: e[:2])
        if not due:
            return
        rest = [e for e in entries if e[0] > timestamp]
        # the arrival counter goes with the buffer: an empty one starts over
        if rest:
            self._state.update((seq, rest))
        else:
            self._state.clear()
        key, side = ctx.get_current_key(), getattr(ctx, "_side", None)
        for ts, _, value in due:
            c = ProcessFunction.Context(ts, _NoTimerService(), side, key)
            self.fn.process_element(value, c, _StampedCollector(out, ts))


class SinkFunction(Function):
    def invoke(self, value, context=None):
        raise NotImplementedError


class RichSinkFunction(RichFunction, SinkFunction):
    pass


class SourceFunction(Function):
    """run(ctx) calls ctx.collect(...) / ctx.collect_with_timestamp(...) / ctx.emit_watermark."""

    def run(self, ctx):
        raise NotImplementedError

    def cancel(self):
        pass


def call_map(fn, v):
    if isinstance(fn, MapFunction):
        return fn.map(v)
    return fn(v)


def call_filter(fn, v) -> bool:
    if isinstance(fn, FilterFunction):
        return bool(fn.filter(v))
    return bool(fn(v))


def call_reduce(fn, a, b):
    if isinstance(fn, ReduceFunction):
        return fn.reduce(a, b)
    return fn(a, b)


def call_key(fn, v):
    if isinstance(fn, KeySelector):
        return fn.get_key(v)
    return fn(v)


Any_ = Any
