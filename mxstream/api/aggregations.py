"""Builtin AggregateFunctions (and two ProcessWindowFunctions, WindowQuantiles and
WindowDistinctCount) that the planner can run natively.

Each behaves exactly like the equivalent hand-written Flink AggregateFunction on the host path
(e.g. ``AvgAggregate(1)`` is ComputeCpuAvg.java:31-58: accumulator (count, sum), result
``sum / count`` or 0.0) and carries a ``native`` descriptor (kind, field) for the GPU/C++ path.
"""
from __future__ import annotations

import struct

from ..ops.kernels import MAX_QUANTILES, PPM_ONE
from .functions import AggregateFunction, ProcessWindowFunction
from .tuples import Tuple


class BuiltinAggregate(AggregateFunction):
    native: tuple[str, int]


class SumAggregate(BuiltinAggregate):
    def __init__(self, field: int):
        self.field = field
        self.native = ("sum", field)

    def create_accumulator(self):
        return None

    def add(self, value, acc):
        x = value[self.field]
        return x if acc is None else acc + x

    def get_result(self, acc):
        return acc

    def merge(self, a, b):
        return b if a is None else (a if b is None else a + b)


class CountAggregate(BuiltinAggregate):
    def __init__(self, field: int = 0):
        self.native = ("count", field)

    def create_accumulator(self):
        return 0

    def add(self, value, acc):
        return acc + 1

    def get_result(self, acc):
        return acc

    def merge(self, a, b):
        return a + b


class AvgAggregate(BuiltinAggregate):
    """Tuple2<Integer count, Double sum> accumulator; result sum/count (0.0 when empty)."""

    def __init__(self, field: int):
        self.field = field
        self.native = ("avg", field)

    def create_accumulator(self):
        return (0, 0.0)

    def add(self, value, acc):
        return (acc[0] + 1, acc[1] + value[self.field])

    def get_result(self, acc):
        return 0.0 if acc[0] == 0 else acc[1] / acc[0]

    def merge(self, a, b):
        return (a[0] + b[0], a[1] + b[1])


class MinAggregate(BuiltinAggregate):
    def __init__(self, field: int):
        self.field = field
        self.native = ("min", field)

    def create_accumulator(self):
        return None

    def add(self, value, acc):
        x = value[self.field]
        return x if acc is None or x < acc else acc

    def get_result(self, acc):
        return acc

    def merge(self, a, b):
        if a is None:
            return b
        if b is None:
            return a
        return a if a <= b else b


class MaxAggregate(MinAggregate):
    def __init__(self, field: int):
        self.field = field
        self.native = ("max", field)

    def add(self, value, acc):
        x = value[self.field]
        return x if acc is None or x > acc else acc

    def merge(self, a, b):
        if a is None:
            return b
        if b is None:
            return a
        return a if a >= b else b


class VectorSumAggregate(BuiltinAggregate):
    """Element-wise sum of a metric-vector field (list/tuple of floats, e.g. one usage value
    per CPU core). Host path: a list accumulator; native path: the MFMA vector-window kernel
    (runtime/vector_window_operator.py). The result is a list of floats."""

    kind = "vsum"

    def __init__(self, field: int):
        self.field = field
        self.native = (self.kind, field)

    def create_accumulator(self):
        return (0, None)

    def add(self, value, acc):
        x = [float(v) for v in value[self.field]]
        n, s = acc
        if s is None:
            return (n + 1, x)
        if len(x) != len(s):
            raise ValueError("metric vectors of one key must have the same length")
        return (n + 1, [a + b for a, b in zip(s, x)])

    def get_result(self, acc):
        return [] if acc[1] is None else list(acc[1])

    def merge(self, a, b):
        if a[1] is None:
            return b
        if b[1] is None:
            return a
        return (a[0] + b[0], [x + y for x, y in zip(a[1], b[1])])


class VectorAvgAggregate(VectorSumAggregate):
    """Element-wise average of a metric-vector field (ComputeCpuAvg.java:31-58 per vector
    component: accumulator (count, sums), result sums / count)."""

    kind = "vavg"

    def get_result(self, acc):
        n, s = acc
        return [] if s is None else [v / n for v in s]


def _double_order(x: float) -> int:
    """Sort key of a double in Java ``Double.compare`` order (-0.0 < 0.0, NaN last): the order
    bits of csrc/mxs_common.h f64_order_bits."""
    if x != x:
        return (1 << 64) - 1
    b = struct.unpack("<Q", struct.pack("<d", x))[0]
    return b ^ ((1 << 64) - 1) if b >> 63 else b | (1 << 63)


def quantile_rank(n: int, ppm: int) -> int:
    """Nearest rank: the index into n >= 1 ascending values of quantile `ppm` (parts per
    million), ``clamp(ceil(n * ppm / 1e6) - 1, 0, n - 1)`` in integers."""
    return min(max((n * ppm + PPM_ONE - 1) // PPM_ONE - 1, 0), n - 1)


class WindowQuantiles(ProcessWindowFunction):
    """Per key and window, the nearest-rank quantiles of one field: ``process`` emits one
    ``Tuple(key, x_1, ..., x_Q)`` whose x_j is the window's element at sorted index
    ``quantile_rank(n, ppm_j)`` -- the element itself, never an interpolation; 0.0 is the
    minimum, 1.0 the maximum. 1 to 8 quantiles in [0, 1], duplicates and any order allowed.

    Each quantile becomes an integer here, once: ``ppm = round(q * 1_000_000)``. ``native``
    hands (field, ppm) to the planner, which runs tumbling and sliding event-time windows on
    the device list-window operator (one staged copy of a key's values serves all Q ranks);
    this method is the exact host implementation used otherwise."""

    def __init__(self, field: int, quantiles):
        qs = list(quantiles)
        if not 1 <= len(qs) <= MAX_QUANTILES:
            raise ValueError(f"WindowQuantiles takes 1 to {MAX_QUANTILES} quantiles, got {len(qs)}")
        for q in qs:
            if isinstance(q, bool) or not isinstance(q, (int, float)) or not 0 <= q <= 1:
                raise ValueError(f"a quantile is a real number in [0, 1], got {q!r}")
        self.field = field
        self.ppm = tuple(int(round(q * PPM_ONE)) for q in qs)
        self.native = ("quantiles", field, self.ppm)

    def process(self, key, context, elements, out):
        values = [t[self.field] for t in elements]
        if all(isinstance(v, float) for v in values):
            values.sort(key=_double_order)
        else:
            values.sort()
        n = len(values)
        out.collect(Tuple([key] + [values[quantile_rank(n, p)] if n else 0.0 for p in self.ppm]))


class WindowTopN(ProcessWindowFunction):
    """The n elements of a ``window_all`` window with the largest (``largest=False``: smallest)
    value in `field`, emitted unchanged in rank order -- "which 10 hosts used the most bandwidth
    this minute" as ``key_by(host).time_window(..).sum(bytes)`` followed by
    ``time_window_all(..).process(WindowTopN(1, 10))``.

    Order: by `field` (integers by value, doubles in Java ``Double.compare`` order: -0.0 < 0.0,
    NaN largest), best first; equal values by `tie_field` ascending in the natural order of the
    Python object (``int``, or ``str``); then by arrival. ``rank`` is that order and this method
    the exact host implementation. ``native`` lets the planner fold the cut into the keyed
    window operator upstream (its ``top_n``): the device then emits only the rows at or above
    the n-th best value of each firing -- every row that ties there included, so the device
    never breaks a tie -- and the operator applies ``rank`` to those candidates."""

    def __init__(self, field: int, n: int, largest: bool = True, tie_field: int = 0):
        if isinstance(n, bool) or not isinstance(n, int) or n < 1:
            raise ValueError(f"WindowTopN: n is an int >= 1, got {n!r}")
        for name, f in (("field", field), ("tie_field", tie_field)):
            if isinstance(f, bool) or not isinstance(f, int) or f < 0:
                raise ValueError(f"WindowTopN: {name} is a non-negative int, got {f!r}")
        if field == tie_field:
            raise ValueError("WindowTopN: field and tie_field must differ")
        self.field, self.n, self.largest, self.tie_field = field, n, bool(largest), tie_field
        self.native = ("topn", field, n, self.largest, tie_field)

    def rank(self, elements) -> list:
        """The first n of `elements` in rank order."""
        elems = list(elements)
        vals = [e[self.field] for e in elems]
        for v in vals:
            if isinstance(v, bool) or not isinstance(v, (int, float)):
                raise TypeError(f"WindowTopN: field {self.field} must be numeric, got {v!r}")
        if all(isinstance(v, int) for v in vals):
            words = vals
        else:
            words = [_double_order(float(v)) for v in vals]
        sign = -1 if self.largest else 1
        order = sorted(range(len(elems)),
                       key=lambda i: (sign * words[i], elems[i][self.tie_field], i))
        return [elems[i] for i in order[:self.n]]

    def process(self, key, context, elements, out):
        for e in self.rank(elements):
            out.collect(e)


class WindowDistinctCount(ProcessWindowFunction):
    """Per key and window, the number of different values of one field: ``process`` emits one
    ``Tuple(key, count)``, the count a Python int (Java prints the Long: ``(host1,42)``). The
    count is exact, never a sketch.

    Equality is Java's ``equals`` of the boxed value: doubles by ``Double.equals`` (the order
    bits of ``_double_order``: every NaN is one value, -0.0 and 0.0 are two), everything else by
    Python equality, and an int never equals a float (a ``Long`` is no ``Double``).

    ``native`` hands the field to the planner, which runs tumbling and sliding event-time
    windows on the device list-window operator (a hash set per key over the pane arena; float
    fields, and int fields up to 2**53 in magnitude); this method is the exact host
    implementation used otherwise."""

    def __init__(self, field: int):
        if isinstance(field, bool) or not isinstance(field, int) or field < 0:
            raise ValueError(f"WindowDistinctCount takes a field index >= 0, got {field!r}")
        self.field = field
        self.native = ("distinct", field)

    def process(self, key, context, elements, out):
        seen = set()
        for t in elements:
            v = t[self.field]
            # the tag keeps 1 and 1.0 (equal in Python) apart
            seen.add(("double", _double_order(v)) if isinstance(v, float) else ("object", v))
        out.collect(Tuple([key, len(seen)]))
