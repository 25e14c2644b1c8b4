"""Burst alerts (``stream.key_by(k).process(BurstAlert(field, when, threshold, times, within))``).

A key is reported once, ``(key, 1, since, value)``, at the breach of ``value <when> threshold``
whose `times` most recent breaches (itself included) lie within `within` ms of it, `since` being
the oldest of them; and once more, ``(key, 0, since, value)``, at the first element of the key,
breaching or not, for which they no longer do. Elements are taken in arrival order; there are no
timers, the rule is evaluated when a sample arrives.

State for dense key ids (the operator's dictionary ids for string keys, an integer key itself --
a key at or above ``dense_limit`` is refused): ``ring int64[cap, times]``, a circular buffer of
the key's last breaches, and ``row int64[cap, 2]`` = (since, meta), meta = firing | held << 1 |
pos << 8 (csrc/mxs_burst.h). The capacity doubles to cover a batch's largest key id.

``process`` is one ``burst_update``: a stable radix sort by key, the look-back and one segmented
wave scan of the transition (csrc/mxs_burst.h has the algebra), the transitions' count read back
and the rows put in arrival order. CPU (device="cpu") runs the C++ twin (csrc/burst_cpu.cpp).
"""
from __future__ import annotations

import numpy as np
import torch

from ..ops import kernels as K
from .sustain_operator import threshold_bits
from .window_operator import OperatorMetrics


def unpack(ring, row):
    """The state as host arrays, independent of the ring's rotation: (since, firing, held,
    recent int64[cap, times]) with a key's held breaches oldest first and unused entries 0."""
    ring, row = (np.ascontiguousarray(x.cpu().numpy()) for x in (ring, row))
    times = ring.shape[1]
    meta = row[:, 1]
    held = (meta >> K.BURST_HELD_SHIFT) & 0x7f
    pos = meta >> K.BURST_POS_SHIFT
    j = np.arange(times, dtype=np.int64)[None, :]
    recent = np.take_along_axis(ring, (pos[:, None] - held[:, None] + j) % times, axis=1)
    recent[j >= held[:, None]] = 0
    return row[:, 0].copy(), meta & 1, held, recent


class KeyedBurstOperator:
    def __init__(self, when, threshold, times: int, within_ms: int, device="cpu",
                 dense_limit: int = 1 << 26, capacity: int = 1024):
        if K.lookup_when(when) == 0:
            raise ValueError("when must be one of '>', '>=', '<', '<=', '==', '!='")
        if isinstance(threshold, bool) or not isinstance(threshold, (int, float)):
            raise TypeError(f"threshold must be an int or a float, got {threshold!r}")
        if isinstance(times, bool) or not isinstance(times, int) \
                or not 2 <= times <= K.BURST_MAX_TIMES:
            raise ValueError(f"times must be an int in [2, {K.BURST_MAX_TIMES}], got {times!r}")
        if isinstance(within_ms, bool) or not isinstance(within_ms, int) \
                or not 0 <= within_ms < K.SUSTAIN_TS_LIMIT:
            raise ValueError("within_ms must be an int in [0, 2**62) (milliseconds), got "
                             f"{within_ms!r}")
        self.when, self.threshold, self.times, self.within_ms = when, threshold, times, within_ms
        self.tbits = threshold_bits(threshold)
        self.device = K.resolve_device(device)
        self.dense_limit = int(dense_limit)
        if self.dense_limit < 1:
            raise ValueError("dense_limit must be >= 1")
        self.ring, self.row = K.burst_table(max(1, min(int(capacity), self.dense_limit)), times,
                                            self.device)
        self.metrics = OperatorMetrics()
        self.wm = K.I64_MIN

    @property
    def cap(self) -> int:
        return self.row.shape[0]

    def _grow(self, need: int) -> None:
        old = self.cap
        if need <= old:
            return
        cap = old
        while cap < need:
            cap *= 2
        ring, row = K.burst_table(min(cap, self.dense_limit), self.times, self.device)
        ring[:old].copy_(self.ring)
        row[:old].copy_(self.row)
        self.ring, self.row = ring, row

    # ---- elements ---------------------------------------------------------------------------
    def process(self, keys, vals, ts, is_float: bool = True) -> list:
        """A batch of elements in arrival order: keys int64 ids, vals the value bits (doubles
        when `is_float`, else longs), ts int64 timestamps. [] or one chunk of five device
        columns (key id, code, since, value bits, ts) in arrival order."""
        n = keys.numel()
        for c, name in ((keys, "keys"), (vals, "vals"), (ts, "ts")):
            if c.dtype != torch.int64 or c.dim() != 1 or c.numel() != n:
                raise TypeError(f"{name}: int64 column of the batch's length expected")
            if c.device != self.device:
                raise ValueError(f"{name}: on {c.device}, expected {self.device}")
        if n == 0:
            return []
        lo, hi, tmin, tmax = torch.stack([keys.min(), keys.max(), ts.min(), ts.max()]).tolist()
        if lo < 0 or hi >= self.dense_limit:
            raise TypeError(f"burst: a key outside [0, {self.dense_limit}) is not dense")
        if tmin <= -K.SUSTAIN_TS_LIMIT or tmax >= K.SUSTAIN_TS_LIMIT:
            raise TypeError("burst: a timestamp at or beyond 2**62")
        self.metrics.num_records_in += n
        self._grow(hi + 1)
        cols = K.burst_update(self.ring, self.row, keys.contiguous(), vals.contiguous(),
                              ts.contiguous(),
                              kind=K.SUSTAIN_DOUBLE if is_float else K.SUSTAIN_LONG,
                              when=self.when, threshold_bits=self.tbits, within=self.within_ms,
                              bounds=(hi, tmin, tmax))
        rows = cols[0].numel()
        if rows == 0:
            return []
        self.metrics.num_fires += 1
        self.metrics.num_records_out += rows
        return [cols]

    def advance_watermark(self, wm: int) -> list:
        """The rule has no timers: a watermark is only remembered."""
        self.wm = max(int(wm), self.wm)
        self.metrics.current_watermark = self.wm
        return []

    def entries(self):
        """The keys with any state as host arrays (key id, since, firing, held, recent int64[.,
        times]: the held breaches oldest first, unused entries 0), ascending by key id."""
        since, firing, held, recent = unpack(self.ring, self.row)
        ids = np.nonzero(held)[0].astype(np.int64)
        return ids, since[ids], firing[ids], held[ids], recent[ids]

    # ---- checkpoints ------------------------------------------------------------------------
    def _params(self) -> dict:
        return {"when": self.when, "threshold_bits": self.tbits, "times": self.times,
                "within_ms": self.within_ms}

    def snapshot_state(self):
        from .checkpoint import OperatorSnapshot

        ids, since, firing, held, recent = self.entries()
        kg = (K.keygroups(torch.from_numpy(ids), max_parallelism=128).numpy()
              if ids.size else np.zeros(0, np.int32))
        meta = {"kind": "burst", **self._params(), "wm": self.wm,
                "metrics": {"num_records_in": self.metrics.num_records_in,
                            "num_records_out": self.metrics.num_records_out,
                            "num_fires": self.metrics.num_fires}}
        cols = {"key": ids, "since": since, "firing": firing, "held": held}
        cols.update({f"r{j}": np.ascontiguousarray(recent[:, j]) for j in range(self.times)})
        return OperatorSnapshot(kg, cols, meta)

    def restore_state(self, rows: dict, meta: dict) -> None:
        if meta.get("kind") != "burst" or any(meta.get(k) != v
                                              for k, v in self._params().items()):
            raise ValueError("checkpoint of a different burst-alert function")
        self.wm = meta.get("wm", K.I64_MIN)
        self.metrics.current_watermark = self.wm
        for k, v in meta.get("metrics", {}).items():
            setattr(self.metrics, k, v)
        col = lambda name: np.ascontiguousarray(  # noqa: E731
            rows.get(name, np.zeros(0, np.int64)), dtype=np.int64)
        ids, since, firing, held = col("key"), col("since"), col("firing"), col("held")
        if ids.size and (int(ids.min()) < 0 or int(ids.max()) >= self.dense_limit):
            raise ValueError("checkpoint with a key outside the dense table")
        if held.size and (int(held.min()) < 0 or int(held.max()) > self.times):
            raise ValueError("checkpoint with more breaches than the rule holds")
        cap = self.cap
        while ids.size and cap <= int(ids.max()):
            cap *= 2
        cap = min(cap, self.dense_limit)
        # Key groups arrive in any order; a key has one row, so the order does not matter. The
        # held breaches go to slots 0 .. held - 1, the next one to slot held mod times.
        ring = np.zeros((cap, self.times), dtype=np.int64)
        row = np.zeros((cap, 2), dtype=np.int64)
        for j in range(self.times):
            ring[ids, j] = col(f"r{j}")
        row[ids, 0] = since
        row[ids, 1] = (firing & 1) | (held << K.BURST_HELD_SHIFT) \
            | ((held % self.times) << K.BURST_POS_SHIFT)
        self.ring = torch.from_numpy(ring).to(self.device)
        self.row = torch.from_numpy(row).to(self.device)
