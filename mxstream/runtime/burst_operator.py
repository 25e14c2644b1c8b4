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

from ..ops import kernels as K
from .rule_operator import KeyedRuleOperator


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


class KeyedBurstOperator(KeyedRuleOperator):
    kind, what, tables = "burst", "burst-alert", ("ring", "row")

    def __init__(self, when, threshold, times: int, within_ms: int, device="cpu",
                 dense_limit: int = 1 << 26, capacity: int = 1024):
        self._check_rule(when, threshold)
        if isinstance(times, bool) or not isinstance(times, int) \
                or not 2 <= times <= K.BURST_MAX_TIMES:
            raise ValueError(f"times must be an int in [2, {K.BURST_MAX_TIMES}], got {times!r}")
        if isinstance(within_ms, bool) or not isinstance(within_ms, int) \
                or not 0 <= within_ms < K.SUSTAIN_TS_LIMIT:
            raise ValueError("within_ms must be an int in [0, 2**62) (milliseconds), got "
                             f"{within_ms!r}")
        self.times, self.within_ms = times, within_ms
        self._open(device, dense_limit, capacity)

    def _params(self) -> dict:
        return {"when": self.when, "threshold_bits": self.tbits, "times": self.times,
                "within_ms": self.within_ms}

    def _fresh(self, cap: int):
        return K.burst_table(cap, self.times, self.device)

    def _update(self, keys, vals, ts, kind, bounds):
        return K.burst_update(self.ring, self.row, keys, vals, ts, kind=kind, when=self.when,
                              threshold_bits=self.tbits, within=self.within_ms, bounds=bounds)

    def entries(self):
        """The keys with any state as host arrays (key id, since, firing, held, recent int64[.,
        times]: the held breaches oldest first, unused entries 0), ascending by key id."""
        since, firing, held, recent = unpack(self.ring, self.row)
        ids = np.nonzero(held)[0].astype(np.int64)
        return ids, since[ids], firing[ids], held[ids], recent[ids]

    # ---- checkpoints ------------------------------------------------------------------------
    def _snapshot_columns(self) -> dict:
        ids, since, firing, held, recent = self.entries()
        cols = {"key": ids, "since": since, "firing": firing, "held": held}
        cols.update({f"r{j}": np.ascontiguousarray(recent[:, j]) for j in range(self.times)})
        return cols

    def _restore_rows(self, ids, col, cap: int):
        since, firing, held = col("since"), col("firing"), col("held")
        if held.size and (int(held.min()) < 0 or int(held.max()) > self.times):
            raise ValueError("checkpoint with more breaches than the rule holds")
        # The held breaches go to slots 0 .. held - 1, the next one to slot held mod times.
        ring = np.zeros((cap, self.times), dtype=np.int64)
        row = np.zeros((cap, 2), dtype=np.int64)
        for j in range(self.times):
            ring[ids, j] = col(f"r{j}")
        row[ids, 0] = since
        row[ids, 1] = (firing & 1) | (held << K.BURST_HELD_SHIFT) \
            | ((held % self.times) << K.BURST_POS_SHIFT)
        return ring, row
