"""Sustained-condition alerts (``stream.key_by(k).process(SustainedAlert(field, when, threshold,
for_))``).

A key is reported once, ``(key, 1, since, value)``, when ``value <when> threshold`` has held for
every element of the key since the element stamped `since` and ``ts - since >= for_ms``; and once
more, ``(key, 0, since, value)``, at the first element that ends such a run. Elements are taken
in arrival order; there are no timers, the rule is evaluated when a sample arrives.

State for dense key ids (the operator's dictionary ids for string keys, an integer key itself --
a key at or above ``dense_limit`` is refused): ``state int64[cap, 2]`` = (since, firing), since
INT64_MIN while no run is open. The capacity doubles to cover a batch's largest key id.

``process`` is one ``sustain_update``: a stable radix sort by key, one segmented wave scan of
the transition (csrc/mxs_sustain.h has the algebra), the transitions' count read back and the
rows put in arrival order. CPU (device="cpu") runs the C++ twin (csrc/sustain_cpu.cpp).
"""
from __future__ import annotations

import numpy as np

from ..ops import kernels as K
from .rule_operator import KeyedRuleOperator, threshold_bits  # noqa: F401  (imported from here)


class KeyedSustainOperator(KeyedRuleOperator):
    kind, what, tables = "sustained", "sustained-alert", ("state",)

    def __init__(self, when, threshold, for_ms: int, device="cpu", dense_limit: int = 1 << 26,
                 capacity: int = 1024):
        self._check_rule(when, threshold)
        if isinstance(for_ms, bool) or not isinstance(for_ms, int) or for_ms < 0:
            raise ValueError(f"for_ms must be an int >= 0 (milliseconds), got {for_ms!r}")
        self.for_ms = for_ms
        self._open(device, dense_limit, capacity)

    def _params(self) -> dict:
        return {"when": self.when, "threshold_bits": self.tbits, "for_ms": self.for_ms}

    def _fresh(self, cap: int):
        return (K.sustain_table(cap, self.device),)

    def _update(self, keys, vals, ts, kind, bounds):
        return K.sustain_update(self.state, keys, vals, ts, kind=kind, when=self.when,
                                threshold_bits=self.tbits, for_ms=self.for_ms, bounds=bounds)

    def entries(self):
        """The keys with an open run as host arrays (key id, since, firing), ascending by key
        id."""
        st = self.state.cpu().numpy()
        ids = np.nonzero(st[:, 0] != K.SUSTAIN_NONE)[0].astype(np.int64)
        return ids, st[ids, 0].copy(), st[ids, 1].copy()

    # ---- checkpoints ------------------------------------------------------------------------
    def _snapshot_columns(self) -> dict:
        ids, since, firing = self.entries()
        return {"key": ids, "since": since, "firing": firing}

    def _restore_rows(self, ids, col, cap: int):
        state = np.zeros((cap, 2), dtype=np.int64)
        state[:, 0] = K.SUSTAIN_NONE
        state[ids, 0], state[ids, 1] = col("since"), col("firing")
        return (state,)
