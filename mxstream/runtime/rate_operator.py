"""Counter rates (``stream.key_by(k).process(CounterRate(field, per, when, threshold,
max_gap))``).

Every key holds its last accepted sample ``(last_ts, last value)``. A sample above the key's
last timestamp is accepted and gives ``dt``, ``inc`` (``v - last``, or ``v`` after a counter
reset) and ``rate = float(inc) * per / dt``; a duplicate or a straggler is ignored and counted in
``out_of_order``. The row ``(key, rate, inc, dt)`` leaves unless ``dt > max_gap`` or the rule
``rate <when> threshold`` fails. Elements are taken in arrival order; there are no timers.

State for dense key ids (the operator's dictionary ids for string keys, an integer key itself --
a key at or above ``dense_limit`` is refused): ``state int64[cap, 2]`` = (last_ts, last value
bits), last_ts INT64_MIN while the key was never seen. The capacity doubles to cover a batch's
largest key id. The counter is all longs or all doubles: the first batch decides, a batch of the
other kind afterwards is a TypeError.

``process`` is one ``rate_update``: a stable radix sort by key, one segmented wave scan of
(timestamp, value) pairs under arg-max (csrc/mxs_rate.h has the algebra) that places
(inc, dt) by arrival index, and a mask / scan / emit compaction in arrival order; the rows'
count and the ignored elements' come back in one readback. The columns are (key id, rate bits,
inc bits, dt, ts). CPU (device="cpu") runs the C++ twin (csrc/rate_cpu.cpp).
"""
from __future__ import annotations

import numpy as np

from ..ops import kernels as K
from .rule_operator import KeyedRuleOperator


class KeyedRateOperator(KeyedRuleOperator):
    kind, what, tables = "counter_rate", "counter-rate", ("state",)

    def __init__(self, per_ms: int = 1000, when=None, threshold=None, max_gap=None,
                 device="cpu", dense_limit: int = 1 << 26, capacity: int = 1024):
        if isinstance(per_ms, bool) or not isinstance(per_ms, int) or not 1 <= per_ms <= K.I64_MAX:
            raise ValueError(f"per_ms must be an int >= 1, got {per_ms!r}")
        if max_gap is not None and (isinstance(max_gap, bool) or not isinstance(max_gap, int)
                                    or not 1 <= max_gap < K.SUSTAIN_TS_LIMIT):
            raise ValueError(f"max_gap must be None or an int in [1, 2**62), got {max_gap!r}")
        if when is None:
            if threshold is not None:
                raise ValueError("a threshold without when")
            self.when, self.threshold, self.tbits = None, None, 0
        else:
            if threshold is None:
                raise ValueError("when without a threshold")
            self._check_rule(when, threshold)
        self.per_ms, self.max_gap = per_ms, max_gap
        self.value_kind = None   # K.SUSTAIN_LONG / K.SUSTAIN_DOUBLE once a batch was taken
        self.out_of_order = 0
        self._open(device, dense_limit, capacity)

    def _params(self) -> dict:
        return {"per_ms": self.per_ms, "when": self.when, "threshold_bits": self.tbits,
                "max_gap": self.max_gap}

    def _fresh(self, cap: int):
        return (K.rate_table(cap, self.device),)

    def process(self, keys, vals, ts, is_float: bool = True) -> list:
        kind = K.SUSTAIN_DOUBLE if is_float else K.SUSTAIN_LONG
        if self.value_kind is not None and kind != self.value_kind and keys.numel():
            raise TypeError("counter_rate: the counter is all longs or all doubles, got a batch "
                            f"of {'doubles' if is_float else 'longs'}")
        return super().process(keys, vals, ts, is_float)

    def _update(self, keys, vals, ts, kind, bounds):
        cols, ignored = K.rate_update(self.state, keys, vals, ts, kind=kind, per_ms=self.per_ms,
                                      when=self.when, threshold_bits=self.tbits,
                                      max_gap=self.max_gap, bounds=bounds)
        self.value_kind = kind
        self.out_of_order += ignored
        return cols

    def entries(self):
        """Every key seen as host arrays (key id, last_ts, last value bits), ascending by key
        id."""
        st = self.state.cpu().numpy()
        ids = np.nonzero(st[:, 0] != K.RATE_NONE)[0].astype(np.int64)
        return ids, st[ids, 0].copy(), st[ids, 1].copy()

    # ---- checkpoints ------------------------------------------------------------------------
    def _snapshot_columns(self) -> dict:
        ids, last_ts, last = self.entries()
        return {"key": ids, "last_ts": last_ts, "last_value": last}

    def snapshot_state(self):
        snap = super().snapshot_state()
        snap.meta["value_kind"] = self.value_kind
        snap.meta["out_of_order"] = self.out_of_order
        return snap

    def restore_state(self, rows: dict, meta: dict) -> None:
        vk = meta.get("value_kind")
        if vk not in (None, K.SUSTAIN_LONG, K.SUSTAIN_DOUBLE):
            raise ValueError("checkpoint with an unknown counter kind")
        super().restore_state(rows, meta)
        self.value_kind = vk
        self.out_of_order = int(meta.get("out_of_order", 0))

    def _restore_rows(self, ids, col, cap: int):
        last_ts, last = col("last_ts"), col("last_value")
        if last_ts.size != ids.size or last.size != ids.size:
            raise ValueError("checkpoint columns of different lengths")
        if last_ts.size and (bool((last_ts <= -K.SUSTAIN_TS_LIMIT).any())
                             or bool((last_ts >= K.SUSTAIN_TS_LIMIT).any())):
            raise ValueError("checkpoint with a key that was never seen")
        state = np.zeros((cap, 2), dtype=np.int64)
        state[:, 0] = K.RATE_NONE
        state[ids, 0], state[ids, 1] = last_ts, last
        return (state,)
