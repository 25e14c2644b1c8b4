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
import torch

from ..ops import kernels as K
from .window_operator import OperatorMetrics


def threshold_bits(threshold) -> int:
    """The bit pattern of ``float(threshold)``."""
    return int(np.array([float(threshold)], dtype=np.float64).view(np.int64)[0])


class KeyedSustainOperator:
    def __init__(self, when, threshold, for_ms: int, device="cpu", dense_limit: int = 1 << 26,
                 capacity: int = 1024):
        if K.lookup_when(when) == 0:
            raise ValueError("when must be one of '>', '>=', '<', '<=', '==', '!='")
        if isinstance(threshold, bool) or not isinstance(threshold, (int, float)):
            raise TypeError(f"threshold must be an int or a float, got {threshold!r}")
        if isinstance(for_ms, bool) or not isinstance(for_ms, int) or for_ms < 0:
            raise ValueError(f"for_ms must be an int >= 0 (milliseconds), got {for_ms!r}")
        self.when, self.threshold, self.for_ms = when, threshold, for_ms
        self.tbits = threshold_bits(threshold)
        self.device = K.resolve_device(device)
        self.dense_limit = int(dense_limit)
        if self.dense_limit < 1:
            raise ValueError("dense_limit must be >= 1")
        self.state = K.sustain_table(max(1, min(int(capacity), self.dense_limit)), self.device)
        self.metrics = OperatorMetrics()
        self.wm = K.I64_MIN

    @property
    def cap(self) -> int:
        return self.state.shape[0]

    def _grow(self, need: int) -> None:
        old = self.cap
        if need <= old:
            return
        cap = old
        while cap < need:
            cap *= 2
        state = K.sustain_table(min(cap, self.dense_limit), self.device)
        state[:old].copy_(self.state)
        self.state = state

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
            raise TypeError(f"sustained: a key outside [0, {self.dense_limit}) is not dense")
        if tmin <= -K.SUSTAIN_TS_LIMIT or tmax >= K.SUSTAIN_TS_LIMIT:
            raise TypeError("sustained: a timestamp at or beyond 2**62")
        self.metrics.num_records_in += n
        self._grow(hi + 1)
        cols = K.sustain_update(self.state, keys.contiguous(), vals.contiguous(),
                                ts.contiguous(),
                                kind=K.SUSTAIN_DOUBLE if is_float else K.SUSTAIN_LONG,
                                when=self.when, threshold_bits=self.tbits, for_ms=self.for_ms,
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
        """The keys with an open run as host arrays (key id, since, firing), ascending by key
        id."""
        st = self.state.cpu().numpy()
        ids = np.nonzero(st[:, 0] != K.SUSTAIN_NONE)[0].astype(np.int64)
        return ids, st[ids, 0].copy(), st[ids, 1].copy()

    # ---- checkpoints ------------------------------------------------------------------------
    def _params(self) -> dict:
        return {"when": self.when, "threshold_bits": self.tbits, "for_ms": self.for_ms}

    def snapshot_state(self):
        from .checkpoint import OperatorSnapshot

        ids, since, firing = self.entries()
        kg = (K.keygroups(torch.from_numpy(ids), max_parallelism=128).numpy()
              if ids.size else np.zeros(0, np.int32))
        meta = {"kind": "sustained", **self._params(), "wm": self.wm,
                "metrics": {"num_records_in": self.metrics.num_records_in,
                            "num_records_out": self.metrics.num_records_out,
                            "num_fires": self.metrics.num_fires}}
        return OperatorSnapshot(kg, {"key": ids, "since": since, "firing": firing}, meta)

    def restore_state(self, rows: dict, meta: dict) -> None:
        if meta.get("kind") != "sustained" or any(meta.get(k) != v
                                                  for k, v in self._params().items()):
            raise ValueError("checkpoint of a different sustained-alert function")
        self.wm = meta.get("wm", K.I64_MIN)
        self.metrics.current_watermark = self.wm
        for k, v in meta.get("metrics", {}).items():
            setattr(self.metrics, k, v)
        col = lambda name: np.ascontiguousarray(  # noqa: E731
            rows.get(name, np.zeros(0, np.int64)), dtype=np.int64)
        ids, since, firing = col("key"), col("since"), col("firing")
        if ids.size and (int(ids.min()) < 0 or int(ids.max()) >= self.dense_limit):
            raise ValueError("checkpoint with a key outside the dense table")
        cap = self.cap
        while ids.size and cap <= int(ids.max()):
            cap *= 2
        cap = min(cap, self.dense_limit)
        # Key groups arrive in any order; a key has one row, so the order does not matter.
        state = np.zeros((cap, 2), dtype=np.int64)
        state[:, 0] = K.SUSTAIN_NONE
        state[ids, 0], state[ids, 1] = since, firing
        self.state = torch.from_numpy(state).to(self.device)
