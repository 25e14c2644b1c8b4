"""What the keyed alert rules' engines share (sustain_operator.py, burst_operator.py): a rule
``value <when> threshold`` over dense key ids, evaluated when a sample arrives, with per-key
tables of `cap` rows that double to cover a batch's largest key id.

A subclass sets `kind` (the checkpoint's kind and the prefix of its errors), `what` (the rule's
name in a checkpoint error) and `tables` (the attributes that hold its tables), checks its own
parameters between ``_check_rule`` and ``_open`` and supplies ``_params``, ``_fresh``,
``_update``, ``entries``, ``_snapshot_columns`` and ``_restore_rows``.
"""
from __future__ import annotations

import numpy as np
import torch

from ..ops import kernels as K
from .window_operator import OperatorMetrics


def threshold_bits(threshold) -> int:
    """The bit pattern of ``float(threshold)``."""
    return int(np.array([float(threshold)], dtype=np.float64).view(np.int64)[0])


def metrics_meta(metrics) -> dict:
    """The counters an engine's checkpoint keeps."""
    return {"num_records_in": metrics.num_records_in,
            "num_records_out": metrics.num_records_out,
            "num_fires": metrics.num_fires}


class KeyedRuleOperator:
    kind = what = ""
    tables: tuple = ()

    def _check_rule(self, when, threshold) -> None:
        if K.lookup_when(when) == 0:
            raise ValueError("when must be one of '>', '>=', '<', '<=', '==', '!='")
        if isinstance(threshold, bool) or not isinstance(threshold, (int, float)):
            raise TypeError(f"threshold must be an int or a float, got {threshold!r}")
        self.when, self.threshold = when, threshold
        self.tbits = threshold_bits(threshold)

    def _open(self, device, dense_limit: int, capacity: int) -> None:
        self.device = K.resolve_device(device)
        self.dense_limit = int(dense_limit)
        if self.dense_limit < 1:
            raise ValueError("dense_limit must be >= 1")
        self._set_tables(self._fresh(max(1, min(int(capacity), self.dense_limit))))
        self.metrics = OperatorMetrics()
        self.wm = K.I64_MIN

    def _set_tables(self, new) -> None:
        for name, t in zip(self.tables, new):
            setattr(self, name, t)

    @property
    def cap(self) -> int:
        return getattr(self, self.tables[-1]).shape[0]

    def _grow(self, need: int) -> None:
        old = self.cap
        if need <= old:
            return
        cap = old
        while cap < need:
            cap *= 2
        new = self._fresh(min(cap, self.dense_limit))
        for name, t in zip(self.tables, new):
            t[:old].copy_(getattr(self, name))
        self._set_tables(new)

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
            raise TypeError(f"{self.kind}: a key outside [0, {self.dense_limit}) is not dense")
        if tmin <= -K.SUSTAIN_TS_LIMIT or tmax >= K.SUSTAIN_TS_LIMIT:
            raise TypeError(f"{self.kind}: a timestamp at or beyond 2**62")
        self.metrics.num_records_in += n
        self._grow(hi + 1)
        cols = self._update(keys.contiguous(), vals.contiguous(), ts.contiguous(),
                            K.SUSTAIN_DOUBLE if is_float else K.SUSTAIN_LONG, (hi, tmin, tmax))
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

    # ---- checkpoints ------------------------------------------------------------------------
    def snapshot_state(self):
        from .checkpoint import OperatorSnapshot

        cols = self._snapshot_columns()
        ids = cols["key"]
        kg = (K.keygroups(torch.from_numpy(ids), max_parallelism=128).numpy()
              if ids.size else np.zeros(0, np.int32))
        meta = {"kind": self.kind, **self._params(), "wm": self.wm,
                "metrics": metrics_meta(self.metrics)}
        return OperatorSnapshot(kg, cols, meta)

    def restore_state(self, rows: dict, meta: dict) -> None:
        if meta.get("kind") != self.kind or any(meta.get(k) != v
                                                for k, v in self._params().items()):
            raise ValueError(f"checkpoint of a different {self.what} function")
        self.wm = meta.get("wm", K.I64_MIN)
        self.metrics.current_watermark = self.wm
        for k, v in meta.get("metrics", {}).items():
            setattr(self.metrics, k, v)
        col = lambda name: np.ascontiguousarray(  # noqa: E731
            rows.get(name, np.zeros(0, np.int64)), dtype=np.int64)
        ids = col("key")
        if ids.size and (int(ids.min()) < 0 or int(ids.max()) >= self.dense_limit):
            raise ValueError("checkpoint with a key outside the dense table")
        cap = self.cap
        while ids.size and cap <= int(ids.max()):
            cap *= 2
        # Key groups arrive in any order; a key has one row, so the order does not matter.
        self._set_tables(torch.from_numpy(a).to(self.device)
                         for a in self._restore_rows(ids, col, min(cap, self.dense_limit)))
