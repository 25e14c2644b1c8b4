"""Keyed latest-value lookup (``samples.connect(rules).key_by(k1, k2).process(LookupLatest(..))``).

A rule stream keeps one value per key; every sample of the other stream reads the value in force
for its key (its key's last rule, else the default, else the sample is dropped) and leaves only
when ``sample <when> value`` holds on the two doubles (Java's rules; `when` None: always).

The state is one device table ``int64[cap, 2]``: row k = (value bits, present 0 / 1) of key id k,
one 16-byte load per lookup. Key ids are dense: the operator's dictionary ids for string keys, an
integer key itself -- a rule key at or above ``dense_limit`` is refused. The capacity doubles,
zero-filled, to cover the largest key id of a rule batch; a sample key at or beyond it has no rule.

* ``upsert``: the rules in arrival order, the last one of a key wins (stable radix sort by key,
  the row that ends its key's run stores; no atomics);
* ``probe``: ``lookup_mask`` (ballot words per 64 rows, tile counts), the tile-count scan, one
  readback of the kept count, ``lookup_emit`` of the kept rows in input order as four int64
  columns (key id, value bits, looked-up bits, ts). With no comparison and a default every row is
  kept and one gather kernel writes the columns.

CPU (device="cpu") runs the C++ twins (csrc/lookup_cpu.cpp).
"""
from __future__ import annotations

import numpy as np
import torch

from ..ops import kernels as K
from .window_operator import OperatorMetrics


class KeyedLookupOperator:
    def __init__(self, when=None, default_bits=None, device="cpu", dense_limit: int = 1 << 26,
                 capacity: int = 1024):
        self.when = when
        K.lookup_when(when)
        self.default_bits = None if default_bits is None else int(default_bits)
        self.device = K.resolve_device(device)
        self.dense_limit = int(dense_limit)
        if self.dense_limit < 1:
            raise ValueError("dense_limit must be >= 1")
        self.table = torch.zeros((max(1, min(int(capacity), self.dense_limit)), 2),
                                 dtype=torch.int64, device=self.device)
        self.metrics = OperatorMetrics()
        self.wm = K.I64_MIN

    @property
    def cap(self) -> int:
        return self.table.shape[0]

    def _cols(self, cols, names) -> int:
        n = cols[0].numel()
        for c, name in zip(cols, names):
            if c.dtype != torch.int64 or c.dim() != 1 or c.numel() != n:
                raise TypeError(f"{name}: int64 column of the batch's length expected")
            if c.device != self.device:
                raise ValueError(f"{name}: on {c.device}, expected {self.device}")
        return n

    def _grow(self, need: int) -> None:
        cap = self.cap
        if need <= cap:
            return
        while cap < need:
            cap *= 2
        table = torch.zeros((min(cap, self.dense_limit), 2), dtype=torch.int64,
                            device=self.device)
        table[:self.cap].copy_(self.table)
        self.table = table

    # ---- elements ---------------------------------------------------------------------------
    def upsert(self, keys, vals) -> None:
        """A batch of rules in arrival order: keys int64 ids, vals int64 value bits."""
        n = self._cols((keys, vals), ("keys", "vals"))
        self.metrics.num_records_in += n
        if n == 0:
            return
        lo, hi = torch.stack([keys.min(), keys.max()]).tolist()
        if lo < 0 or hi >= self.dense_limit:
            raise TypeError(f"lookup: a rule key outside [0, {self.dense_limit}) is not dense")
        self._grow(hi + 1)
        K.lookup_upsert(self.table, keys.contiguous(), vals.contiguous(), max_key=hi)

    def probe(self, keys, vals, ts):
        """A batch of samples: the kept rows in input order as four device columns (key id, value
        bits, looked-up bits, ts)."""
        n = self._cols((keys, vals, ts), ("keys", "vals", "ts"))
        self.metrics.num_records_in += n
        keys, vals, ts = keys.contiguous(), vals.contiguous(), ts.contiguous()
        if self.when is None and self.default_bits is not None:
            out = K.lookup_gather(self.table, keys, vals, ts, self.default_bits)
        else:
            lm = K.lookup_mask(self.table, keys, vals, self.when, self.default_bits)
            out = K.lookup_emit(lm, ts)
        kept = out[0].numel()
        if kept:
            self.metrics.num_fires += 1
            self.metrics.num_records_out += kept
        return out

    def process(self, side: int, keys, ts, vals) -> list:
        """Side 1 (rules) upserts and emits nothing; side 0 (samples) probes."""
        if side not in (0, 1):
            raise ValueError("side must be 0 (samples) or 1 (rules)")
        if side == 1:
            self.upsert(keys, vals)
            return []
        out = self.probe(keys, vals, ts)
        return [out] if out[0].numel() else []

    def advance_watermark(self, wm: int) -> list:
        """Nothing is late and nothing fires: the watermark is only remembered."""
        if int(wm) > self.wm:
            self.wm = int(wm)
            self.metrics.current_watermark = self.wm
        return []

    def entries(self):
        """The present entries as host arrays (key id, value bits), ascending by key id."""
        tab = self.table.cpu().numpy()
        ids = np.nonzero(tab[:, 1])[0].astype(np.int64)
        return ids, tab[ids, 0].copy()

    # ---- checkpoints ------------------------------------------------------------------------
    def snapshot_state(self):
        from .checkpoint import OperatorSnapshot

        ids, bits = self.entries()
        kg = (K.keygroups(torch.from_numpy(ids), max_parallelism=128).numpy()
              if ids.size else np.zeros(0, np.int32))
        meta = {"kind": "lookup", "when": self.when, "default_bits": self.default_bits,
                "wm": self.wm,
                "metrics": {"num_records_in": self.metrics.num_records_in,
                            "num_records_out": self.metrics.num_records_out,
                            "num_fires": self.metrics.num_fires}}
        return OperatorSnapshot(kg, {"key": ids, "val": bits}, meta)

    def restore_state(self, rows: dict, meta: dict) -> None:
        if meta.get("kind") != "lookup" or meta.get("when") != self.when \
                or meta.get("default_bits") != self.default_bits:
            raise ValueError("checkpoint of a different lookup")
        self.wm = meta.get("wm", K.I64_MIN)
        for k, v in meta.get("metrics", {}).items():
            setattr(self.metrics, k, v)
        ids = np.ascontiguousarray(rows.get("key", np.zeros(0, np.int64)), dtype=np.int64)
        bits = np.ascontiguousarray(rows.get("val", np.zeros(0, np.int64)), dtype=np.int64)
        self.table.zero_()
        if ids.size:
            # Key groups arrive in any order; a key has one row, so the order does not matter.
            n_in = self.metrics.num_records_in
            self.upsert(torch.from_numpy(ids).to(self.device),
                        torch.from_numpy(bits).to(self.device))
            self.metrics.num_records_in = n_in
