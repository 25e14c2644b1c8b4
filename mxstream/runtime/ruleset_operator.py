"""Broadcast rule set (``samples.key_by(k).connect(rules.broadcast(RuleSetAlert.DESCRIPTOR))
.process(RuleSetAlert(..))``).

Up to 64 rules ``id -> (comparison, threshold)`` hold for every key; every sample is tested
against all of them and leaves once per rule that it breaks, ``sample <when> threshold`` on the
two doubles (Java's rules), in ascending rule id.

The state is one table ``int64[64, 2]``: row r = (threshold bits, comparison code 1..6), code 0:
no rule r. Broadcast state is operator state: there is one copy, it has no key groups, and the
host copy is authoritative -- a run of rules is applied to it in arrival order and its 1 KiB is
copied to the device once per run.

* ``update``: the rules in arrival order, the last one of an id wins, code 0 withdraws;
* ``probe``: ``ruleset_count`` (rows per group of 64 samples, tile counts), the lookup's
  tile-count scan, one readback of the row count, ``ruleset_emit`` of the rows in sample order,
  then ascending rule id, as five int64 columns (key id, value bits, rule id, threshold bits,
  ts). With R active rules the batch is probed in slices of ``max(1, row_chunk // R)`` samples,
  so no slice emits more than `row_chunk` rows; R == 0 launches nothing.

CPU (device="cpu") runs the C++ twins (csrc/ruleset_cpu.cpp).
"""
from __future__ import annotations

import numpy as np
import torch

from ..ops import kernels as K
from .window_operator import OperatorMetrics


class RuleSetOperator:
    def __init__(self, device="cpu", row_chunk: int = 1 << 24):
        self.device = K.resolve_device(device)
        self.row_chunk = int(row_chunk)
        if self.row_chunk < 1:
            raise ValueError("row_chunk must be >= 1")
        self.host = np.zeros((K.RULESET_MAX, 2), dtype=np.int64)   # authoritative
        self.table = torch.zeros((K.RULESET_MAX, 2), dtype=torch.int64, device=self.device)
        self.metrics = OperatorMetrics()
        self.wm = K.I64_MIN

    def _cols(self, cols, names) -> int:
        n = cols[0].numel()
        for c, name in zip(cols, names):
            if c.dtype != torch.int64 or c.dim() != 1 or c.numel() != n:
                raise TypeError(f"{name}: int64 column of the batch's length expected")
            if c.device != self.device:
                raise ValueError(f"{name}: on {c.device}, expected {self.device}")
        return n

    @property
    def num_rules(self) -> int:
        return int(np.count_nonzero(self.host[:, 1]))

    # ---- elements ---------------------------------------------------------------------------
    def update(self, ids, codes, thr_bits) -> None:
        """A run of rules in arrival order: ids in [0, 64), codes 1..6 (0 withdraws the rule),
        thresholds as the bit patterns of their doubles. Sequences or numpy arrays of ints."""
        ids = np.asarray(ids, dtype=np.int64).reshape(-1)
        codes = np.asarray(codes, dtype=np.int64).reshape(-1)
        thr = np.asarray(thr_bits, dtype=np.int64).reshape(-1)
        if not ids.size == codes.size == thr.size:
            raise ValueError("ruleset: ids, codes and thresholds of one length expected")
        self.metrics.num_records_in += int(ids.size)
        if ids.size == 0:
            return
        if ids.min() < 0 or ids.max() >= K.RULESET_MAX:
            raise TypeError(f"ruleset: a rule id outside [0, {K.RULESET_MAX})")
        if codes.min() < 0 or codes.max() >= len(K.LOOKUP_WHENS):
            raise ValueError("ruleset: unknown comparison code")
        for r, c, t in zip(ids.tolist(), codes.tolist(), thr.tolist()):
            self.host[r] = (t, c) if c else (0, 0)   # arrival order: the last rule of an id wins
        self._sync_table()

    def _sync_table(self) -> None:
        self.table.copy_(torch.from_numpy(self.host))

    def probe(self, keys, vals, ts) -> list:
        """A batch of samples: one tuple of five device columns (key id, value bits, rule id,
        threshold bits, ts) per slice that has rows; rows in sample order, then ascending id."""
        n = self._cols((keys, vals, ts), ("keys", "vals", "ts"))
        self.metrics.num_records_in += n
        active = self.num_rules
        if n == 0 or active == 0:
            return []
        keys, vals, ts = keys.contiguous(), vals.contiguous(), ts.contiguous()
        step = max(1, self.row_chunk // active)
        out = []
        for lo in range(0, n, step):
            sl = slice(lo, min(n, lo + step))
            rc = K.ruleset_count(self.table, vals[sl])
            if rc.total == 0:
                continue
            out.append(K.ruleset_emit(rc, keys[sl], ts[sl]))
            self.metrics.num_fires += 1
            self.metrics.num_records_out += rc.total
        return out

    def process(self, side: int, keys, ts, vals) -> list:
        """Side 0 (samples) probes. Side 1 (rules) updates and emits nothing: `keys` are the rule
        ids, `ts` the comparison codes and `vals` the threshold bits, as host sequences."""
        if side not in (0, 1):
            raise ValueError("side must be 0 (samples) or 1 (rules)")
        if side == 1:
            self.update(keys, ts, vals)
            return []
        return self.probe(keys, vals, ts)

    def advance_watermark(self, wm: int) -> list:
        """Nothing is late and nothing fires: the watermark is only remembered."""
        if int(wm) > self.wm:
            self.wm = int(wm)
            self.metrics.current_watermark = self.wm
        return []

    def rules(self) -> dict:
        """The present rules: id -> (comparison code, threshold bits)."""
        return {int(r): (int(self.host[r, 1]), int(self.host[r, 0]))
                for r in np.nonzero(self.host[:, 1])[0]}

    # ---- checkpoints ------------------------------------------------------------------------
    def snapshot_state(self):
        from .checkpoint import OperatorSnapshot

        meta = {"kind": "ruleset", "wm": self.wm,
                "rules": [[r, c, t] for r, (c, t) in sorted(self.rules().items())],
                "metrics": {"num_records_in": self.metrics.num_records_in,
                            "num_records_out": self.metrics.num_records_out,
                            "num_fires": self.metrics.num_fires}}
        # operator state: no keyed rows, so no key groups
        return OperatorSnapshot(np.zeros(0, np.int32), {}, meta)

    def restore_state(self, rows: dict, meta: dict) -> None:
        if meta.get("kind") != "ruleset":
            raise ValueError("checkpoint of a different operator (not a rule set)")
        self.wm = meta.get("wm", K.I64_MIN)
        for k, v in meta.get("metrics", {}).items():
            setattr(self.metrics, k, v)
        self.host[:] = 0
        for r, c, t in meta.get("rules", []):
            if not 0 <= r < K.RULESET_MAX or not 1 <= c < len(K.LOOKUP_WHENS):
                raise ValueError("checkpoint with a rule outside the table")
            self.host[r] = (t, c)
        self._sync_table()
