"""Keyed interval joins (Flink 1.8 ``a.intervalJoin(b).between(lo, hi).process(fn)``).

A pair (l, r) of one key matches iff ``l.ts + lo <= r.ts <= l.ts + hi``. An arriving element is
joined at once with every matching element the other side has buffered, then buffered itself. A
left element is removed by a watermark ``wm >= l.ts + max(hi, 0)``, a right one by
``wm >= r.ts + max(-lo, 0)``; an element behind the watermark is late, dropped and counted. All
``ts +- bound`` sums saturate at the int64 limits.

Each side keeps one buffer of three int64 device columns (key id, ts, value bits), ascending by
(key, ts) with equal (key, ts) in arrival order. ``process(side, ...)``

* drops late rows and sorts the batch by (key, ts) (two stable radix passes over the used bits);
* ``ijoin_probe``: every batch element's range of rows in the other side's buffer;
* ``ijoin_scan``: the exclusive 64-bit scan of the range lengths, non-empty elements compacted;
* one readback of the batch's pair total P;
* ``ijoin_expand`` over [p0, p1) in chunks of at most ``pair_chunk`` pairs: four int64 columns
  (key id, left value bits, right value bits, max(l.ts, r.ts));
* ``ijoin_merge``: the batch goes into its own side's buffer (old rows first on ties).

Clean-up is lazy: ``advance_watermark`` only moves each side's cut-off timestamp (rows with
``ts <= cutoff`` are expired). The probe takes the other side's cut-off and never matches an
expired row; a side is compacted (``ijoin_purge``) before the next merge into it and before a
snapshot. A restored buffer holds live rows only, so ``restore_state`` applies the same step
back of the cut-off as a compaction does (``_step_back``): rows at ts == wm stay visible.

Host readbacks of a ``process`` call: the batch's extremes and late count (they size the radix
passes), (P, m, error), and the survivor count of a compaction when the side's cut-off has moved
since the last one. CPU (device="cpu") runs the C++ twins (csrc/ijoin_cpu.cpp).
"""
from __future__ import annotations

import numpy as np
import torch

from ..ops import kernels as K
from .window_operator import OperatorMetrics

I64_MIN, I64_MAX = K.I64_MIN, K.I64_MAX
FLINK_BOUNDS_MSG = "lowerBound <= upperBound must be fulfilled"


def check_bounds(lo: int, hi: int) -> tuple[int, int]:
    lo, hi = int(lo), int(hi)
    if not (I64_MIN < lo <= I64_MAX and I64_MIN < hi <= I64_MAX):
        raise ValueError("interval join bounds must be int64 milliseconds")
    if lo > hi:
        raise ValueError(FLINK_BOUNDS_MSG)
    return lo, hi


class KeyedIntervalJoinOperator:
    def __init__(self, *, lo: int, hi: int, device="cpu", pair_chunk: int = 1 << 24,
                 capacity: int = 1024):
        if int(pair_chunk) < 1:
            raise ValueError("pair_chunk must be >= 1")
        self.lo, self.hi = check_bounds(lo, hi)
        self.pair_chunk = int(pair_chunk)
        self.device = K.resolve_device(device)
        # How long an element outlives its timestamp: left max(hi, 0), right max(-lo, 0).
        self.keep = (max(self.hi, 0), max(-self.lo, 0))
        cap = max(2, int(capacity))
        self.buf = [torch.empty((3, cap), dtype=torch.int64, device=self.device) for _ in range(2)]
        self.spare = [None, None]      # the previous buffer of a side, reused by the next merge
        self.n = [0, 0]                # rows of a buffer, expired ones included
        self.cutoff = [I64_MIN, I64_MIN]   # rows with ts <= cutoff are expired
        self.purged = [I64_MIN, I64_MIN]   # the cut-off a buffer was last compacted for
        self.wm = I64_MIN
        self.metrics = OperatorMetrics()
        self.pairs_out = 0

    # ---- buffers ----------------------------------------------------------------------------
    def _cols(self, side: int):
        b, n = self.buf[side], self.n[side]
        return b[0, :n], b[1, :n], b[2, :n]

    def _target(self, side: int, rows: int) -> torch.Tensor:
        """A buffer of >= rows that is not the side's current one (capacity grows geometrically)."""
        sp = self.spare[side]
        if sp is None or sp.shape[1] < rows:
            cap = max(self.buf[side].shape[1], 2)
            while cap < rows:
                cap *= 2
            sp = torch.empty((3, cap), dtype=torch.int64, device=self.device)
        return sp

    def _swap(self, side: int, new: torch.Tensor, rows: int) -> None:
        old = self.buf[side]
        self.buf[side], self.n[side] = new, rows
        self.spare[side] = old if old.shape[1] >= new.shape[1] else None

    def _purge(self, side: int) -> None:
        if self.purged[side] == self.cutoff[side]:
            return
        if self.n[side]:
            out = self._target(side, self.n[side])
            self._swap(side, out, K.ijoin_purge(self._cols(side), self.cutoff[side], out))
        self.purged[side] = self.cutoff[side]

    def _step_back(self, side: int) -> None:
        """For a side whose buffer holds no expired row (just compacted, or just restored). An
        element at ts == wm is not late and outlives this watermark (its clean-up timer fires with
        the next one); where the cut-off equals the watermark, stepping it back by one keeps
        exactly the rows that are in the buffer now or arrive from now on."""
        if self.cutoff[side] == self.wm != I64_MIN:
            self.cutoff[side] = self.purged[side] = self.wm - 1

    def buffered(self, side: int):
        """The live rows of a side as host arrays (key, ts, val), in buffer order."""
        self._purge(side)
        return tuple(c.cpu().numpy().copy() for c in self._cols(side))

    # ---- elements ---------------------------------------------------------------------------
    def _sorted_batch(self, keys, ts, vals):
        """Late rows dropped; the rest stably sorted by (key, ts). One readback of the batch's
        extremes (they size the two radix passes)."""
        n = keys.numel()
        late = ts < self.wm if self.wm != I64_MIN else None
        stats = torch.stack([ts.min(), ts.max(), keys.min(), keys.max(),
                             late.sum() if late is not None else ts.new_zeros(())]).tolist()
        tmin, tmax, kmin, kmax, nlate = stats
        if tmin == I64_MIN:
            raise ValueError("interval join: an element without a timestamp (Long.MIN_VALUE); "
                             "assign timestamps and watermarks first")
        if nlate:
            self.metrics.num_late_records_dropped += nlate
            keep = ~late
            keys, ts, vals = keys[keep], ts[keep], vals[keep]
            n = keys.numel()
            if n == 0:
                return keys, ts, vals
            tmin = max(tmin, self.wm)
        idx = torch.arange(n, dtype=torch.int64, device=keys.device)
        tbits = max(1, (tmax - tmin).bit_length())
        _, perm = K.sort_pairs((ts - tmin).contiguous(), idx, bits=tbits)
        kbits = max(1, (kmax - kmin).bit_length())
        _, perm = K.sort_pairs((keys[perm] - kmin).contiguous(), perm, bits=kbits)
        return keys[perm], ts[perm], vals[perm]

    def process(self, side: int, keys, ts, vals) -> list:
        """Join a batch of side 0 (left) or 1 (right) with the other side's buffer and buffer it:
        keys int64 ids, ts int64, vals int64 value bits. Returns the pairs as chunks of device
        columns (key id, left value bits, right value bits, ts)."""
        if side not in (0, 1):
            raise ValueError("side must be 0 (left) or 1 (right)")
        n = keys.numel()
        for c, name in ((keys, "keys"), (ts, "ts"), (vals, "vals")):
            if c.dtype != torch.int64 or c.dim() != 1 or c.numel() != n:
                raise TypeError(f"{name}: int64 column of the batch's length expected")
            if c.device != self.device:
                raise ValueError(f"{name}: on {c.device}, expected {self.device}")
        self.metrics.num_records_in += n
        if n == 0:
            return []
        batch = tuple(c.contiguous() for c in self._sorted_batch(keys, ts, vals))
        if batch[0].numel() == 0:
            return []
        out = []
        other = 1 - side
        if self.n[other]:
            jp = K.ijoin_plan(side, batch, self._cols(other), self.lo, self.hi, self.cutoff[other])
            for p0 in range(0, jp.pairs, self.pair_chunk):
                out.append(K.ijoin_expand(jp, p0, min(jp.pairs, p0 + self.pair_chunk)))
            if jp.pairs:
                self.metrics.num_fires += 1
                self.metrics.num_records_out += jp.pairs
                self.pairs_out += jp.pairs
        self._purge(side)
        self._step_back(side)
        rows = self.n[side] + batch[0].numel()
        dst = self._target(side, rows)
        self._swap(side, dst, K.ijoin_merge(self._cols(side), batch, dst))
        return out

    def advance_watermark(self, wm: int) -> list:
        """Move both sides' cut-offs; emits nothing. A row is expired once
        ``wm >= ts + keep`` (saturating), i.e. ``ts <= wm - keep``; Long.MAX_VALUE expires all."""
        wm = int(wm)
        if wm <= self.wm:
            return []
        self.wm = wm
        self.metrics.current_watermark = wm
        for s in (0, 1):
            self.cutoff[s] = I64_MAX if wm == I64_MAX else K.sat_add_i64(wm, -self.keep[s])
        return []

    # ---- checkpoints ------------------------------------------------------------------------
    def snapshot_state(self):
        """Both buffers' live rows (side, key, ts, value bits) + bounds, watermark, counters."""
        from .checkpoint import OperatorSnapshot

        sides = [self.buffered(s) for s in (0, 1)]
        cols = {name: np.concatenate([sd[i] for sd in sides])
                for i, name in enumerate(("key", "ts", "val"))}
        cols["side"] = np.concatenate([np.full(sd[0].size, s, dtype=np.int64)
                                       for s, sd in enumerate(sides)])
        keys = cols["key"]
        kg = (K.keygroups(torch.from_numpy(keys), max_parallelism=128).numpy()
              if keys.size else np.zeros(0, np.int32))
        meta = {"kind": "interval_join", "lo": self.lo, "hi": self.hi, "wm": self.wm,
                "pairs_out": self.pairs_out,
                "metrics": {"num_records_in": self.metrics.num_records_in,
                            "num_late_records_dropped": self.metrics.num_late_records_dropped,
                            "num_records_out": self.metrics.num_records_out,
                            "num_fires": self.metrics.num_fires}}
        return OperatorSnapshot(kg, cols, meta)

    def restore_state(self, rows: dict, meta: dict) -> None:
        if meta.get("kind") != "interval_join" or (meta["lo"], meta["hi"]) != (self.lo, self.hi):
            raise ValueError("checkpoint of a different interval join")
        self.wm = I64_MIN
        self.advance_watermark(meta["wm"])
        self.pairs_out = meta.get("pairs_out", 0)
        for k, v in meta.get("metrics", {}).items():
            setattr(self.metrics, k, v)
        side = np.asarray(rows.get("side", np.zeros(0, np.int64)), dtype=np.int64)
        for s in (0, 1):
            sel = side == s
            cols = [np.asarray(rows[name], dtype=np.int64)[sel] if side.size
                    else np.zeros(0, np.int64) for name in ("key", "ts", "val")]
            # Key groups arrive in any order: restore the (key, ts) order, arrival order on ties
            # (within a key group the rows keep the snapshot's order).
            order = np.lexsort((cols[1], cols[0]))
            rows_n = int(order.size)
            dst = self._target(s, rows_n)
            for i, c in enumerate(cols):
                dst[i, :rows_n].copy_(torch.from_numpy(np.ascontiguousarray(c[order])))
            self._swap(s, dst, rows_n)
            self.purged[s] = self.cutoff[s]
            self._step_back(s)  # a snapshot holds live rows only, some of them at ts == wm
