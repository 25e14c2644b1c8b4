"""Keyed event-time timers (``stream.key_by(k).process(CountWithTimeout(timeout))``).

Every key counts its elements and remembers the timestamp of the last one; when the watermark
passes ``last + timeout`` the key emits ``(key, count, last)`` stamped with that deadline. The
per-record operator registers a timer per element, and every timer but the one at
``last + timeout`` finds a newer `last` and emits nothing. The engine keeps that one timer: a key
is *armed* with ``deadline = last + timeout`` by every batch that holds it (again after it fired,
also when the deadline already lies at or below the watermark) and disarmed by its firing.

State for dense key ids (the operator's dictionary ids for string keys, an integer key itself --
a key at or above ``dense_limit`` is refused): ``state int64[cap, 2]`` = (count, last),
``deadline int64[cap]`` (INT64_MAX: not armed) and ``tile_min``, a lower bound of the deadlines
of every tile of 4096 key ids. The capacity doubles to cover a batch's largest key id.

* ``process``: ``timeout_update`` (stable radix sort by key; the row that ends its key's run
  writes count, last and deadline and lowers the tile's bound);
* ``advance_watermark``: ``timeout_mask`` reads only the tiles whose bound the watermark has
  reached, the tile-count scan and one readback give the number of due keys, ``timeout_emit``
  writes them in key order and disarms them; the rows are then ordered by deadline (stable radix
  sort over the bits their span needs: ties stay in key order).

CPU (device="cpu") runs the C++ twins (csrc/timeout_cpu.cpp).
"""
from __future__ import annotations

import numpy as np
import torch

from ..ops import kernels as K
from .rule_operator import metrics_meta
from .window_operator import OperatorMetrics


class KeyedTimeoutOperator:
    def __init__(self, timeout: int, device="cpu", dense_limit: int = 1 << 26,
                 capacity: int = 1024):
        if isinstance(timeout, bool) or not isinstance(timeout, int) or timeout <= 0:
            raise ValueError(f"timeout must be a positive int (milliseconds), got {timeout!r}")
        self.timeout = timeout
        self.device = K.resolve_device(device)
        self.dense_limit = int(dense_limit)
        if self.dense_limit < 1:
            raise ValueError("dense_limit must be >= 1")
        self.state, self.deadline, self.tile_min = K.timeout_tables(
            max(1, min(int(capacity), self.dense_limit)), self.device)
        self.metrics = OperatorMetrics()
        self.wm = K.I64_MIN

    @property
    def cap(self) -> int:
        return self.deadline.shape[0]

    def _grow(self, need: int) -> None:
        old = self.cap
        if need <= old:
            return
        cap = old
        while cap < need:
            cap *= 2
        state, deadline, tile_min = K.timeout_tables(min(cap, self.dense_limit), self.device)
        state[:old].copy_(self.state)
        deadline[:old].copy_(self.deadline)
        tile_min[:self.tile_min.numel()].copy_(self.tile_min)
        self.state, self.deadline, self.tile_min = state, deadline, tile_min

    # ---- elements ---------------------------------------------------------------------------
    def process(self, keys, ts) -> list:
        """A batch of elements in arrival order: keys int64 ids, ts int64 timestamps."""
        n = keys.numel()
        for c, name in ((keys, "keys"), (ts, "ts")):
            if c.dtype != torch.int64 or c.dim() != 1 or c.numel() != n:
                raise TypeError(f"{name}: int64 column of the batch's length expected")
            if c.device != self.device:
                raise ValueError(f"{name}: on {c.device}, expected {self.device}")
        if n == 0:
            return []
        lo, hi, tmax = torch.stack([keys.min(), keys.max(), ts.max()]).tolist()
        if lo < 0 or hi >= self.dense_limit:
            raise TypeError(f"timeout: a key outside [0, {self.dense_limit}) is not dense")
        if tmax >= K.I64_MAX - self.timeout:
            raise TypeError("timeout: timestamp + timeout reaches INT64_MAX")
        self.metrics.num_records_in += n
        self._grow(hi + 1)
        K.timeout_update(self.state, self.deadline, self.tile_min, keys.contiguous(),
                         ts.contiguous(), self.timeout, bounds=(hi, tmax))
        return []

    def advance_watermark(self, wm: int) -> list:
        """Every armed key whose deadline the watermark has reached, ascending by (deadline, key
        id): [] or one chunk of four device columns (key id, count, last, deadline)."""
        w = max(int(wm), self.wm)
        self.wm = w
        self.metrics.current_watermark = w
        tm = K.timeout_mask(self.deadline, self.tile_min, w)
        if tm.total == 0:
            return []
        key, count, last, dl = K.timeout_emit(self.state, self.deadline, tm)
        if tm.total > 1:
            # Stable sort by deadline over the bits the rows' span needs (a second readback:
            # the deadlines of one advance lie close together, two radix passes instead of
            # eight); a span beyond 62 bits sorts the sign-flipped deadline bits.
            lo, hi = torch.stack([dl.min(), dl.max()]).tolist()
            idx = torch.arange(tm.total, dtype=torch.int64, device=self.device)
            if hi == lo:
                order = idx
            elif hi - lo < (1 << 62):
                _, order = K.sort_pairs(dl - lo, idx, bits=max(1, (hi - lo).bit_length()))
            else:
                _, order = K.sort_pairs(dl ^ K.I64_MIN, idx)
            key, count, last, dl = key[order], count[order], last[order], dl[order]
        self.metrics.num_fires += 1
        self.metrics.num_records_out += tm.total
        return [(key, count, last, dl)]

    def entries(self):
        """The keys seen so far as host arrays (key id, count, last, deadline), ascending by key
        id; deadline is INT64_MAX for a key that is not armed."""
        st = self.state.cpu().numpy()
        ids = np.nonzero(st[:, 0])[0].astype(np.int64)
        return ids, st[ids, 0].copy(), st[ids, 1].copy(), self.deadline.cpu().numpy()[ids].copy()

    # ---- checkpoints ------------------------------------------------------------------------
    def snapshot_state(self):
        from .checkpoint import OperatorSnapshot

        ids, count, last, dl = self.entries()
        kg = (K.keygroups(torch.from_numpy(ids), max_parallelism=128).numpy()
              if ids.size else np.zeros(0, np.int32))
        meta = {"kind": "count_timeout", "timeout": self.timeout, "wm": self.wm,
                "metrics": metrics_meta(self.metrics)}
        return OperatorSnapshot(kg, {"key": ids, "count": count, "last": last, "deadline": dl},
                                meta)

    def restore_state(self, rows: dict, meta: dict) -> None:
        if meta.get("kind") != "count_timeout" or meta.get("timeout") != self.timeout:
            raise ValueError("checkpoint of a different timeout function")
        self.wm = meta.get("wm", K.I64_MIN)
        self.metrics.current_watermark = self.wm
        for k, v in meta.get("metrics", {}).items():
            setattr(self.metrics, k, v)
        col = lambda name: np.ascontiguousarray(  # noqa: E731
            rows.get(name, np.zeros(0, np.int64)), dtype=np.int64)
        ids, count, last, dl = col("key"), col("count"), col("last"), col("deadline")
        if ids.size and (int(ids.min()) < 0 or int(ids.max()) >= self.dense_limit):
            raise ValueError("checkpoint with a key outside the dense table")
        cap = self.cap
        while ids.size and cap <= int(ids.max()):
            cap *= 2
        cap = min(cap, self.dense_limit)
        # Key groups arrive in any order; a key has one row, so the order does not matter.
        state = np.zeros((cap, 2), dtype=np.int64)
        deadline = np.full(cap, K.TIMEOUT_NONE, dtype=np.int64)
        tile_min = np.full((cap + K.TIMEOUT_TILE - 1) // K.TIMEOUT_TILE, K.TIMEOUT_NONE,
                           dtype=np.int64)
        state[ids, 0], state[ids, 1], deadline[ids] = count, last, dl
        np.minimum.at(tile_min, ids // K.TIMEOUT_TILE, dl)
        self.state, self.deadline, self.tile_min = (
            torch.from_numpy(a).to(self.device) for a in (state, deadline, tile_min))
