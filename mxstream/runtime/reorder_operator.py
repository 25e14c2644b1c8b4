"""The event-time reorder buffer in front of the keyed rules
(``stream.key_by(k).process(EventTimeOrdered(rule))``; design: csrc/mxs_reorder.h).

Rows ``(key id, ts, value bits)`` are held until the watermark reaches them and leave in
(ts, arrival) order; a row with ``ts <= watermark`` on arrival is late: dropped and counted.

State: one linear device arena ``int64[3, cap]`` (SoA: the rule wants three contiguous columns
and the cut reads only ``ts``). A pushed batch becomes one *chunk*, a run sorted by (ts, arrival)
appended at the arena's tail; the host keeps ``[offset, head, n]`` per chunk and the bounds
``tmin_live`` / ``tmax_seen``. A release moves the chunks' heads and never a retained row: retained
rows move only in a consolidation (more than `max_chunks` live chunks, a full arena, a restore),
which collects every live row, sorts stably by ts and gathers into a fresh arena as one chunk.

The same code runs both devices: on "cpu" the three kernels are their C++ twins
(csrc/reorder_cpu.cpp) and the radix sort is a stable host sort.
"""
from __future__ import annotations

import numpy as np
import torch

from ..ops import kernels as K
from .window_operator import OperatorMetrics


class EventOrderBuffer:
    def __init__(self, device="cpu", capacity: int = 1 << 16, max_chunks: int = 256):
        if isinstance(capacity, bool) or not isinstance(capacity, int) or capacity < 1:
            raise ValueError(f"capacity must be an int >= 1, got {capacity!r}")
        if isinstance(max_chunks, bool) or not isinstance(max_chunks, int) \
                or not 1 <= max_chunks < K.REORDER_MAX_CHUNKS:
            # (one chunk more than max_chunks is live when a consolidation collects them)
            raise ValueError(f"max_chunks must be an int in [1, {K.REORDER_MAX_CHUNKS}), got "
                             f"{max_chunks!r}")
        self.device = K.resolve_device(device)
        self.max_chunks = max_chunks
        self.arena = torch.empty((3, capacity), dtype=torch.int64, device=self.device)
        # word 0: the kernels' error flag; words 1 .. k: a release's cuts (one readback for both)
        self._words = torch.zeros(1 + K.REORDER_MAX_CHUNKS, dtype=torch.int64, device=self.device)
        self.metrics = OperatorMetrics()
        self.wm = K.I64_MIN
        self.consolidations = 0
        self.last_contrib = 0   # chunks that fed the last release (1: the slice path)
        self._clear()

    def _clear(self) -> None:
        self.chunks: list = []          # [offset, head, n]: live rows offset + head .. offset + n
        self.tail = 0
        self.tmin_live, self.tmax_seen = K.I64_MAX, K.I64_MIN

    @property
    def cap(self) -> int:
        return self.arena.shape[1]

    @property
    def rows_buffered(self) -> int:
        return sum(n - h for _, h, n in self.chunks)

    @property
    def _err(self) -> torch.Tensor:
        return self._words[:1]

    def _columns(self, cols, names) -> int:
        n = cols[0].numel()
        for c, name in zip(cols, names):
            if c.dtype != torch.int64 or c.dim() != 1 or c.numel() != n:
                raise TypeError(f"{name}: int64 column of the batch's length expected")
            if c.device != self.device:
                raise ValueError(f"{name}: on {c.device}, expected {self.device}")
        return n

    # ---- elements ---------------------------------------------------------------------------
    def push(self, keys, ts, bits, bounds: tuple | None = None) -> None:
        """A batch in arrival order (key ids, timestamps, value bits; int64 columns on the
        buffer's device) becomes one chunk; its rows with ``ts <= wm`` are late: dropped and
        counted in ``metrics.num_late_records_dropped``. `bounds` = (smallest, largest timestamp)
        when the caller has read them: then the only readback is the late count, and only when
        the smallest timestamp is at or behind the watermark. Timestamps lie strictly inside
        (-2**62, 2**62). An empty batch launches nothing."""
        n = self._columns((keys, ts, bits), ("keys", "ts", "bits"))
        if n == 0:
            return
        late = 0
        if bounds is None:
            tmin, tmax, late = torch.stack([ts.min(), ts.max(), (ts <= self.wm).sum()]).tolist()
        else:
            tmin, tmax = (int(b) for b in bounds)
            if tmin <= self.wm:
                late = int((ts <= self.wm).sum().item())
        if tmin <= -K.SUSTAIN_TS_LIMIT or tmax >= K.SUSTAIN_TS_LIMIT:
            raise TypeError("reorder: a timestamp at or beyond 2**62")
        self.metrics.num_records_in += n
        self.metrics.num_late_records_dropped += late
        if late < n:
            self._append(keys.contiguous(), ts.contiguous(), bits.contiguous(), n - late,
                         tmin, tmax)

    def _append(self, keys, ts, bits, live: int, tmin: int, tmax: int) -> None:
        """The batch's `live` rows behind the watermark, sorted by (ts, arrival), to the tail."""
        n = ts.numel()
        lo = max(tmin, self.wm + 1)
        span = tmax - lo
        if n == 1:
            perm = torch.zeros(1, dtype=torch.int64, device=self.device)
        else:
            key = ts - lo
            if live < n:
                key.masked_fill_(ts <= self.wm, span + 1)   # late rows sort last
            idx = torch.arange(n, dtype=torch.int64, device=self.device)
            perm = K.sort_pairs(key, idx, bits=max(1, (span + 1).bit_length()))[1]
        if self.tail + live > self.cap:
            self._consolidate(extra=live)
        t = self.tail
        K.reorder_gather(perm[:live], (keys, ts, bits), n,
                         tuple(self.arena[c, t:t + live] for c in range(3)), self._err)
        self.chunks.append([t, 0, live])
        self.tail = t + live
        self.tmin_live, self.tmax_seen = min(self.tmin_live, lo), max(self.tmax_seen, tmax)
        if len(self.chunks) > self.max_chunks:
            self._consolidate()

    def _collect_sorted(self, begins, counts, lo: int, hi: int) -> torch.Tensor:
        """Arena indices of the chunks' rows ``[begin, begin + count)`` in (ts, arrival) order:
        collected in chunk order, then one stable radix sort over the bits of ``hi - lo``."""
        key, src = K.reorder_collect(self.arena[1], self.tail, begins, counts, lo, self._err)
        if len(begins) == 1:
            return src   # one chunk is sorted already
        return K.sort_pairs(key, src, bits=max(1, (hi - lo).bit_length()))[1]

    def _consolidate(self, extra: int = 0) -> None:
        """Every live row into a fresh arena as one chunk; the arena doubles until the live rows
        fill at most half of it and `extra` more rows fit. The only place retained rows move."""
        live = self.rows_buffered
        cap = self.cap
        while live + extra > cap or 2 * live > cap:
            cap *= 2
        arena = torch.empty((3, cap), dtype=torch.int64, device=self.device)
        if live:
            src = self._collect_sorted([o + h for o, h, _ in self.chunks],
                                       [n - h for _, h, n in self.chunks],
                                       self.tmin_live, self.tmax_seen)
            K.reorder_gather(src, tuple(self.arena[c] for c in range(3)), self.tail,
                             tuple(arena[c, :live] for c in range(3)), self._err)
            self.chunks, self.tail = [[0, 0, live]], live
            self.consolidations += 1
        else:
            self._clear()
        self.arena = arena

    def release(self, w: int):
        """The rows with ``ts <= w`` leave the buffer: three device columns (key ids, timestamps,
        value bits) in (ts, arrival) order, or None when there are none. A `w` at or below the
        current watermark is ignored. When one chunk alone contributes, the columns are slices
        of the arena (no kernel, no sort): the caller must consume them before it touches the
        buffer again, a later push may overwrite them."""
        w = int(w)
        if w <= self.wm:
            return None
        prev, self.wm = self.wm, w
        self.metrics.current_watermark = w
        self.last_contrib = 0
        if not self.chunks:
            return None
        lo, hi = max(prev + 1, self.tmin_live), min(w, self.tmax_seen)
        if hi < lo:
            return None   # nothing can be due: no launch, no readback
        k = len(self.chunks)
        begins = [o + h for o, h, _ in self.chunks]
        K.reorder_cut(self.arena[1], self.tail, begins, [o + n for o, _, n in self.chunks], w,
                      self._words[1:1 + k])
        flag, *cuts = self._words[:1 + k].tolist()   # the one readback: it is the total as well
        self._check_flag(flag)
        counts = [c - b for c, b in zip(cuts, begins)]
        if any(not 0 <= c <= n - h for c, (_, h, n) in zip(counts, self.chunks)):
            raise RuntimeError("reorder: a cut outside its chunk")
        total = sum(counts)
        self.tmin_live = max(self.tmin_live, min(w, K.I64_MAX - 1) + 1)
        if total == 0:
            return None
        contrib = [(b, c) for b, c in zip(begins, counts) if c]
        self.last_contrib = len(contrib)
        if len(contrib) == 1:
            b, c = contrib[0]
            out = tuple(self.arena[j, b:b + c] for j in range(3))
        else:
            src = self._collect_sorted([b for b, _ in contrib], [c for _, c in contrib], lo, hi)
            dst = torch.empty((3, total), dtype=torch.int64, device=self.device)
            K.reorder_gather(src, tuple(self.arena[j] for j in range(3)), self.tail,
                             tuple(dst[j] for j in range(3)), self._err)
            out = tuple(dst[j] for j in range(3))
        for ch, c in zip(self.chunks, counts):
            ch[1] += c
        self.chunks = [ch for ch in self.chunks if ch[1] < ch[2]]
        if not self.chunks:
            self._clear()   # a drained arena starts over at its beginning
        self.metrics.num_fires += 1
        self.metrics.num_records_out += total
        return out

    def _check_flag(self, flag=None) -> None:
        if flag is None:
            flag = int(self._words[0].item())
        if flag:
            raise RuntimeError("reorder: a kernel met an index outside its column")

    # ---- contents ---------------------------------------------------------------------------
    def rows(self):
        """The buffered rows as host arrays (key id, ts, value bits) in arena order."""
        self._check_flag()
        a = self.arena[:, :self.tail].cpu().numpy()
        parts = [a[:, o + h:o + n] for o, h, n in self.chunks]
        a = np.concatenate(parts, axis=1) if parts else np.zeros((3, 0), dtype=np.int64)
        return tuple(np.ascontiguousarray(a[j]) for j in range(3))

    def contents(self):
        """The buffered rows as host arrays in (ts, arrival) order: within equal timestamps the
        arena order is the arrival order."""
        key, ts, bits = self.rows()
        o = np.argsort(ts, kind="stable")
        return key[o], ts[o], bits[o]

    # ---- checkpoints ------------------------------------------------------------------------
    def snapshot_state(self):
        from .checkpoint import OperatorSnapshot

        key, ts, bits = self.rows()
        kg = (K.keygroups(torch.from_numpy(key), max_parallelism=128).numpy()
              if key.size else np.zeros(0, np.int32))
        meta = {"kind": "reorder", "wm": self.wm,
                "late": self.metrics.num_late_records_dropped,
                "metrics": {"num_records_in": self.metrics.num_records_in,
                            "num_records_out": self.metrics.num_records_out,
                            "num_fires": self.metrics.num_fires}}
        cols = {"key": key, "ts": ts, "bits": bits, "ord": np.arange(key.size, dtype=np.int64)}
        return OperatorSnapshot(kg, cols, meta)

    def restore_state(self, rows: dict, meta: dict) -> None:
        if meta.get("kind") != "reorder":
            raise ValueError("checkpoint of a different operator (not a reorder buffer)")
        col = lambda name: np.ascontiguousarray(  # noqa: E731
            rows.get(name, np.zeros(0, np.int64)), dtype=np.int64)
        key, ts, bits, rank = col("key"), col("ts"), col("bits"), col("ord")
        if not key.size == ts.size == bits.size == rank.size:
            raise ValueError("checkpoint with columns of different lengths")
        wm = meta.get("wm", K.I64_MIN)
        if ts.size and (int(ts.min()) <= max(wm, -K.SUSTAIN_TS_LIMIT)
                        or int(ts.max()) >= K.SUSTAIN_TS_LIMIT):
            raise ValueError("checkpoint with a row at or behind its watermark, or beyond 2**62")
        self._clear()
        self.wm = wm
        self.metrics.current_watermark = wm
        self.metrics.num_late_records_dropped = meta.get("late", 0)
        for k, v in meta.get("metrics", {}).items():
            setattr(self.metrics, k, v)
        if ts.size:
            # Key groups arrive in any order: `ord` puts the rows back in arena order, where
            # equal timestamps are in arrival order; one chunk holds them all.
            o = np.argsort(rank, kind="stable")
            dev = lambda x: torch.from_numpy(np.ascontiguousarray(x[o])).to(self.device)  # noqa: E731
            self._append(dev(key), dev(ts), dev(bits), int(ts.size), int(ts.min()),
                         int(ts.max()))
