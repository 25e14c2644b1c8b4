"""Keyed window joins (Flink 1.8 ``JoinedStreams``: ``a.join(b).where().equalTo().window().apply``).

Flink tags both inputs with their side, unions them, keys the union by the side's own selector,
windows it and, when a window fires, runs the nested loop over the (key, window)'s left and
right elements. Here each side keeps its elements in a device pane arena of its own (the arena
of the ``process`` windows, runtime/list_window_operator.py); there is one watermark.

A firing gathers both sides into key segments (``_gather_window``: ascending key ids, segment
starts, values as f64 order bits), then

* ``join_match``: every left segment's right segment (binary search) and its pair count nL * nR;
* ``join_scan``: the exclusive 64-bit scan of the counts and the matched segments compacted;
* one readback of the firing's pair total P;
* ``join_expand`` over [p0, p1) in chunks of at most ``pair_chunk`` pairs: three int64 columns
  (key id, left value bits, right value bits), left-major inside a key, keys ascending.

Each chunk is one fired row ``(start, end, keys, lvals, rvals)`` of device tensors; a window in
which one side has no element emits nothing. Tumbling and sliding event-time windows, allowed
lateness 0: an element whose last window is behind the watermark is dropped and counted,
whichever side it arrives on. CPU (device="cpu") runs the C++ twins (csrc/join_cpu.cpp).
"""
from __future__ import annotations

import numpy as np

from ..ops import kernels as K
from .list_window_operator import I64_MAX, I64_MIN, KeyedListWindowOperator
from .window_operator import OperatorMetrics


class KeyedJoinWindowOperator:
    def __init__(self, *, size: int, slide: int | None = None, offset: int = 0, device="cpu",
                 pair_chunk: int = 1 << 24):
        if int(pair_chunk) < 1:
            raise ValueError("pair_chunk must be >= 1")
        slide = size if slide is None else slide
        self.size, self.slide, self.offset = int(size), int(slide), int(offset)
        self.pair_chunk = int(pair_chunk)
        self.device = K.resolve_device(device)
        # One pane arena per side (no window function of theirs is ever run).
        self.arenas = [KeyedListWindowOperator(size=self.size, slide=self.slide, offset=self.offset,
                                               lateness=0, device=self.device)
                       for _ in range(2)]
        self.wm = I64_MIN
        self.metrics = OperatorMetrics()
        self.pairs_out = 0

    def _sync_metrics(self) -> None:
        l, r = (a.metrics for a in self.arenas)
        self.metrics.num_records_in = l.num_records_in + r.num_records_in
        self.metrics.num_late_records_dropped = (l.num_late_records_dropped
                                                 + r.num_late_records_dropped)

    def process(self, side: int, keys, ts, vals_f64) -> list:
        """Append a batch to side 0 (left) or 1 (right): keys int64, ts int64, vals the f64 bit
        patterns (int64). Fires nothing (lateness 0: no late re-firing)."""
        if side not in (0, 1):
            raise ValueError("side must be 0 (left) or 1 (right)")
        self.arenas[side].process(keys, ts, vals_f64)
        self._sync_metrics()
        return []

    def advance_watermark(self, wm: int) -> list:
        """Fire every due window start of either arena's schedule; purge both arenas."""
        if wm <= self.wm:
            return []
        self.wm = wm
        for a in self.arenas:
            a.wm = wm
        out = []
        starts = [a.next_fire_start for a in self.arenas if a.next_fire_start is not None]
        if starts:
            s = min(starts)
            lives = [lv for lv in (a._live_range() for a in self.arenas) if lv is not None]
            last_pane = max(lv[1] for lv in lives) if lives else None
            ctl = self.arenas[0]
            # Windows after the last pane hold no data: never iterate past it (wm may be MAX).
            while s + self.size - 1 <= wm and last_pane is not None \
                    and ctl._pane_of(s) <= last_pane:
                out += self._fire_window(s)
                s += self.slide
            if s + self.size - 1 <= wm:  # caught up: resume at the first window not yet due
                s = ctl._align_up(wm - self.size + 2) if wm < I64_MAX - self.size else s
            for a in self.arenas:
                a.next_fire_start = s
        for a in self.arenas:
            a._purge()
        return out

    def _fire_window(self, s: int) -> list:
        gl = self.arenas[0]._gather_window(s)
        gr = self.arenas[1]._gather_window(s)
        if gl is None or gr is None:
            return []
        lkeys, lheads, kl, ltotal, lord = gl
        rkeys, rheads, kr, rtotal, rord = gr
        jp = K.join_plan(lkeys.contiguous(), lheads[:kl], ltotal, rkeys.contiguous(), rheads[:kr],
                         rtotal, validate=False)
        if jp.pairs == 0:
            return []
        self.metrics.num_fires += 1
        self.metrics.num_records_out += jp.pairs
        self.pairs_out += jp.pairs
        out = []
        for p0 in range(0, jp.pairs, self.pair_chunk):
            p1 = min(jp.pairs, p0 + self.pair_chunk)
            out.append((s, s + self.size) + K.join_expand(jp, lord, rord, p0, p1))
        return out

    # ---- checkpoints ------------------------------------------------------------------------
    def snapshot_state(self):
        """Both arenas' live rows (side, pane, key, f64 bits) + the watermark and fire schedule."""
        from .checkpoint import OperatorSnapshot

        snaps = [a.snapshot_state() for a in self.arenas]
        cols = {name: np.concatenate([sn.columns[name] for sn in snaps])
                for name in ("key", "pane", "val")}
        cols["side"] = np.concatenate([np.full(sn.columns["key"].size, i, dtype=np.int64)
                                       for i, sn in enumerate(snaps)])
        meta = {"kind": "join_window", "size": self.size, "slide": self.slide,
                "offset": self.offset, "wm": self.wm, "pairs_out": self.pairs_out,
                "sides": [sn.meta for sn in snaps],
                "metrics": {"num_records_out": self.metrics.num_records_out,
                            "num_fires": self.metrics.num_fires}}
        return OperatorSnapshot(np.concatenate([sn.kg for sn in snaps]), cols, meta)

    def restore_state(self, rows: dict, meta: dict) -> None:
        if meta.get("kind") != "join_window" or (meta["size"], meta["slide"], meta["offset"]) != \
                (self.size, self.slide, self.offset):
            raise ValueError("checkpoint of a different join window")
        side = np.asarray(rows.get("side", np.zeros(0, np.int64)), dtype=np.int64)
        for i, a in enumerate(self.arenas):
            sel = side == i
            a.restore_state({name: np.asarray(rows[name])[sel] for name in ("key", "pane", "val")}
                            if side.size else {}, meta["sides"][i])
        self.wm = meta["wm"]
        self.pairs_out = meta.get("pairs_out", 0)
        for k, v in meta.get("metrics", {}).items():
            setattr(self.metrics, k, v)
        self._sync_metrics()
