"""Keyed state machines (``stream.key_by(k).process(StateMachineAlert(field, bounds, table,
initial, report))``).

Every key runs one finite state machine: an element's class is the number of `bounds` its value
reaches, the key moves ``to = table[from][class]``, and a reported pair (from, to) gives the row
``(key, from, to, since, value)``, `since` being the timestamp at which the key entered `from`.
A key enters `initial` at its first element. Elements are taken in arrival order; there are no
timers.

State for dense key ids (the operator's dictionary ids for string keys, an integer key itself --
a key at or above ``dense_limit`` is refused): ``state int64[cap, 2]`` = (since, state), since
INT64_MIN while the key was never seen. The capacity doubles to cover a batch's largest key id.

``process`` is one ``fsm_update``: a stable radix sort by key, one segmented wave scan of the
elements' transition functions, packed 4 bits per state (csrc/mxs_fsm.h has the algebra), the
rows' count read back and the rows put in arrival order. The code column is ``from << 4 | to``.
CPU (device="cpu") runs the C++ twin (csrc/fsm_cpu.cpp).
"""
from __future__ import annotations

import numpy as np

from ..ops import kernels as K
from .rule_operator import KeyedRuleOperator


class KeyedStateMachineOperator(KeyedRuleOperator):
    kind, what, tables = "state_machine", "state-machine", ("state",)

    def __init__(self, bounds, table, initial: int = 0, report="change", device="cpu",
                 dense_limit: int = 1 << 26, capacity: int = 1024):
        table = [list(r) for r in table]
        if isinstance(report, str):
            if report != "change":
                raise ValueError(f"report must be 'change' or (from, to) pairs, got {report!r}")
            report = [(a, b) for a in range(len(table)) for b in range(len(table)) if a != b]
        self.cuts, self.cols, self.masks = K.fsm_pack(bounds, table, report)
        self.states, self.classes = len(self.masks), len(self.cols)
        if isinstance(initial, bool) or not isinstance(initial, int) \
                or not 0 <= initial < self.states:
            raise ValueError(f"initial must be a state in [0, {self.states}), got {initial!r}")
        self.initial = initial
        self._open(device, dense_limit, capacity)

    def _params(self) -> dict:
        # lists: a checkpoint that went through a text format compares equal
        return {"bounds": list(self.cuts), "cols": list(self.cols), "report": list(self.masks),
                "initial": self.initial}

    def _fresh(self, cap: int):
        return (K.fsm_table(cap, self.device),)

    def _update(self, keys, vals, ts, kind, bounds):
        return K.fsm_update(self.state, keys, vals, ts, kind=kind, cuts=self.cuts,
                            cols=self.cols, report=self.masks, states=self.states,
                            classes=self.classes, initial=self.initial, bounds=bounds)

    def entries(self):
        """Every key seen as host arrays (key id, since, state), ascending by key id."""
        st = self.state.cpu().numpy()
        ids = np.nonzero(st[:, 0] != K.FSM_NONE)[0].astype(np.int64)
        return ids, st[ids, 0].copy(), st[ids, 1].copy()

    # ---- checkpoints ------------------------------------------------------------------------
    def _snapshot_columns(self) -> dict:
        ids, since, state = self.entries()
        return {"key": ids, "since": since, "state": state}

    def _restore_rows(self, ids, col, cap: int):
        since, st = col("since"), col("state")
        if st.size and (int(st.min()) < 0 or int(st.max()) >= self.states):
            raise ValueError("checkpoint with a state the machine does not have")
        if since.size and bool((since == K.FSM_NONE).any()):
            raise ValueError("checkpoint with a key that was never seen")
        state = np.zeros((cap, 2), dtype=np.int64)
        state[:, 0] = K.FSM_NONE
        state[ids, 0], state[ids, 1] = since, st
        return (state,)
