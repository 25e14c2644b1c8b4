"""Validated launch wrappers around the native kernels.

Every wrapper checks dtype, device, contiguity and the sizes the kernel's grid assumes BEFORE
launching (a mis-shaped operand must never reach a hand-written kernel), then dispatches to the
gfx950 kernel for CUDA(HIP) tensors or to the C++ twin for CPU tensors. There is no Python
fallback: a missing extension raises.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from . import expr as _expr
from .native import load

REC_WORDS = 3  # 24-byte record = 3 x int64 words
STAT_COUNT = 8
STAT_MAXTS, STAT_MINPANE, STAT_MAXPANE, STAT_LATE, STAT_OVERFLOW, STAT_ACCEPTED, STAT_MAXBUCKET = range(7)
AGG_SLICE = 131072  # records per workgroup of a split sub-table (csrc kAggSliceMin)

I64_MIN = -(1 << 63)
I64_MAX = (1 << 63) - 1

# AggKind (csrc/mxs_common.h)
AGG_SUM_I64, AGG_SUM_F64, AGG_MIN_I64, AGG_MAX_I64, AGG_MIN_F64, AGG_MAX_F64, AGG_COUNT, \
    AGG_AVG_F64, AGG_AVG_I64 = range(9)
AGG_IS_F64 = {AGG_SUM_F64, AGG_MIN_F64, AGG_MAX_F64, AGG_AVG_F64}


def _is_gpu(t: torch.Tensor) -> bool:
    return t.device.type == "cuda"


def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def _p(t: torch.Tensor | None) -> int:
    return 0 if t is None else t.data_ptr()


def resolve_device(d) -> torch.device:
    """torch.device with an explicit index: a bare 'cuda' means the current device (operators
    compare tensor devices against theirs, and tensors always carry the index)."""
    d = torch.device(d)
    if d.type == "cuda" and d.index is None:
        return torch.device("cuda", torch.cuda.current_device())
    return d


def _check(t: torch.Tensor, dtype: torch.dtype, numel_min: int, name: str, dev: torch.device):
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    if t.numel() < numel_min:
        raise ValueError(f"{name}: needs >= {numel_min} elements, has {t.numel()}")
    if t.device != dev and t.device != resolve_device(dev):
        raise ValueError(f"{name}: on {t.device}, expected {dev}")


def new_stats(device) -> torch.Tensor:
    s = torch.zeros(STAT_COUNT, dtype=torch.int64, device=device)
    s[STAT_MAXTS] = I64_MIN
    s[STAT_MINPANE] = I64_MAX
    s[STAT_MAXPANE] = I64_MIN
    return s


def reset_stats(s: torch.Tensor) -> None:
    init = torch.tensor([I64_MIN, I64_MAX, I64_MIN, 0, 0, 0, 0, 0], dtype=torch.int64)
    s.copy_(init, non_blocking=False)


def gen_events(keys, ts, vals, *, seed: int, stream_id: int, idx0: int, nkeys: int,
               ts_base: int, ts_span: int, disorder: int, val_lo: int, val_span: int,
               val_f64: bool = False, zipf: float = 0.0, key_base: int = 0) -> None:
    """keys: int64, or int32 (dictionary ids, nkeys < 2^31). zipf > 0: power-law skewed keys
    with that exponent (key 0 hottest; csrc/mxs_common.h zipf_key), 0: uniform. key_base: added
    to every key (a drifting key window without a separate pass)."""
    n = keys.numel()
    dev = keys.device
    key32 = keys.dtype == torch.int32
    _check(keys, torch.int32 if key32 else torch.int64, n, "keys", dev)
    _check(ts, torch.int64, n, "ts", dev)
    _check(vals, torch.int64, n, "vals", dev)
    if nkeys <= 0 or nkeys >= (1 << (31 if key32 else 63)):
        raise ValueError("nkeys out of range")
    m = load()
    args = (_p(keys), _p(ts), _p(vals), n, seed & (2**64 - 1), stream_id & (2**64 - 1), idx0,
            nkeys, ts_base, ts_span, disorder, val_lo, val_span, int(val_f64) | (2 if key32 else 0),
            float(zipf))
    if zipf < 0:
        raise ValueError("zipf exponent must be >= 0")
    if key_base < 0:
        raise ValueError("key_base must be >= 0")
    if _is_gpu(keys):
        m.gpu_gen_events(*args, _stream(keys), key_base)
    else:
        m.cpu_gen_events(*args, key_base)


@dataclass
class PartitionPlan:
    """keyBy + window assignment plan of one step (csrc/mxs_common.h PartPlan)."""

    max_parallelism: int
    nsub_log2: int
    nranks: int
    window_mode: int
    drop_late: int
    hash_mode: int
    bucket_cap: int
    late_ts: int = I64_MIN   # elements with ts < late_ts are late (all windows cleaned)
    tbase: int = 0           # start of the step's base pane
    pane: int = 1            # pane length (ms)
    ablate: int = 0          # profiling-only ablation bits
    rec_words: int = 3       # 3: 24-byte records; 2: 16-byte records (int32 values, window path)
    dense_bits: int = 0      # > 0: dense key ids < 2^dense_bits, directly addressed
    dense_mul: int = 0       # odd multiplier of the dense slot bijection
    key32: int = 0           # 1: int32 key column (compact-record GPU partition only)
    scratch: int = 0         # GPU two-level partition (> 512 buckets): coarse staging buffer
    scratch_cursor: int = 0  # ... and its 512 coarse cursors (data pointers; 0 = plain scatter)

    @property
    def nbuckets(self) -> int:
        return self.nranks << self.nsub_log2

    def as_dict(self) -> dict:
        return dict(self.__dict__)


def partition(keys, ts, vals, plan: PartitionPlan, kg_dest, cursor, out, stats,
              jhash=None, late_idx=None) -> None:
    n = keys.numel()
    dev = keys.device
    nb = plan.nbuckets
    _check(keys, torch.int64, n, "keys", dev)
    _check(ts, torch.int64, n, "ts", dev)
    _check(vals, torch.int64, n, "vals", dev)
    _check(kg_dest, torch.int32, plan.max_parallelism, "kg_dest", dev)
    _check(cursor, torch.int32, nb, "cursor", dev)
    _check(out, torch.int64, nb * plan.bucket_cap * REC_WORDS, "out", dev)
    _check(stats, torch.int64, STAT_COUNT, "stats", dev)
    if plan.hash_mode:
        if jhash is None:
            raise ValueError("hash_mode=1 needs the dictionary jhash table")
        _check(jhash, torch.int32, 1, "jhash", dev)
    if nb > 16384:
        raise ValueError("too many buckets (ranks x sub-tables > 16384)")
    if n >= (1 << 32):
        raise ValueError("batch too large (2^32 events)")
    late_cap = 0 if late_idx is None else late_idx.numel()
    if late_idx is not None:
        _check(late_idx, torch.int32, 0, "late_idx", dev)
    m = load()
    args = (_p(keys), _p(ts), _p(vals), _p(jhash), n, plan.as_dict(), _p(kg_dest), _p(cursor),
            _p(out), _p(stats), _p(late_idx), late_cap)
    if _is_gpu(keys):
        m.gpu_partition(*args, _stream(keys))
    else:
        m.cpu_partition(*args)


@dataclass
class AggPlan:
    cap_log2: int
    nsub: int
    ring: int
    agg: int
    nsrc: int
    bucket_cap: int
    np_step: int
    pg: int
    pane_base: int
    p_lo: int
    fired_hi: int
    combined: int = 0    # records are pre-aggregated by window_combine (aux = element count)
    rec_words: int = 3   # layout of the input records (3: Rec, 2: RecC)
    dlist: int = 0       # touched-slot list (data pointers, 0 = off): slot ids ...
    dlist_n: int = 0     # ... its length ...
    slot_mark: int = 0   # ... and the per-slot listed marks
    dense_bits: int = 0  # > 0: directly addressed dense key ids (see PartitionPlan)
    dense_mul: int = 0
    split: int = 1       # workgroups sharing an oversized sub-table (hot keys; GPU, see AGG_SLICE)
    det: int = 0         # 1: deterministic f64 sums (128-bit fixed-point per-step slot sums)
    dacc: int = 0        # local-global delta ring of late data (data pointers, 0 = off) ...
    dcnt: int = 0        # ... and its counts
    skip: int = 0        # device int64: non-zero -> leave the state untouched (incomplete exchange)
    pmask: int = 0       # GPU: relative panes with records (sparse pane rows; np_step = popcount)

    def as_dict(self) -> dict:
        return dict(self.__dict__)


def window_combine(recs, counts, plan: AggPlan, out, ccap: int, out_counts, flags) -> None:
    """Sender-side combiner: one pre-aggregated record per (key, pane) of every send bucket.
    `plan.nsub` here is the number of send buckets (ranks x sub-tables)."""
    dev = recs.device
    nb = plan.nsub
    _check(recs, torch.int64, nb * plan.bucket_cap * REC_WORDS, "recs", dev)
    _check(counts, torch.int32, nb, "counts", dev)
    _check(out, torch.int64, nb * ccap * REC_WORDS, "out", dev)
    _check(out_counts, torch.int32, nb, "out_counts", dev)
    _check(flags, torch.int32, 1, "flags", dev)
    if (1 << plan.cap_log2) * 8 + plan.pg * (1 << plan.cap_log2) * 12 + 16 > 160 * 1024:
        raise ValueError("window_combine: LDS plan too large")
    m = load()
    args = (_p(recs), _p(counts), nb, plan.as_dict(), _p(out), int(ccap), _p(out_counts), _p(flags))
    if _is_gpu(recs):
        m.gpu_window_combine(*args, _stream(recs))
    else:
        m.cpu_window_combine(*args)


def window_agg(recs, counts, plan: AggPlan, keys_g, acc_g, cnt_g, dirty_g, occ, flags) -> None:
    dev = keys_g.device
    nslots = plan.nsub << plan.cap_log2
    _check(recs, torch.int64, plan.nsrc * plan.nsub * plan.bucket_cap * REC_WORDS, "recs", dev)
    _check(counts, torch.int32, plan.nsrc * plan.nsub, "counts", dev)
    _check(keys_g, torch.int64, nslots, "keys_g", dev)
    _check(acc_g, torch.int64, plan.ring * nslots, "acc_g", dev)
    _check(cnt_g, torch.int32, plan.ring * nslots, "cnt_g", dev)
    _check(dirty_g, torch.uint8, plan.ring * nslots, "dirty_g", dev)
    _check(occ, torch.int32, plan.nsub, "occupancy", dev)
    _check(flags, torch.int32, 1, "flags", dev)
    if plan.np_step > plan.ring:
        raise ValueError("step touches more panes than the ring holds")
    m = load()
    args = (_p(recs), _p(counts), plan.as_dict(), _p(keys_g), _p(acc_g), _p(cnt_g), _p(dirty_g),
            _p(occ), _p(flags))
    if _is_gpu(keys_g):
        m.gpu_window_agg(*args, _stream(keys_g))
    else:
        m.cpu_window_agg(*args)


def window_fire(keys_g, acc_g, cnt_g, dirty_g, *, agg: int, npanes: int, ring: int, p0: int,
                wstart: int, wend: int, only_dirty: bool, map_prog: _expr.Program,
                filt_prog: _expr.Program, out_keys, out_vals, out_raw, out_cnt, out_n,
                ablate: int = 0, slot_list=None, slot_list_n=None, key32: bool = False) -> None:
    """slot_list/slot_list_n (int32 device tensors): visit only the listed slots (re-firings of
    late-but-allowed data) instead of sweeping the table. Compact rows: out_raw / out_cnt None
    (not written) and key32 (keys < 2^32 written as uint32 into out_keys' first 4*n bytes)."""
    dev = keys_g.device
    nslots = keys_g.numel()
    cap = out_keys.numel()
    _check(acc_g, torch.int64, ring * nslots, "acc_g", dev)
    _check(cnt_g, torch.int32, ring * nslots, "cnt_g", dev)
    _check(dirty_g, torch.uint8, ring * nslots, "dirty_g", dev)
    _check(out_vals, torch.float64, cap, "out_vals", dev)
    if out_raw is not None:
        _check(out_raw, torch.int64, cap, "out_raw", dev)
    if out_cnt is not None:
        _check(out_cnt, torch.int32, cap, "out_cnt", dev)
    _check(out_n, torch.int32, 1, "out_n", dev)
    if npanes > ring:
        raise ValueError("window spans more panes than the ring")
    plan = dict(agg=agg, npanes=npanes, ring=ring, only_dirty=int(only_dirty), nslots=nslots,
                p0=p0, wstart=float(wstart), wend=float(wend), out_cap=cap,
                map=tuple(map_prog.as_args()), filt=tuple(filt_prog.as_args()), ablate=ablate,
                key32=int(key32))
    if slot_list is not None:
        _check(slot_list, torch.int32, 0, "slot_list", dev)
        _check(slot_list_n, torch.int32, 1, "slot_list_n", dev)
        plan.update(list=_p(slot_list), list_n=_p(slot_list_n))
    m = load()
    args = (_p(keys_g), _p(acc_g), _p(cnt_g), _p(dirty_g), plan, _p(out_keys), _p(out_vals),
            0 if out_raw is None else _p(out_raw), 0 if out_cnt is None else _p(out_cnt),
            _p(out_n))
    if _is_gpu(keys_g):
        m.gpu_window_fire(*args, _stream(keys_g))
    else:
        m.cpu_window_fire(*args)


def scatter_partials(keys, acc, cnt, n_dev, *, n_cap: int, max_parallelism: int, nranks: int,
                     nsub_log2: int, hash_mode: int, jhash, kg_dest, bucket_cap: int, cursor, out,
                     flags) -> None:
    """Local-global window aggregation: the first min(n_dev[0], n_cap) rows of a local fire
    (key, partial accumulator, count) -> combined records in their owner's (rank, sub-table)
    bucket of `out` (bucket_cap records each; cursor counts). A bucket overflow sets flags bit0
    (the owner's sub-table cannot hold that many keys)."""
    dev = keys.device
    nb = nranks << nsub_log2
    _check(keys, torch.int64, n_cap, "keys", dev)
    _check(acc, torch.int64, n_cap, "acc", dev)
    _check(cnt, torch.int32, n_cap, "cnt", dev)
    _check(n_dev, torch.int32, 1, "n", dev)
    _check(kg_dest, torch.int32, max_parallelism, "kg_dest", dev)
    _check(cursor, torch.int32, nb, "cursor", dev)
    _check(out, torch.int64, nb * bucket_cap * REC_WORDS, "out", dev)
    _check(flags, torch.int32, 1, "flags", dev)
    if hash_mode:
        if jhash is None:
            raise ValueError("hash_mode=1 needs the dictionary jhash table")
        _check(jhash, torch.int32, 1, "jhash", dev)
    if n_cap >= (1 << 32):
        raise ValueError("too many rows")
    plan = dict(max_parallelism=max_parallelism, nranks=nranks, nsub_log2=nsub_log2,
                hash_mode=hash_mode, bucket_cap=bucket_cap, n_cap=n_cap)
    m = load()
    args = (_p(keys), _p(acc), _p(cnt), _p(n_dev), plan, _p(jhash), _p(kg_dest), _p(cursor),
            _p(out), _p(flags))
    if _is_gpu(keys):
        m.gpu_scatter_partials(*args, _stream(keys))
    else:
        m.cpu_scatter_partials(*args)


def dirty_clear(slot_list, slot_list_n, *, ring: int, nslots: int, dirty_g, slot_mark,
                p_lo: int = 0, np_: int | None = None, dacc=None, dcnt=None) -> None:
    """Reset the touched-slot list's dirty bytes (panes p_lo .. p_lo + np_ - 1; default every
    ring pane) and marks -- and the delta ring (dacc/dcnt) of the same slots and panes; the
    caller zeroes the list length afterwards."""
    dev = dirty_g.device
    _check(slot_list, torch.int32, 0, "slot_list", dev)
    _check(slot_list_n, torch.int32, 1, "slot_list_n", dev)
    _check(dirty_g, torch.uint8, ring * nslots, "dirty_g", dev)
    _check(slot_mark, torch.int32, nslots, "slot_mark", dev)
    if dacc is not None:
        _check(dacc, torch.int64, ring * nslots, "dacc", dev)
        _check(dcnt, torch.int32, ring * nslots, "dcnt", dev)
    m = load()
    np_ = ring if np_ is None else max(0, min(int(np_), ring))
    args = (_p(slot_list), _p(slot_list_n), slot_list.numel(), ring, nslots, _p(dirty_g),
            _p(slot_mark), int(p_lo), np_)
    extra = (0, 0) if dacc is None else (_p(dacc), _p(dcnt))
    if _is_gpu(dirty_g):
        m.gpu_dirty_clear(*args, _stream(dirty_g), *extra)
    else:
        m.cpu_dirty_clear(*args, *extra)


def rolling(recs, counts, *, cap_log2: int, nsub: int, agg: int, nsrc: int, bucket_cap: int,
            emit: bool, keys_g, acc_g, cnt_g, occ, flags, out_vals=None) -> None:
    dev = keys_g.device
    nslots = nsub << cap_log2
    _check(recs, torch.int64, nsrc * nsub * bucket_cap * REC_WORDS, "recs", dev)
    _check(counts, torch.int32, nsrc * nsub, "counts", dev)
    _check(keys_g, torch.int64, nslots, "keys_g", dev)
    _check(acc_g, torch.int64, nslots, "acc_g", dev)
    _check(cnt_g, torch.int32, nslots, "cnt_g", dev)
    _check(occ, torch.int32, nsub, "occupancy", dev)
    if emit and out_vals is None:
        raise ValueError("emit needs out_vals")
    plan = dict(cap_log2=cap_log2, nsub=nsub, agg=agg, nsrc=nsrc, bucket_cap=bucket_cap,
                emit=int(emit))
    m = load()
    args = (_p(recs), _p(counts), plan, _p(keys_g), _p(acc_g), _p(cnt_g), _p(occ), _p(flags),
            _p(out_vals))
    if _is_gpu(keys_g):
        m.gpu_rolling(*args, _stream(keys_g))
    else:
        m.cpu_rolling(*args)


def step_begin(cursor: torch.Tensor, stats: torch.Tensor) -> None:
    _check(stats, torch.int64, STAT_COUNT, "stats", cursor.device)
    _check(cursor, torch.int32, cursor.numel(), "cursor", cursor.device)
    m = load()
    if _is_gpu(cursor):
        m.gpu_step_begin(_p(cursor), cursor.numel(), _p(stats), _stream(cursor))
    else:
        m.cpu_step_begin(_p(cursor), cursor.numel(), _p(stats))


RED_WORDS = 16  # [-qmax, qmin, wm, -bucket_ovf, -pane_ovf, -compact_ovf, -table_full, 0, stats[8]]


def step_finish(stats: torch.Tensor, local_maxts: torch.Tensor, red: torch.Tensor, *,
                bound: int, event_mode: bool, proc_now: int,
                flags: torch.Tensor | None = None) -> None:
    """Reduce the partition stats into the step's all-reduce vector (RED_WORDS). With the
    operator's `flags`, red[6] = -(table full): a key that found no slot in a previous
    aggregation surfaces in the step's one host sync."""
    dev = stats.device
    _check(stats, torch.int64, STAT_COUNT, "stats", dev)
    _check(local_maxts, torch.int64, 1, "local_maxts", dev)
    _check(red, torch.int64, RED_WORDS, "red", dev)
    if flags is not None:
        _check(flags, torch.int32, 1, "flags", dev)
    m = load()
    args = (_p(stats), _p(local_maxts), int(bound), int(event_mode), int(proc_now), _p(red),
            _p(flags))
    if _is_gpu(stats):
        m.gpu_step_finish(*args, _stream(stats))
    else:
        m.cpu_step_finish(*args)


def expr_filter_compact(x: torch.Tensor, prog: _expr.Program) -> tuple[torch.Tensor, torch.Tensor]:
    """Indices (int64, input order) of the rows of one f64 column that pass a traced predicate,
    and their number as a 1-element device tensor (the index buffer has x.numel() entries;
    entries past the count are unspecified). No host sync."""
    _check(x, torch.float64, x.numel(), "x", x.device)
    n = x.numel()
    idx = torch.empty(max(n, 1), dtype=torch.int64, device=x.device)
    total = torch.zeros(1, dtype=torch.int64, device=x.device)
    m = load()
    code, consts = prog.as_args()
    if _is_gpu(x):
        scratch = torch.empty(max(1, m.gpu_filter_compact_scratch_bytes(n)), dtype=torch.uint8,
                              device=x.device)
        m.gpu_expr_filter_compact(_p(x), n, code, consts, _p(scratch), _p(idx), _p(total),
                                  _stream(x))
    else:
        m.cpu_expr_filter_compact(_p(x), n, code, consts, _p(idx), _p(total))
    return idx, total


def expr_filter(x: torch.Tensor, prog: _expr.Program) -> torch.Tensor:
    """Evaluate a traced predicate over one f64 column; returns a bool mask."""
    _check(x, torch.float64, x.numel(), "x", x.device)
    keep = torch.empty(x.numel(), dtype=torch.uint8, device=x.device)
    m = load()
    code, consts = prog.as_args()
    if _is_gpu(x):
        m.gpu_expr_filter(_p(x), x.numel(), code, consts, _p(keep), _stream(x))
    else:
        m.cpu_expr_filter(_p(x), x.numel(), code, consts, _p(keep))
    return keep.bool()


def keygroups(keys: torch.Tensor, *, max_parallelism: int, hash_mode: int = 0,
              jhash: torch.Tensor | None = None) -> torch.Tensor:
    """Flink key group of every key (murmur(javaHash) % maxParallelism), int32."""
    dev = keys.device
    _check(keys, torch.int64, keys.numel(), "keys", dev)
    if hash_mode:
        if jhash is None:
            raise ValueError("hash_mode=1 needs the dictionary jhash table")
        _check(jhash, torch.int32, 1, "jhash", dev)
        if keys.numel() and int(keys.max().item()) >= jhash.numel():
            raise ValueError("dictionary id outside the jhash table")
    kg = torch.empty(keys.numel(), dtype=torch.int32, device=dev)
    m = load()
    args = (_p(keys), keys.numel(), int(hash_mode), _p(jhash), int(max_parallelism), _p(kg))
    if _is_gpu(keys):
        m.gpu_keygroups(*args, _stream(keys))
    else:
        m.cpu_keygroups(*args)
    return kg


def table_insert(keys: torch.Tensor, keys_g: torch.Tensor, *, nsub_log2: int,
                 cap_log2: int) -> torch.Tensor:
    """Insert keys into the sub-table hash layout; returns their global slots (-1: table full)."""
    dev = keys.device
    _check(keys, torch.int64, keys.numel(), "keys", dev)
    _check(keys_g, torch.int64, (1 << nsub_log2) << cap_log2, "keys_g", dev)
    if bool(((keys == -1) | (keys == -2)).any()):
        raise ValueError("keys -1 / -2 are reserved (empty / tombstone)")
    slots = torch.empty(keys.numel(), dtype=torch.int64, device=dev)
    m = load()
    args = (_p(keys), keys.numel(), int(nsub_log2), int(cap_log2), _p(keys_g), _p(slots))
    if _is_gpu(keys):
        m.gpu_table_insert(*args, _stream(keys))
    else:
        m.cpu_table_insert(*args)
    return slots


def sort_pairs(keys: torch.Tensor, vals: torch.Tensor, *, bits: int = 64):
    """Stable ascending sort of (uint64 key bits, int64 value) pairs over the low `bits` key bits.
    GPU: the hand-written LSD radix sort (csrc/sort_hip.hip); CPU: torch stable sort."""
    n = keys.numel()
    dev = keys.device
    _check(keys, torch.int64, n, "keys", dev)
    _check(vals, torch.int64, n, "vals", dev)
    if not 1 <= bits <= 64:
        raise ValueError("bits must be in [1, 64]")
    if _is_gpu(keys):
        m = load()
        ko = torch.empty_like(keys)
        vo = torch.empty_like(vals)
        if n:
            need = m.gpu_sort_pairs_temp_bytes(n, 0, bits)
            tmp = torch.empty(max(1, need), dtype=torch.uint8, device=dev)
            m.gpu_sort_pairs(tmp.data_ptr(), tmp.numel(), keys.data_ptr(), ko.data_ptr(),
                             vals.data_ptr(), vo.data_ptr(), n, 0, bits, _stream(keys))
        return ko, vo
    k = keys if bits == 64 else keys & ((1 << bits) - 1)
    # Unsigned order of the 64-bit patterns: flip the sign bit for a signed sort.
    ks = k ^ I64_MIN if bits == 64 else k
    order = torch.sort(ks, stable=True).indices
    return keys[order], vals[order]


def f64_order_bits(v: torch.Tensor) -> torch.Tensor:
    """f64 bit patterns (int64 view) -> u64 bits whose unsigned order is Double.compareTo order."""
    _check(v, torch.int64, v.numel(), "v", v.device)
    o = torch.empty_like(v)
    m = load()
    if _is_gpu(v):
        m.gpu_f64_order_bits(v.data_ptr(), v.numel(), o.data_ptr(), _stream(v))
    else:
        m.cpu_f64_order_bits(v.data_ptr(), v.numel(), o.data_ptr())
    return o


def segment_median(heads: torch.Tensor, ord_bits: torch.Tensor, *, sorted_values: bool = True
                   ) -> torch.Tensor:
    """Median (Java ComputeCpuMiddle semantics) of every segment starting at `heads`.
    sorted_values=False: the values inside a segment are in any order (per-segment selection:
    LDS bitonic sort or radix select, csrc segment_median_select)."""
    dev = ord_bits.device
    _check(heads, torch.int64, heads.numel(), "heads", dev)
    _check(ord_bits, torch.int64, ord_bits.numel(), "ord", dev)
    if heads.numel() and (int(heads[0]) != 0 or int(heads[-1]) >= max(1, ord_bits.numel())):
        raise ValueError("segment heads out of range")
    out = torch.empty(heads.numel(), dtype=torch.float64, device=dev)
    m = load()
    args = (heads.data_ptr(), heads.numel(), ord_bits.numel(), ord_bits.data_ptr(), out.data_ptr())
    name = "segment_median" if sorted_values else "segment_median_select"
    if _is_gpu(ord_bits):
        getattr(m, "gpu_" + name)(*args, _stream(ord_bits))
    else:
        getattr(m, "cpu_" + name)(*args)
    return out


MAX_QUANTILES = 8
PPM_ONE = 1_000_000


def check_ppm(ppm) -> tuple:
    """1..8 quantiles in parts per million, each an integer in 0..1_000_000."""
    ppm = tuple(ppm)
    if not 1 <= len(ppm) <= MAX_QUANTILES:
        raise ValueError(f"1 to {MAX_QUANTILES} quantiles per window, got {len(ppm)}")
    for p in ppm:
        if isinstance(p, bool) or not hasattr(p, "__index__") or not 0 <= int(p) <= PPM_ONE:
            raise ValueError(f"quantile in parts per million must be an integer in 0..{PPM_ONE}: {p!r}")
    return tuple(int(p) for p in ppm)


def segment_quantiles(heads: torch.Tensor, ord_bits: torch.Tensor, ppm) -> torch.Tensor:
    """Nearest-rank quantiles of every segment of unsorted order bits starting at `heads`:
    float64 [Q, nseg], row j = the element at sorted index clamp(ceil(n * ppm[j] / 1e6) - 1, 0,
    n - 1) of each segment (the element itself; 0.0 for an empty segment)."""
    ppm = check_ppm(ppm)
    dev = ord_bits.device
    _check(heads, torch.int64, heads.numel(), "heads", dev)
    _check(ord_bits, torch.int64, ord_bits.numel(), "ord", dev)
    if heads.numel() and (int(heads[0]) != 0 or int(heads[-1]) >= max(1, ord_bits.numel())):
        raise ValueError("segment heads out of range")
    out = torch.empty((len(ppm), heads.numel()), dtype=torch.float64, device=dev)
    m = load()
    args = (heads.data_ptr(), heads.numel(), ord_bits.numel(), ord_bits.data_ptr(), list(ppm),
            out.data_ptr())
    if _is_gpu(ord_bits):
        m.gpu_segment_quantile_select(*args, _stream(ord_bits))
    else:
        m.cpu_segment_quantile_select(*args)
    return out


TOPN_SOURCES = {"value": 0, "raw": 1, "count": 2}  # csrc/mxs_common.h TopSrc


def topn_source(agg: int, has_map: bool) -> str:
    """The order-word source of a window operator's top-N cut (csrc/mxs_common.h topn_source)."""
    code = load().topn_source(int(agg), bool(has_map))
    return next(k for k, v in TOPN_SOURCES.items() if v == code)


def topn_select(keys: torch.Tensor, vals: torch.Tensor, raw: torch.Tensor | None,
                cnt: torch.Tensor | None, bounds: torch.Tensor, *, n: int, source: str = "value",
                smallest: bool = False):
    """Top-N candidates of fired windows, cut on the input's device without a host read.

    The columns hold ``bounds.numel()`` windows back to back; ``bounds[w]`` (int32, device) = rows
    of windows 0..w, rows past the columns' length do not exist. keys: int64, or int32 (the
    ``emit="key_value"`` layout); vals: float64; raw (int64) / cnt (int32) may be None unless
    they are the order `source` ("value": Double.compare order of vals, "raw": signed int64,
    "count"). A window's candidates are its rows whose order word is >= its n-th largest (with
    `smallest`: <= its n-th smallest) -- every row tying at the threshold included, all rows of a
    window with <= n rows. Returns (keys, vals, raw, cnt, out_bounds): columns of the inputs'
    capacity holding the candidates contiguous in window order (any order inside a window) and
    their cumulative bounds."""
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise ValueError("topn_select: n must be an int >= 1")
    if source not in TOPN_SOURCES:
        raise ValueError(f"topn_select: source must be one of {sorted(TOPN_SOURCES)}")
    dev = keys.device
    key32 = keys.dtype == torch.int32
    cap = keys.numel()
    nwin = bounds.numel()
    m = load()
    _check(keys, torch.int32 if key32 else torch.int64, cap, "keys", dev)
    _check(vals, torch.float64, cap, "vals", dev)
    if raw is not None:
        _check(raw, torch.int64, cap, "raw", dev)
    if cnt is not None:
        _check(cnt, torch.int32, cap, "cnt", dev)
    _check(bounds, torch.int32, nwin, "bounds", dev)
    if source == "raw" and raw is None:
        raise ValueError("topn_select: source 'raw' needs the raw column")
    if source == "count" and cnt is None:
        raise ValueError("topn_select: source 'count' needs the cnt column")
    if nwin > m.TOPN_MAX_WIN:
        raise ValueError(f"topn_select: at most {m.TOPN_MAX_WIN} windows a call")
    if cap >= 1 << 32:
        raise ValueError("topn_select: columns must hold fewer than 2^32 rows")
    okeys, ovals = torch.empty_like(keys), torch.empty_like(vals)
    oraw = None if raw is None else torch.empty_like(raw)
    ocnt = None if cnt is None else torch.empty_like(cnt)
    obounds = torch.zeros_like(bounds)
    if nwin == 0:
        return okeys, ovals, oraw, ocnt, obounds
    cols = (_p(keys), _p(vals), _p(raw), _p(cnt))
    out = (_p(okeys), _p(ovals), _p(oraw), _p(ocnt))
    plan = (TOPN_SOURCES[source], bool(smallest), key32, nwin, min(n, 1 << 62), cap)
    if _is_gpu(keys):
        scratch = torch.empty(m.topn_scratch_bytes(nwin) // 4, dtype=torch.int32, device=dev)
        m.gpu_topn_select(cols, _p(bounds), plan, out, _p(obounds), _p(scratch), _stream(keys))
    else:
        m.cpu_topn_select(cols, _p(bounds), plan, out, _p(obounds))
    return okeys, ovals, oraw, ocnt, obounds


def segment_distinct_launch(heads: torch.Tensor, nseg: int, total: int, ord_bits: torch.Tensor):
    """Launch the distinct count of the `nseg` segments of `ord_bits[:total]` (operands already
    validated). Returns (int64 [nseg] counts, meta): `meta` is the device error word holder to
    pass to ``segment_distinct_check`` after the caller's next readback (None on the CPU).

    GPU: segments of up to 1024 words are counted in LDS by one pass; longer ones are listed by
    it, and only when `total` allows one to exist are (n_long, scratch words) read back (one
    small D2H), the scratch (2 words per element of the long segments, never 2 * total)
    allocated and filled with the empty marker, and the second pass launched."""
    dev = ord_bits.device
    out = torch.empty(nseg, dtype=torch.int64, device=dev)
    if not nseg:
        return out, None
    m = load()
    if not _is_gpu(ord_bits):
        m.cpu_segment_distinct_count(heads.data_ptr(), nseg, total, ord_bits.data_ptr(),
                                     out.data_ptr())
        return out, None
    st = _stream(ord_bits)
    list_cap = max(1, total // (m.DISTINCT_LDS + 1))
    buf = torch.zeros(m.DISTINCT_META + list_cap * m.DISTINCT_ENTRY, dtype=torch.int64, device=dev)
    meta, lst = buf[:m.DISTINCT_META], buf[m.DISTINCT_META:]
    m.gpu_segment_distinct_short(heads.data_ptr(), nseg, total, ord_bits.data_ptr(), out.data_ptr(),
                                 lst.data_ptr(), list_cap, meta.data_ptr(), st)
    if total > m.DISTINCT_LDS:
        cursor, err = meta.tolist()
        n_long, words = cursor >> m.DISTINCT_WORD_BITS, cursor & ((1 << m.DISTINCT_WORD_BITS) - 1)
        if err or n_long > list_cap or words > 2 * total:
            raise RuntimeError(f"segment_distinct: long-segment list overflow ({n_long} segments, "
                               f"{words} words, error word {err})")
        if n_long:
            scratch = torch.full((words,), -1, dtype=torch.int64, device=dev)  # the empty marker
            m.gpu_segment_distinct_long(heads.data_ptr(), nseg, total, ord_bits.data_ptr(),
                                        lst.data_ptr(), n_long, words // 2, scratch.data_ptr(),
                                        out.data_ptr(), meta.data_ptr(), st)
    return out, meta


def segment_distinct_check(meta) -> None:
    """Raise if a probe loop of the distinct kernels hit its bound (tables are at most half
    full, so it never should): the counts of that launch are not to be trusted."""
    if meta is not None:
        err = int(meta[load().DISTINCT_ERR])
        if err:
            raise RuntimeError(f"segment_distinct: probe bound hit (error word {err})")


def segment_distinct(heads: torch.Tensor, ord_bits: torch.Tensor) -> torch.Tensor:
    """Number of different 64-bit words in every segment of `ord_bits` starting at `heads`
    (words in any order, any 64-bit pattern): int64 [nseg], exact; 0 for an empty segment."""
    dev = ord_bits.device
    _check(heads, torch.int64, heads.numel(), "heads", dev)
    _check(ord_bits, torch.int64, ord_bits.numel(), "ord", dev)
    if heads.numel() and (int(heads[0]) != 0 or int(heads[-1]) >= max(1, ord_bits.numel())):
        raise ValueError("segment heads out of range")
    if heads.numel() > 1 and bool((heads[1:] < heads[:-1]).any()):
        raise ValueError("segment heads must ascend")
    out, meta = segment_distinct_launch(heads, heads.numel(), ord_bits.numel(), ord_bits)
    segment_distinct_check(meta)
    return out


# ---- keyed window joins (csrc/mxs_join.h) ------------------------------------------------------

@dataclass
class JoinPlan:
    """A matched and scanned pair of gathered firings (``join_plan``): what ``join_expand``
    needs to write any range of the firing's P pairs."""
    lkeys: torch.Tensor
    lheads: torch.Tensor
    ltotal: int
    rkeys: torch.Tensor
    rheads: torch.Tensor
    rtotal: int
    match: torch.Tensor     # int64 [kL]: the right segment of each left segment, or -1
    cnt: torch.Tensor       # int64 [kL]: nL * nR
    pair_off: torch.Tensor  # int64 [kL + 1]: exclusive scan of cnt, pair_off[kL] = P
    plan: torch.Tensor      # int64 [JOIN_PLAN_COLS * (kL + 1)]: the matched segments, compacted
    pairs: int              # P
    matched: int            # m


def _join_side(keys, heads, total: int, name: str, dev, validate: bool):
    _check(keys, torch.int64, 0, name + "keys", dev)
    _check(heads, torch.int64, keys.numel(), name + "heads", dev)
    if keys.dim() != 1 or heads.dim() != 1 or heads.numel() != keys.numel():
        raise ValueError(f"{name}keys / {name}heads: one start per key segment expected")
    if total < 0 or (keys.numel() == 0) != (total == 0):
        raise ValueError(f"{name}total: {total} elements in {keys.numel()} segments")
    if validate and keys.numel():
        if int(heads[0]) != 0 or int(heads[-1]) >= total or \
                (heads.numel() > 1 and bool((heads[1:] <= heads[:-1]).any())):
            raise ValueError(f"{name}heads: segment starts must ascend from 0 below {name}total")
        if keys.numel() > 1 and bool((keys[1:] <= keys[:-1]).any()):
            raise ValueError(f"{name}keys: key ids must ascend strictly")


def join_plan(lkeys: torch.Tensor, lheads: torch.Tensor, ltotal: int, rkeys: torch.Tensor,
              rheads: torch.Tensor, rtotal: int, *, validate: bool = True) -> JoinPlan:
    """Match the key segments of two gathered firings and scan the pair counts: every left
    segment's right segment (binary search in `rkeys`) and nL * nR, the exclusive 64-bit scan
    ``pair_off`` and the compacted plan of the matched segments. One readback (P, m, the error
    word); a firing of 2**62 pairs or more raises OverflowError."""
    dev = lkeys.device
    ltotal, rtotal = int(ltotal), int(rtotal)
    _join_side(lkeys, lheads, ltotal, "l", dev, validate)
    _join_side(rkeys, rheads, rtotal, "r", dev, validate)
    m = load()
    kl, kr = lkeys.numel(), rkeys.numel()
    cuda = _is_gpu(lkeys)
    st = _stream(lkeys) if cuda else 0
    match = torch.empty(kl, dtype=torch.int64, device=dev)
    cnt = torch.empty(kl, dtype=torch.int64, device=dev)
    pair_off = torch.empty(kl + 1, dtype=torch.int64, device=dev)
    plan = torch.empty(m.JOIN_PLAN_COLS * (kl + 1), dtype=torch.int64, device=dev)
    meta = torch.zeros(m.JOIN_META, dtype=torch.int64, device=dev)
    scratch = torch.empty(max(16, m.join_scan_scratch_bytes(kl)), dtype=torch.uint8, device=dev)
    sides = (lkeys.data_ptr(), lheads.data_ptr(), kl, ltotal,
             rkeys.data_ptr(), rheads.data_ptr(), kr, rtotal)
    m.join_match(cuda, *sides, match.data_ptr(), cnt.data_ptr(), st)
    m.join_scan(cuda, *sides, match.data_ptr(), cnt.data_ptr(), scratch.data_ptr(),
                pair_off.data_ptr(), plan.data_ptr(), meta.data_ptr(), st)
    pairs, matched, err, _ = meta.tolist()
    if err or pairs >= m.JOIN_MAX_PAIRS:
        raise OverflowError("window join: a firing of 2**62 pairs or more")
    return JoinPlan(lkeys, lheads, ltotal, rkeys, rheads, rtotal, match, cnt, pair_off, plan,
                    pairs, matched)


def _pair_range(p0: int, p1: int, pairs: int) -> None:
    """[p0, p1) must lie inside the plan's [0, pairs)."""
    if not 0 <= p0 <= p1 <= pairs:
        raise ValueError(f"pair range [{p0}, {p1}) outside [0, {pairs})")


def _pair_columns(ncols: int, n: int, dev):
    """`ncols` int64 output columns of n rows, every one 16-byte aligned (the expand kernels'
    paired stores): the rows of one tensor whose row length is n rounded up to even."""
    return torch.empty((ncols, n + (n & 1)), dtype=torch.int64, device=dev)[:, :n].unbind(0)


def join_expand(jp: JoinPlan, lord: torch.Tensor, rord: torch.Tensor, p0: int, p1: int):
    """Pairs [p0, p1) of the planned firing as three int64 columns of p1 - p0 rows: the key id,
    the left value's and the right value's f64 bit patterns (`lord` / `rord`: the sides' order
    bits). Position p of a matched key is left-major: a = q / nR, b = q % nR."""
    dev = jp.lkeys.device
    p0, p1 = int(p0), int(p1)
    _check(lord, torch.int64, jp.ltotal, "lord", dev)
    _check(rord, torch.int64, jp.rtotal, "rord", dev)
    _pair_range(p0, p1, jp.pairs)
    ok, ol, orr = _pair_columns(3, p1 - p0, dev)
    if p0 == p1:
        return ok, ol, orr
    m = load()
    if _is_gpu(lord):
        m.gpu_join_expand(jp.plan.data_ptr(), jp.lkeys.numel(), jp.matched, jp.pairs,
                          lord.data_ptr(), rord.data_ptr(), p0, p1, ok.data_ptr(), ol.data_ptr(),
                          orr.data_ptr(), _stream(lord))
    else:
        m.cpu_join_expand(jp.lkeys.data_ptr(), jp.lheads.data_ptr(), jp.lkeys.numel(), jp.ltotal,
                          jp.rkeys.data_ptr(), jp.rheads.data_ptr(), jp.rkeys.numel(), jp.rtotal,
                          jp.match.data_ptr(), jp.pair_off.data_ptr(), lord.data_ptr(),
                          rord.data_ptr(), p0, p1, ok.data_ptr(), ol.data_ptr(), orr.data_ptr())
    return ok, ol, orr


# ---- keyed interval joins (csrc/mxs_ijoin.h) ---------------------------------------------------

def sat_add_i64(a: int, b: int) -> int:
    """a + b saturated at the int64 limits (the interval join's timestamp arithmetic)."""
    return max(I64_MIN, min(I64_MAX, int(a) + int(b)))


def _ijoin_cols(cols, name: str, dev):
    """(key, ts, val) int64 columns of one length."""
    k, t, v = cols
    n = k.numel()
    for c, nm in ((k, "key"), (t, "ts"), (v, "val")):
        _check(c, torch.int64, n, f"{name}.{nm}", dev)
        if c.dim() != 1 or c.numel() != n:
            raise ValueError(f"{name}.{nm}: one word per row expected")
    return n


@dataclass
class IJoinPlan:
    """A probed and scanned batch (``ijoin_plan``): what ``ijoin_expand`` needs to write any range
    of the batch's P pairs."""
    side: int               # the batch's side: 0 = left, 1 = right
    batch: tuple            # (key, ts, val), sorted by (key, ts)
    other: tuple            # the other side's buffer (key, ts, val)
    lb: torch.Tensor        # int64 [n]: the first row of each element's range in `other`
    cnt: torch.Tensor       # int64 [n]: the length of the range
    plan: torch.Tensor      # int64 [IJOIN_PLAN_COLS * (n + 1)]: the non-empty elements, compacted
    pairs: int              # P
    rows: int               # m


def ijoin_probe(bkey: torch.Tensor, bts: torch.Tensor, okey: torch.Tensor, ots: torch.Tensor,
                rlo: int, rhi: int, cutoff: int = I64_MIN):
    """Every batch element's range in the other side's buffer: ``lb`` = the first row >=
    (k, max(t + rlo, cutoff + 1)), ``cnt`` = the rows from there up to (k, t + rhi). Sums
    saturate; rows with ts <= cutoff are expired and never counted."""
    dev = bkey.device
    nb, no = bkey.numel(), okey.numel()
    _check(bkey, torch.int64, nb, "bkey", dev)
    _check(bts, torch.int64, nb, "bts", dev)
    _check(okey, torch.int64, no, "okey", dev)
    _check(ots, torch.int64, no, "ots", dev)
    if bts.numel() != nb or ots.numel() != no:
        raise ValueError("ijoin_probe: one timestamp per key expected")
    for b in (rlo, rhi, cutoff):
        if not I64_MIN <= int(b) <= I64_MAX:
            raise ValueError("ijoin_probe: bounds must be int64")
    lb = torch.empty(nb, dtype=torch.int64, device=dev)
    cnt = torch.empty(nb, dtype=torch.int64, device=dev)
    cuda = _is_gpu(bkey)
    load().ijoin_probe(cuda, _p(bkey), _p(bts), nb, _p(okey), _p(ots), no, int(rlo), int(rhi),
                       int(cutoff), _p(lb), _p(cnt), _stream(bkey) if cuda else 0)
    return lb, cnt


def ijoin_scan(cnt: torch.Tensor, lb: torch.Tensor):
    """Exclusive 64-bit saturating scan of the counts and the non-empty elements compacted:
    (plan, P, m, error word). One readback."""
    dev = cnt.device
    n = cnt.numel()
    _check(cnt, torch.int64, n, "cnt", dev)
    _check(lb, torch.int64, n, "lb", dev)
    m = load()
    plan = torch.empty(m.IJOIN_PLAN_COLS * (n + 1), dtype=torch.int64, device=dev)
    meta = torch.zeros(m.IJOIN_META, dtype=torch.int64, device=dev)
    scratch = torch.empty(max(16, m.ijoin_scan_scratch_bytes(n)), dtype=torch.uint8, device=dev)
    cuda = _is_gpu(cnt)
    m.ijoin_scan(cuda, _p(cnt), _p(lb), n, _p(scratch), _p(plan), _p(meta),
                 _stream(cnt) if cuda else 0)
    pairs, rows, err, _ = meta.tolist()
    return plan, pairs, rows, err


def ijoin_plan(side: int, batch, other, lo: int, hi: int, cutoff: int = I64_MIN) -> IJoinPlan:
    """Probe `other` (the other side's buffer) with the sorted `batch` of `side` under the
    bounds l.ts + lo <= r.ts <= l.ts + hi and scan the counts. 2**62 pairs or more raise
    OverflowError before anything is expanded."""
    if side not in (0, 1):
        raise ValueError("side must be 0 (left) or 1 (right)")
    dev = batch[0].device
    _ijoin_cols(batch, "batch", dev)
    _ijoin_cols(other, "other", dev)
    rlo, rhi = (lo, hi) if side == 0 else (sat_add_i64(0, -int(hi)), sat_add_i64(0, -int(lo)))
    lb, cnt = ijoin_probe(batch[0], batch[1], other[0], other[1], rlo, rhi, cutoff)
    plan, pairs, rows, err = ijoin_scan(cnt, lb)
    if err or pairs >= load().JOIN_MAX_PAIRS:
        raise OverflowError("interval join: a batch of 2**62 pairs or more")
    return IJoinPlan(side, tuple(batch), tuple(other), lb, cnt, plan, pairs, rows)


def ijoin_expand(jp: IJoinPlan, p0: int, p1: int):
    """Pairs [p0, p1) of the planned batch as four int64 columns of p1 - p0 rows: the key id, the
    left and the right value bits and max(l.ts, r.ts). Batch elements in order, each with its
    partners in the other buffer's order."""
    dev = jp.lb.device
    p0, p1 = int(p0), int(p1)
    _pair_range(p0, p1, jp.pairs)
    ok, ol, orr, ot = _pair_columns(4, p1 - p0, dev)
    if p0 == p1:
        return ok, ol, orr, ot
    bk, bt, bv = jp.batch
    _, ots, ov = jp.other
    m = load()
    if _is_gpu(jp.lb):
        m.gpu_ijoin_expand(_p(jp.plan), bk.numel(), jp.rows, jp.pairs, _p(bk), _p(bt), _p(bv),
                           _p(ots), _p(ov), ots.numel(), jp.side, p0, p1, _p(ok), _p(ol), _p(orr),
                           _p(ot), _stream(jp.lb))
    else:
        m.cpu_ijoin_expand(_p(jp.cnt), _p(jp.lb), _p(bk), _p(bt), _p(bv), bk.numel(), _p(ots),
                           _p(ov), ots.numel(), jp.side, p0, p1, _p(ok), _p(ol), _p(orr), _p(ot))
    return ok, ol, orr, ot


def _ijoin_out(out: torch.Tensor, rows: int, inputs, name: str) -> None:
    """`out` must be a contiguous int64 [3, >= rows] tensor that shares no storage with `inputs`."""
    if out.dtype != torch.int64 or out.dim() != 2 or out.shape[0] != 3 or out.shape[1] < rows \
            or not out.is_contiguous():
        raise ValueError(f"{name}: out must be a contiguous int64 [3, >= rows] tensor")
    for c in inputs:
        if c.numel() and c.untyped_storage().data_ptr() == out.untyped_storage().data_ptr():
            raise ValueError(f"{name}: out must not alias an input")


def ijoin_merge(old, batch, out: torch.Tensor) -> int:
    """Merge the sorted `batch` into the sorted buffer `old` (both (key, ts, val)) into the rows
    of `out` (int64 [3, cap]); on equal (key, ts) the old rows stay first. Returns the row count."""
    dev = out.device
    no = _ijoin_cols(old, "old", dev)
    nb = _ijoin_cols(batch, "batch", dev)
    _ijoin_out(out, no + nb, (*old, *batch), "ijoin_merge")
    cuda = _is_gpu(out)
    load().ijoin_merge(cuda, *(_p(c) for c in old), no, *(_p(c) for c in batch), nb,
                       _p(out[0]), _p(out[1]), _p(out[2]), _stream(out) if cuda else 0)
    return no + nb


def ijoin_purge(src, cutoff: int, out: torch.Tensor) -> int:
    """Order-preserving compaction of the rows of `src` (key, ts, val) with ts > cutoff into the
    rows of `out` (int64 [3, cap >= rows]). Returns the number of survivors (one readback)."""
    dev = out.device
    n = _ijoin_cols(src, "src", dev)
    _ijoin_out(out, n, src, "ijoin_purge")
    m = load()
    if not _is_gpu(out):
        return m.cpu_ijoin_purge(*(_p(c) for c in src), n, int(cutoff), _p(out[0]), _p(out[1]),
                                 _p(out[2]))
    if n == 0:
        return 0
    st = _stream(out)
    keep = torch.empty(n, dtype=torch.int64, device=dev)
    m.gpu_ijoin_keep(_p(src[1]), n, int(cutoff), _p(keep), st)
    plan, _, rows, _ = ijoin_scan(keep, keep)
    m.gpu_ijoin_gather(_p(plan), n, rows, *(_p(c) for c in src), _p(out[0]), _p(out[1]),
                       _p(out[2]), st)
    return rows


# ---- keyed latest-value lookup (csrc/mxs_lookup.h) ---------------------------------------------

LOOKUP_WHENS = {None: 0, ">": 1, ">=": 2, "<": 3, "<=": 4, "==": 5, "!=": 6}
LOOKUP_TILE = 4096


def lookup_when(when) -> int:
    """The comparison's code (csrc LookupWhen); anything but None and the six operators raises."""
    try:
        return LOOKUP_WHENS[when]
    except (KeyError, TypeError):
        raise ValueError(f"when must be one of '>', '>=', '<', '<=', '==', '!=' or None, "
                         f"got {when!r}") from None


def _lookup_table(table: torch.Tensor) -> int:
    if table.dtype != torch.int64 or table.dim() != 2 or table.shape[1] != 2 \
            or table.shape[0] < 1 or not table.is_contiguous() or table.data_ptr() % 16:
        raise ValueError("lookup: the table must be a contiguous, 16-byte aligned int64 [cap, 2] "
                         "tensor with cap >= 1")
    return table.shape[0]


def _lookup_cols(cols, names, dev) -> int:
    n = cols[0].numel()
    for c, nm in zip(cols, names):
        _check(c, torch.int64, n, nm, dev)
        if c.dim() != 1 or c.numel() != n:
            raise ValueError(f"{nm}: one word per row expected")
    return n


def _lookup_default(default_bits):
    if default_bits is None:
        return False, 0
    d = int(default_bits)
    if not I64_MIN <= d <= I64_MAX:
        raise ValueError("lookup: default_bits must be an int64 bit pattern")
    return True, d


def lookup_upsert(table: torch.Tensor, keys: torch.Tensor, vals: torch.Tensor,
                  max_key: int | None = None) -> None:
    """Store (vals[i], present) at table[keys[i]] for a batch of rules in arrival order; the last
    rule of a key wins. Every key must lie in [0, cap) (`max_key`: the batch's largest key when
    the caller knows it, else one readback of the extremes). GPU: stable radix sort by key, then
    the row that ends its key's run stores; a one-row batch skips the sort."""
    dev = table.device
    cap = _lookup_table(table)
    n = _lookup_cols((keys, vals), ("keys", "vals"), dev)
    if n == 0:
        return
    if max_key is None or not _is_gpu(table):
        lo, hi = torch.stack([keys.min(), keys.max()]).tolist()
    else:
        lo, hi = 0, int(max_key)
    if lo < 0 or hi >= cap:
        raise ValueError(f"lookup_upsert: keys must lie in [0, {cap})")
    m = load()
    if not _is_gpu(table):
        m.cpu_lookup_upsert(_p(keys), _p(vals), n, _p(table), cap)
        return
    if n == 1:
        skeys, perm = keys, torch.zeros(1, dtype=torch.int64, device=dev)
    else:
        idx = torch.arange(n, dtype=torch.int64, device=dev)
        skeys, perm = sort_pairs(keys, idx, bits=max(1, hi.bit_length()))
    m.gpu_lookup_upsert(_p(skeys), _p(perm), _p(vals), n, _p(table), cap, _stream(table))


@dataclass
class LookupMask:
    """A probed sample batch (``lookup_mask``): what ``lookup_emit`` needs to write the kept rows."""
    table: torch.Tensor
    keys: torch.Tensor
    vals: torch.Tensor
    has_default: bool
    default_bits: int
    words: torch.Tensor     # int64 [ntiles * 64]: one bit per row, 64 words per tile
    counts: torch.Tensor    # int32 [ntiles]: kept rows per tile
    offsets: torch.Tensor   # int64 [ntiles]: exclusive scan of counts
    kept: int


def lookup_mask(table: torch.Tensor, keys: torch.Tensor, vals: torch.Tensor, when,
                default_bits=None) -> LookupMask:
    """Probe the table with a batch of samples: row i is kept when key i has a value in force
    (its rule's, else the default) and ``vals[i] <when> value`` holds on the two doubles (`when`
    None: always). Mask words, tile counts, their exclusive scan and the total (one readback)."""
    dev = table.device
    cap = _lookup_table(table)
    n = _lookup_cols((keys, vals), ("keys", "vals"), dev)
    code = lookup_when(when)
    has_default, dbits = _lookup_default(default_bits)
    m = load()
    ntiles = (n + m.LOOKUP_TILE - 1) // m.LOOKUP_TILE
    words = torch.empty(max(1, ntiles * m.LOOKUP_WORDS), dtype=torch.int64, device=dev)
    counts = torch.empty(max(1, ntiles), dtype=torch.int32, device=dev)
    offsets = torch.empty(max(1, ntiles), dtype=torch.int64, device=dev)
    meta = torch.zeros(m.LOOKUP_META, dtype=torch.int64, device=dev)
    cuda = _is_gpu(table)
    st = _stream(table) if cuda else 0
    m.lookup_mask(cuda, _p(keys), _p(vals), n, _p(table), cap, code, has_default, dbits,
                  _p(words), _p(counts), st)
    m.lookup_scan(cuda, _p(counts), ntiles, _p(offsets), _p(meta), st)
    kept = int(meta[0].item())
    return LookupMask(table, keys, vals, has_default, dbits, words[:ntiles * m.LOOKUP_WORDS],
                      counts[:ntiles], offsets[:ntiles], kept)


def lookup_emit(lm: LookupMask, ts: torch.Tensor):
    """The kept rows of a probed batch, in input order, as four int64 columns: key id, value
    bits, looked-up bits and timestamp."""
    dev = lm.table.device
    n = _lookup_cols((lm.keys, lm.vals, ts), ("keys", "vals", "ts"), dev)
    out = torch.empty((4, lm.kept), dtype=torch.int64, device=dev)
    if lm.kept == 0:
        return out[0], out[1], out[2], out[3]
    if not 0 <= lm.kept <= n:
        raise ValueError("lookup_emit: kept rows outside [0, n]")
    cuda = _is_gpu(lm.table)
    load().lookup_emit(cuda, _p(lm.keys), _p(lm.vals), _p(ts), n, _p(lm.table), lm.table.shape[0],
                       lm.has_default, lm.default_bits, _p(lm.words), _p(lm.counts),
                       _p(lm.offsets), lm.kept, _p(out[0]), _p(out[1]), _p(out[2]), _p(out[3]),
                       _stream(lm.table) if cuda else 0)
    return out[0], out[1], out[2], out[3]


def lookup_gather(table: torch.Tensor, keys: torch.Tensor, vals: torch.Tensor, ts: torch.Tensor,
                  default_bits: int):
    """Every row kept (no comparison, a default): the four columns of ``lookup_emit`` without
    mask and scan."""
    dev = table.device
    cap = _lookup_table(table)
    n = _lookup_cols((keys, vals, ts), ("keys", "vals", "ts"), dev)
    _, dbits = _lookup_default(default_bits)
    out = torch.empty((4, n), dtype=torch.int64, device=dev)
    cuda = _is_gpu(table)
    load().lookup_gather(cuda, _p(keys), _p(vals), _p(ts), n, _p(table), cap, dbits, _p(out[0]),
                         _p(out[1]), _p(out[2]), _p(out[3]), _stream(table) if cuda else 0)
    return out[0], out[1], out[2], out[3]


# ---- broadcast rule set (csrc/mxs_ruleset.h) ---------------------------------------------------

RULESET_MAX = 64  # rule ids [0, 64): one mask bit each


def _ruleset_table(rules: torch.Tensor) -> None:
    if rules.dtype != torch.int64:
        raise TypeError(f"ruleset: the rule table is int64, got {rules.dtype}")
    if tuple(rules.shape) != (RULESET_MAX, 2) or not rules.is_contiguous() \
            or rules.data_ptr() % 16:
        raise ValueError("ruleset: the rule table must be a contiguous, 16-byte aligned int64 "
                         f"[{RULESET_MAX}, 2] tensor")


@dataclass
class RuleSetCount:
    """A counted sample batch (``ruleset_count``): what ``ruleset_emit`` needs to write the rows."""
    rules: torch.Tensor
    vals: torch.Tensor
    gsum: torch.Tensor      # int32 [ntiles * 64]: rows per group of 64 samples
    counts: torch.Tensor    # int32 [ntiles]: rows per tile
    offsets: torch.Tensor   # int64 [ntiles]: exclusive scan of counts
    total: int


def ruleset_count(rules: torch.Tensor, vals: torch.Tensor) -> RuleSetCount:
    """Test a batch of samples against the rule table (row r = threshold bits, comparison code
    1..6, 0: no rule r): the rows (sample, broken rule) per group of 64 samples and per tile, the
    tiles' exclusive scan and the total (one readback)."""
    dev = rules.device
    _ruleset_table(rules)
    n = _lookup_cols((vals,), ("vals",), dev)
    m = load()
    ntiles = (n + m.LOOKUP_TILE - 1) // m.LOOKUP_TILE
    gsum = torch.empty(max(1, ntiles * m.RULESET_GROUPS), dtype=torch.int32, device=dev)
    counts = torch.empty(max(1, ntiles), dtype=torch.int32, device=dev)
    offsets = torch.empty(max(1, ntiles), dtype=torch.int64, device=dev)
    meta = torch.zeros(m.LOOKUP_META, dtype=torch.int64, device=dev)
    cuda = _is_gpu(rules)
    st = _stream(rules) if cuda else 0
    m.ruleset_count(cuda, _p(vals), n, _p(rules), _p(gsum), _p(counts), st)
    m.lookup_scan(cuda, _p(counts), ntiles, _p(offsets), _p(meta), st)
    total = int(meta[0].item())
    return RuleSetCount(rules, vals, gsum[:ntiles * m.RULESET_GROUPS], counts[:ntiles],
                        offsets[:ntiles], total)


def ruleset_emit(rc: RuleSetCount, keys: torch.Tensor, ts: torch.Tensor):
    """The rows of a counted batch, in sample order, then ascending rule id, as five int64
    columns: key id, value bits, rule id, threshold bits and timestamp."""
    dev = rc.rules.device
    _ruleset_table(rc.rules)
    n = _lookup_cols((rc.vals, keys, ts), ("vals", "keys", "ts"), dev)
    if not 0 <= rc.total <= n * RULESET_MAX:
        raise ValueError("ruleset_emit: rows outside [0, 64 n]")
    ntiles = (n + LOOKUP_TILE - 1) // LOOKUP_TILE
    _check(rc.gsum, torch.int32, ntiles * (LOOKUP_TILE // 64), "gsum", dev)
    _check(rc.counts, torch.int32, ntiles, "counts", dev)
    _check(rc.offsets, torch.int64, ntiles, "offsets", dev)
    out = torch.empty((5, rc.total), dtype=torch.int64, device=dev)
    if rc.total:
        cuda = _is_gpu(rc.rules)
        load().ruleset_emit(cuda, _p(keys), _p(rc.vals), _p(ts), n, _p(rc.rules), _p(rc.gsum),
                            _p(rc.counts), _p(rc.offsets), rc.total, *(_p(out[c]) for c in range(5)),
                            _stream(rc.rules) if cuda else 0)
    return out[0], out[1], out[2], out[3], out[4]


# ---- keyed event-time timers (csrc/mxs_timeout.h) -----------------------------------------------

TIMEOUT_TILE = 4096
TIMEOUT_NONE = I64_MAX  # deadline of a key that is not armed


def timeout_tables(cap: int, device):
    """Fresh state for `cap` key ids: state int64[cap, 2] of zeros, deadline int64[cap] and
    tile_min int64[ceil(cap / TIMEOUT_TILE)] of TIMEOUT_NONE."""
    if cap < 1:
        raise ValueError("timeout: cap must be >= 1")
    state = torch.zeros((cap, 2), dtype=torch.int64, device=device)
    deadline = torch.full((cap,), TIMEOUT_NONE, dtype=torch.int64, device=device)
    tile_min = torch.full(((cap + TIMEOUT_TILE - 1) // TIMEOUT_TILE,), TIMEOUT_NONE,
                          dtype=torch.int64, device=device)
    return state, deadline, tile_min


def _timeout_tables(state, deadline, tile_min) -> int:
    cap = deadline.numel()
    dev = deadline.device
    if deadline.dtype != torch.int64 or deadline.dim() != 1 or cap < 1 \
            or not deadline.is_contiguous() or deadline.data_ptr() % 16:
        raise ValueError("timeout: deadline must be a contiguous, 16-byte aligned int64 [cap] "
                         "tensor with cap >= 1")
    if state is not None and (state.dtype != torch.int64 or state.dim() != 2
                              or tuple(state.shape) != (cap, 2) or not state.is_contiguous()
                              or state.data_ptr() % 16 or state.device != dev):
        raise ValueError("timeout: state must be a contiguous, 16-byte aligned int64 [cap, 2] "
                         "tensor on the deadlines' device")
    if tile_min is not None and (tile_min.dtype != torch.int64 or tile_min.dim() != 1
                                 or tile_min.numel() != (cap + TIMEOUT_TILE - 1) // TIMEOUT_TILE
                                 or not tile_min.is_contiguous() or tile_min.device != dev):
        raise ValueError("timeout: tile_min must be a contiguous int64 [ceil(cap / 4096)] tensor "
                         "on the deadlines' device")
    return cap


def timeout_update(state: torch.Tensor, deadline: torch.Tensor, tile_min: torch.Tensor,
                   keys: torch.Tensor, ts: torch.Tensor, timeout: int,
                   bounds: tuple | None = None) -> None:
    """A batch of elements in arrival order: per key, count += its rows, last = the timestamp of
    its last row, deadline = last + timeout (armed), tile_min lowered. Every key must lie in
    [0, cap) and max(ts) + timeout below INT64_MAX (`bounds` = (largest key, largest timestamp)
    when the caller has read them, else one readback). GPU: stable radix sort by key, then the
    row that ends its key's run writes; a one-row batch skips the sort."""
    dev = deadline.device
    cap = _timeout_tables(state, deadline, tile_min)
    n = _lookup_cols((keys, ts), ("keys", "ts"), dev)
    timeout = int(timeout)
    if not 0 < timeout < I64_MAX:
        raise ValueError("timeout_update: timeout must be a positive int64")
    if n == 0:
        return
    if bounds is None or not _is_gpu(deadline):
        lo, hi, tmax = torch.stack([keys.min(), keys.max(), ts.max()]).tolist()
    else:
        lo, (hi, tmax) = 0, (int(b) for b in bounds)
    if lo < 0 or hi >= cap:
        raise ValueError(f"timeout_update: keys must lie in [0, {cap})")
    if tmax >= I64_MAX - timeout:
        raise TypeError("timeout_update: timestamp + timeout reaches INT64_MAX")
    m = load()
    if not _is_gpu(deadline):
        m.cpu_timeout_update(_p(keys), _p(ts), n, timeout, _p(state), _p(deadline), _p(tile_min),
                             cap)
        return
    if n == 1:
        skeys, perm = keys, torch.zeros(1, dtype=torch.int64, device=dev)
    else:
        idx = torch.arange(n, dtype=torch.int64, device=dev)
        skeys, perm = sort_pairs(keys, idx, bits=max(1, hi.bit_length()))
    m.gpu_timeout_update(_p(skeys), _p(perm), _p(ts), n, timeout, _p(state), _p(deadline),
                         _p(tile_min), cap, _stream(deadline))


@dataclass
class TimeoutMask:
    """A scanned firing (``timeout_mask``): what ``timeout_emit`` needs to write the due keys."""
    words: torch.Tensor     # int64 [ntiles * 64]: one bit per key id (a skipped tile's: unwritten)
    counts: torch.Tensor    # int32 [ntiles]: due keys per tile
    offsets: torch.Tensor   # int64 [ntiles]: exclusive scan of counts
    total: int


def timeout_mask(deadline: torch.Tensor, tile_min: torch.Tensor, w: int) -> TimeoutMask:
    """The keys due at watermark `w` (armed and deadline <= w): mask words and counts per tile of
    4096 key ids, their exclusive scan and the total (one readback). A tile whose tile_min lies
    above `w` is not read (MXS_TIMEOUT_TILESKIP=0: every tile is); a scanned tile's tile_min
    becomes the exact minimum of the deadlines that stay armed."""
    dev = deadline.device
    cap = _timeout_tables(None, deadline, tile_min)
    w = int(w)
    if not I64_MIN <= w <= I64_MAX:
        raise ValueError("timeout_mask: the watermark must be an int64")
    m = load()
    ntiles = tile_min.numel()
    words = torch.empty(ntiles * m.TIMEOUT_WORDS, dtype=torch.int64, device=dev)
    counts = torch.empty(ntiles, dtype=torch.int32, device=dev)
    offsets = torch.empty(ntiles, dtype=torch.int64, device=dev)
    meta = torch.zeros(m.LOOKUP_META, dtype=torch.int64, device=dev)
    cuda = _is_gpu(deadline)
    st = _stream(deadline) if cuda else 0
    m.timeout_mask(cuda, _p(deadline), cap, w, _p(tile_min), _p(words), _p(counts), st)
    m.lookup_scan(cuda, _p(counts), ntiles, _p(offsets), _p(meta), st)
    return TimeoutMask(words, counts, offsets, int(meta[0].item()))


def timeout_emit(state: torch.Tensor, deadline: torch.Tensor, tm: TimeoutMask):
    """The due keys of a scanned firing in key order as four int64 columns (key id, count, last,
    deadline); every emitted key is disarmed."""
    dev = deadline.device
    cap = _timeout_tables(state, deadline, None)
    ntiles = (cap + TIMEOUT_TILE - 1) // TIMEOUT_TILE
    out = torch.empty((4, tm.total), dtype=torch.int64, device=dev)
    if tm.total == 0:
        return out[0], out[1], out[2], out[3]
    if not 0 <= tm.total <= cap or tm.counts.numel() != ntiles or tm.offsets.numel() != ntiles \
            or tm.words.numel() != ntiles * 64:
        raise ValueError("timeout_emit: the mask is not of these tables")
    for t, dt, nm in ((tm.words, torch.int64, "words"), (tm.counts, torch.int32, "counts"),
                      (tm.offsets, torch.int64, "offsets")):
        _check(t, dt, t.numel(), nm, dev)
    cuda = _is_gpu(deadline)
    load().timeout_emit(cuda, _p(state), _p(deadline), cap, _p(tm.words), _p(tm.counts),
                        _p(tm.offsets), tm.total, _p(out[0]), _p(out[1]), _p(out[2]), _p(out[3]),
                        _stream(deadline) if cuda else 0)
    return out[0], out[1], out[2], out[3]


# ---- sustained-condition alerts (csrc/mxs_sustain.h) --------------------------------------------

SUSTAIN_NONE = I64_MIN        # `since` of a key without an open run
SUSTAIN_TS_LIMIT = 1 << 62    # |ts| must stay below it: ts - since cannot overflow
SUSTAIN_LONG, SUSTAIN_DOUBLE = 0, 1


def sustain_table(cap: int, device) -> torch.Tensor:
    """Fresh state for `cap` key ids: int64[cap, 2], every row (SUSTAIN_NONE, 0)."""
    if cap < 1:
        raise ValueError("sustain: cap must be >= 1")
    state = torch.zeros((cap, 2), dtype=torch.int64, device=device)
    state[:, 0] = SUSTAIN_NONE
    return state


def _rule_update(row: torch.Tensor, keys, vals, ts, bounds, name: str, twin, scan,
                 code_bits: int = 1, gather: str = "gpu_sustain_gather"):
    """What the rules over a batch sorted by key share once their parameters are checked (`row`
    is the rule's [cap, 2] table, `name` the caller's for messages): the bounds, then on the CPU
    ``twin(*five output pointers)`` -> rows, else the sort by key, ``scan(skeys, perm, tags,
    since, count, stream)`` (pointers), the count's readback, the sort by arrival index and the
    gather. Five columns in arrival order. A row's tag is ``arrival << code_bits | code``;
    `gather` names the native function that takes such tags apart (the family's, for one bit)."""
    dev = row.device
    cap, n = row.shape[0], keys.numel()
    out = torch.empty((5, n), dtype=torch.int64, device=dev)
    if n == 0:
        return tuple(out[c] for c in range(5))
    if bounds is None or not _is_gpu(row):
        lo, hi, tmin, tmax = torch.stack([keys.min(), keys.max(), ts.min(), ts.max()]).tolist()
    else:
        lo, (hi, tmin, tmax) = 0, (int(b) for b in bounds)
    if lo < 0 or hi >= cap:
        raise ValueError(f"{name}: keys must lie in [0, {cap})")
    if tmin <= -SUSTAIN_TS_LIMIT or tmax >= SUSTAIN_TS_LIMIT:
        raise TypeError(f"{name}: a timestamp at or beyond 2**62")
    if not _is_gpu(row):
        rows = twin(*(_p(out[c]) for c in range(5)))
        return tuple(out[c, :rows] for c in range(5))
    st = _stream(row)
    if n == 1:
        skeys, perm = keys, torch.zeros(1, dtype=torch.int64, device=dev)
    else:
        idx = torch.arange(n, dtype=torch.int64, device=dev)
        skeys, perm = sort_pairs(keys, idx, bits=max(1, hi.bit_length()))
    scratch = torch.empty((2, n), dtype=torch.int64, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    scan(_p(skeys), _p(perm), _p(scratch[0]), _p(scratch[1]), _p(count), st)
    rows = int(count.item())  # the only readback
    if not 0 <= rows <= n:
        raise RuntimeError(f"{name}: more transitions than rows")
    if rows == 0:
        return tuple(out[c, :0] for c in range(5))
    # Arrival order: the tags are ``arrival << code_bits | code``, one per element at most.
    tags, since = scratch[0, :rows], scratch[1, :rows]
    if rows > 1:
        tags, since = sort_pairs(tags, since, bits=(n - 1).bit_length() + code_bits)
    getattr(load(), gather)(_p(tags), _p(since), rows, _p(keys), _p(vals), _p(ts), n,
                            *(_p(out[c]) for c in range(5)), st)
    return tuple(out[c, :rows] for c in range(5))


def sustain_update(state: torch.Tensor, keys: torch.Tensor, vals: torch.Tensor, ts: torch.Tensor,
                   *, kind: int, when, threshold_bits: int, for_ms: int,
                   bounds: tuple | None = None):
    """A batch of elements in arrival order (key ids, value bits of `kind`, timestamps) against
    the rule ``value <when> threshold`` held for `for_ms`: the table is updated and the batch's
    transitions come back in arrival order as five int64 columns (key id, code 1 = fired /
    0 = resolved, since, value bits, ts). Every key must lie in [0, cap) and every timestamp
    strictly inside (-2**62, 2**62) (`bounds` = (largest key, smallest and largest timestamp)
    when the caller has read them, else one readback). GPU: stable radix sort by key, one
    segmented wave scan, the rows' count read back, a radix sort of the rows by arrival index; a
    one-row batch skips the first sort."""
    dev = state.device
    cap = _lookup_table(state)
    n = _lookup_cols((keys, vals, ts), ("keys", "vals", "ts"), dev)
    code = lookup_when(when)
    if code == 0:
        raise ValueError("sustain_update: a comparison is required")
    if kind not in (SUSTAIN_LONG, SUSTAIN_DOUBLE):
        raise ValueError("sustain_update: kind must be SUSTAIN_LONG or SUSTAIN_DOUBLE")
    for_ms, tbits = int(for_ms), int(threshold_bits)
    if not 0 <= for_ms <= I64_MAX:
        raise ValueError("sustain_update: for_ms must be a non-negative int64")
    if not I64_MIN <= tbits <= I64_MAX:
        raise ValueError("sustain_update: threshold_bits must be an int64 bit pattern")
    if n >= 1 << 31:
        raise ValueError("sustain_update: at most 2**31 - 1 rows per batch")
    rule = (n, kind, code, tbits, for_ms, _p(state), cap)
    return _rule_update(
        state, keys, vals, ts, bounds, "sustain_update",
        lambda *outs: load().cpu_sustain_update(_p(keys), _p(vals), _p(ts), *rule, *outs),
        lambda skeys, perm, *outs: load().gpu_sustain_scan(skeys, perm, _p(vals), _p(ts), *rule,
                                                           *outs))


# ---- burst alerts (csrc/mxs_burst.h) ------------------------------------------------------------

BURST_MAX_TIMES = 16          # the engine's largest `times`
BURST_HELD_SHIFT, BURST_POS_SHIFT = 1, 8   # meta = firing | held << 1 | pos << 8


def burst_table(cap: int, times: int, device):
    """Fresh state for `cap` key ids: (ring int64[cap, times], row int64[cap, 2]), all zero: no
    breach held, not firing."""
    if cap < 1:
        raise ValueError("burst: cap must be >= 1")
    if isinstance(times, bool) or not isinstance(times, int) or not 2 <= times <= BURST_MAX_TIMES:
        raise ValueError(f"burst: times must be an int in [2, {BURST_MAX_TIMES}]")
    return (torch.zeros((cap, times), dtype=torch.int64, device=device),
            torch.zeros((cap, 2), dtype=torch.int64, device=device))


def burst_update(ring: torch.Tensor, row: torch.Tensor, keys: torch.Tensor, vals: torch.Tensor,
                 ts: torch.Tensor, *, kind: int, when, threshold_bits: int, within: int,
                 bounds: tuple | None = None):
    """A batch of elements in arrival order (key ids, value bits of `kind`, timestamps) against
    the rule "`times` breaches of ``value <when> threshold`` within `within` ms" (`times` is the
    ring's width): ring and row are updated and the batch's transitions come back in arrival
    order as five int64 columns (key id, code 1 = fired / 0 = resolved, since, value bits, ts).
    Every key must lie in [0, cap) and every timestamp strictly inside (-2**62, 2**62) (`bounds`
    = (largest key, smallest and largest timestamp) when the caller has read them, else one
    readback). GPU: stable radix sort by key, the look-back and one segmented wave scan, the
    rows' count read back, a radix sort of the rows by arrival index and sustain's gather; a
    one-row batch skips the first sort."""
    dev = row.device
    cap = _lookup_table(row)
    if ring.dtype != torch.int64 or ring.dim() != 2 or ring.shape[0] != cap \
            or not 2 <= ring.shape[1] <= BURST_MAX_TIMES or not ring.is_contiguous() \
            or ring.device != dev or ring.data_ptr() % 8:
        raise ValueError("burst_update: the ring must be a contiguous int64 [cap, times] tensor "
                         f"beside the rows, times in [2, {BURST_MAX_TIMES}]")
    times = ring.shape[1]
    n = _lookup_cols((keys, vals, ts), ("keys", "vals", "ts"), dev)
    code = lookup_when(when)
    if code == 0:
        raise ValueError("burst_update: a comparison is required")
    if kind not in (SUSTAIN_LONG, SUSTAIN_DOUBLE):
        raise ValueError("burst_update: kind must be SUSTAIN_LONG or SUSTAIN_DOUBLE")
    within, tbits = int(within), int(threshold_bits)
    if not 0 <= within < SUSTAIN_TS_LIMIT:
        raise ValueError("burst_update: within must lie in [0, 2**62)")
    if not I64_MIN <= tbits <= I64_MAX:
        raise ValueError("burst_update: threshold_bits must be an int64 bit pattern")
    if n >= 1 << 31:
        raise ValueError("burst_update: at most 2**31 - 1 rows per batch")
    rule = (n, kind, code, tbits, times, within, _p(ring), _p(row), cap)
    return _rule_update(
        row, keys, vals, ts, bounds, "burst_update",
        lambda *outs: load().cpu_burst_update(_p(keys), _p(vals), _p(ts), *rule, *outs),
        lambda skeys, perm, *outs: load().gpu_burst_scan(skeys, perm, _p(vals), _p(ts), *rule,
                                                         *outs))


# ---- keyed state machines (csrc/mxs_fsm.h) ------------------------------------------------------

FSM_NONE = I64_MIN            # `since` of a key that was never seen
FSM_MAX_STATES = FSM_MAX_CLASSES = 16   # a function S -> S packs into one 64-bit word
FSM_TAG_BITS = 8              # a row's tag = arrival << 8 | from << 4 | to


def fsm_table(cap: int, device) -> torch.Tensor:
    """Fresh state for `cap` key ids: int64[cap, 2], every row (FSM_NONE, 0)."""
    if cap < 1:
        raise ValueError("fsm: cap must be >= 1")
    state = torch.zeros((cap, 2), dtype=torch.int64, device=device)
    state[:, 0] = FSM_NONE
    return state


def _is_int(x) -> bool:
    return isinstance(x, int) and not isinstance(x, bool)


def fsm_pack(bounds, table, report):
    """A state machine's parameters as the engine takes them: (cuts, cols, masks). `bounds`:
    classes - 1 finite numbers, strictly ascending as doubles; `table`: states rows of classes
    ints in [0, states); `report`: (from, to) pairs. cuts: the bounds as floats; cols[c]: the
    table's column c as a function, nibble s = table[s][c]; masks[from]: bit `to` set for a
    reported pair. At most 16 states and 16 classes."""
    table = [list(r) for r in table]
    states = len(table)
    if not 1 <= states <= FSM_MAX_STATES:
        raise ValueError(f"fsm: 1 to {FSM_MAX_STATES} states, got {states}")
    classes = len(table[0])
    if not 1 <= classes <= FSM_MAX_CLASSES:
        raise ValueError(f"fsm: 1 to {FSM_MAX_CLASSES} classes, got {classes}")
    bounds = list(bounds)
    if len(bounds) != classes - 1:
        raise ValueError("fsm: the table has one more column than there are bounds")
    if any(isinstance(b, bool) or not isinstance(b, (int, float)) for b in bounds):
        raise TypeError("fsm: a bound must be an int or a float")
    cuts = tuple(float(b) for b in bounds)
    if any(c != c or c in (float("inf"), float("-inf")) for c in cuts) \
            or any(a >= b for a, b in zip(cuts, cuts[1:])):
        raise ValueError("fsm: the bounds must be finite and strictly ascending")
    cols = [0] * classes
    for s, row in enumerate(table):
        if len(row) != classes:
            raise ValueError("fsm: every table row has one entry per class")
        for c, to in enumerate(row):
            if not _is_int(to) or not 0 <= to < states:
                raise ValueError(f"fsm: table[{s}][{c}] = {to!r} is no state in [0, {states})")
            cols[c] |= to << (4 * s)
    masks = [0] * states
    for pair in report:
        a, b = pair
        if not _is_int(a) or not _is_int(b) or not (0 <= a < states and 0 <= b < states):
            raise ValueError(f"fsm: the reported pair {pair!r} is no pair of states")
        masks[a] |= 1 << b
    return cuts, tuple(cols), tuple(masks)


def fsm_update(state: torch.Tensor, keys: torch.Tensor, vals: torch.Tensor, ts: torch.Tensor,
               *, kind: int, cuts, cols, report, states: int, classes: int, initial: int,
               bounds: tuple | None = None):
    """A batch of elements in arrival order (key ids, value bits of `kind`, timestamps) against
    a state machine per key (`cuts`, `cols`, `report` as fsm_pack gives them, `report` being its
    masks; `states` and `classes` their lengths): an element's class is the number of cuts its
    value reaches, ``to = table[from][class]``, and a reported (from, to) is a row. The table is
    updated and the rows come back in arrival order as five int64 columns (key id,
    from << 4 | to, since, value bits, ts), `since` being the timestamp at which the key entered
    `from`. Every key must lie in [0, cap) and every timestamp strictly inside (-2**62, 2**62)
    (`bounds` = (largest key, smallest and largest timestamp) when the caller has read them,
    else one readback). GPU: stable radix sort by key, one segmented wave scan of the packed
    functions, the rows' count read back, a radix sort of the rows by arrival index; a one-row
    batch skips the first sort."""
    dev = state.device
    try:
        cap = _lookup_table(state)
    except ValueError:
        raise ValueError("fsm_update: the table must be a contiguous, 16-byte aligned int64 "
                         "[cap, 2] tensor with cap >= 1") from None
    n = _lookup_cols((keys, vals, ts), ("keys", "vals", "ts"), dev)
    if kind not in (SUSTAIN_LONG, SUSTAIN_DOUBLE):
        raise ValueError("fsm_update: kind must be SUSTAIN_LONG or SUSTAIN_DOUBLE")
    if not _is_int(states) or not 1 <= states <= FSM_MAX_STATES:
        raise ValueError(f"fsm_update: states must be an int in [1, {FSM_MAX_STATES}]")
    if not _is_int(classes) or not 1 <= classes <= FSM_MAX_CLASSES:
        raise ValueError(f"fsm_update: classes must be an int in [1, {FSM_MAX_CLASSES}]")
    cuts, cols, report = tuple(cuts), tuple(cols), tuple(report)
    if len(cuts) != classes - 1 or len(cols) != classes or len(report) != states:
        raise ValueError("fsm_update: classes - 1 cuts, classes columns and states masks expected")
    if not _is_int(initial) or not 0 <= initial < states:
        raise ValueError(f"fsm_update: initial must be a state in [0, {states})")
    if any(not isinstance(c, float) or c != c or abs(c) == float("inf") for c in cuts) \
            or any(a >= b for a, b in zip(cuts, cuts[1:])):
        raise ValueError("fsm_update: the cuts must be finite floats, strictly ascending")
    for c in cols:
        if not _is_int(c) or not 0 <= c < 1 << 64 or c >> (4 * states) \
                or any((c >> (4 * s)) & 15 >= states for s in range(states)):
            raise ValueError(f"fsm_update: a table entry is no state in [0, {states})")
    if any(not _is_int(m) or not 0 <= m < 1 << states for m in report):
        raise ValueError("fsm_update: a reported pair is no pair of states")
    if n >= 1 << 31:
        raise ValueError("fsm_update: at most 2**31 - 1 rows per batch")
    rule = (n, cuts, cols, report, initial, kind, _p(state), cap)
    return _rule_update(
        state, keys, vals, ts, bounds, "fsm_update",
        lambda *outs: load().cpu_fsm_update(_p(keys), _p(vals), _p(ts), *rule, *outs),
        lambda skeys, perm, *outs: load().gpu_fsm_scan(skeys, perm, _p(vals), _p(ts), *rule,
                                                       *outs),
        code_bits=FSM_TAG_BITS, gather="gpu_fsm_gather")


# ---- counter rates (csrc/mxs_rate.h) ------------------------------------------------------------

RATE_NONE = I64_MIN           # last_ts of a key that was never seen


def rate_table(cap: int, device) -> torch.Tensor:
    """Fresh state for `cap` key ids: int64[cap, 2], every row (RATE_NONE, 0)."""
    if cap < 1:
        raise ValueError("rate: cap must be >= 1")
    state = torch.zeros((cap, 2), dtype=torch.int64, device=device)
    state[:, 0] = RATE_NONE
    return state


def rate_update(state: torch.Tensor, keys: torch.Tensor, vals: torch.Tensor, ts: torch.Tensor,
                *, kind: int, per_ms: int, when, threshold_bits: int, max_gap,
                bounds: tuple | None = None):
    """A batch of counter readings in arrival order (key ids, value bits of `kind`, timestamps):
    an element whose timestamp is above its key's last accepted one is accepted, becomes the
    key's row, and, when the key had a row, gives ``dt``, ``inc`` (``v - last``, or ``v`` after
    a restart) and ``rate = float(inc) * per_ms / dt``; the row leaves when ``dt <= max_gap``
    (`max_gap` None: always) and ``rate <when> threshold`` holds (`when` None: always). Every
    other element of a key that has a row is ignored and counted. Returns ``(five int64 columns
    in arrival order (key id, rate bits, inc bits, dt, ts), ignored elements)``. Every key must
    lie in [0, cap) and every timestamp strictly inside (-2**62, 2**62) (`bounds` = (largest
    key, smallest and largest timestamp) when the caller has read them, else one readback). GPU:
    stable radix sort by key, one segmented wave scan that places (inc, dt) by arrival index, a
    mask over tiles, their scan, the counts' readback (the only one) and the emit in arrival
    order: no second sort. A one-row batch skips the sort."""
    dev = state.device
    try:
        cap = _lookup_table(state)
    except ValueError:
        raise ValueError("rate_update: the table must be a contiguous, 16-byte aligned int64 "
                         "[cap, 2] tensor with cap >= 1") from None
    n = _lookup_cols((keys, vals, ts), ("keys", "vals", "ts"), dev)
    code = lookup_when(when)
    if kind not in (SUSTAIN_LONG, SUSTAIN_DOUBLE):
        raise ValueError("rate_update: kind must be SUSTAIN_LONG or SUSTAIN_DOUBLE")
    if not _is_int(per_ms) or not 1 <= per_ms <= I64_MAX:
        raise ValueError("rate_update: per_ms must be a positive int64")
    if max_gap is not None and (not _is_int(max_gap) or not 1 <= max_gap < SUSTAIN_TS_LIMIT):
        raise ValueError("rate_update: max_gap must be None or an int in [1, 2**62)")
    tbits = int(threshold_bits)
    if not I64_MIN <= tbits <= I64_MAX:
        raise ValueError("rate_update: threshold_bits must be an int64 bit pattern")
    if n >= 1 << 31:
        raise ValueError("rate_update: at most 2**31 - 1 rows per batch")
    out = torch.empty((5, n), dtype=torch.int64, device=dev)
    if n == 0:
        return tuple(out[c] for c in range(5)), 0
    cuda = _is_gpu(state)
    if bounds is None or not cuda:
        lo, hi, tmin, tmax = torch.stack([keys.min(), keys.max(), ts.min(), ts.max()]).tolist()
    else:
        lo, (hi, tmin, tmax) = 0, (int(b) for b in bounds)
    if lo < 0 or hi >= cap:
        raise ValueError(f"rate_update: keys must lie in [0, {cap})")
    if tmin <= -SUSTAIN_TS_LIMIT or tmax >= SUSTAIN_TS_LIMIT:
        raise TypeError("rate_update: a timestamp at or beyond 2**62")
    m = load()
    rule = (kind, code, tbits, per_ms, max_gap or 0)
    if not cuda:
        rows, ignored = m.cpu_rate_update(_p(keys), _p(vals), _p(ts), n, *rule, _p(state), cap,
                                          *(_p(out[c]) for c in range(5)))
        return tuple(out[c, :rows] for c in range(5)), ignored
    st = _stream(state)
    if n == 1:
        skeys, perm = keys, torch.zeros(1, dtype=torch.int64, device=dev)
    else:
        idx = torch.arange(n, dtype=torch.int64, device=dev)
        skeys, perm = sort_pairs(keys, idx, bits=max(1, hi.bit_length()))
    ntiles = (n + m.LOOKUP_TILE - 1) // m.LOOKUP_TILE
    scratch = torch.empty((n, 2), dtype=torch.int64, device=dev)   # (inc bits, dt) by arrival
    words = torch.empty(ntiles * m.LOOKUP_WORDS, dtype=torch.int64, device=dev)
    counts = torch.empty(ntiles, dtype=torch.int32, device=dev)
    offsets = torch.empty(ntiles, dtype=torch.int64, device=dev)
    # [rows, unused (lookup_scan's), ignored elements (a uint32 in the low half)]
    meta = torch.zeros(m.LOOKUP_META + 1, dtype=torch.int64, device=dev)
    m.gpu_rate_scan(_p(skeys), _p(perm), _p(vals), _p(ts), n, kind, _p(state), cap, _p(scratch),
                    _p(meta) + 8 * m.LOOKUP_META, st)
    m.gpu_rate_mask(_p(scratch), n, *rule, _p(words), _p(counts), st)
    m.lookup_scan(True, _p(counts), ntiles, _p(offsets), _p(meta), st)
    got = meta.tolist()  # the only readback
    rows, ignored = got[0], got[m.LOOKUP_META]
    if not 0 <= rows <= n or not 0 <= ignored <= n:
        raise RuntimeError("rate_update: more rows than elements")
    if rows:
        m.gpu_rate_emit(_p(scratch), _p(keys), _p(ts), n, *rule, _p(words), _p(counts),
                        _p(offsets), rows, *(_p(out[c]) for c in range(5)), st)
    return tuple(out[c, :rows] for c in range(5)), ignored


# ---- event-time reorder buffer (csrc/mxs_reorder.h) ---------------------------------------------

REORDER_TILE = 4096           # output positions a workgroup of the collect owns
REORDER_MAX_CHUNKS = 1024     # chunks one cut / collect takes


def _reorder_ts(ts: torch.Tensor, n_arena: int) -> None:
    _check(ts, torch.int64, n_arena, "ts", ts.device)
    if ts.dim() != 1 or n_arena < 0:
        raise ValueError("reorder: ts must be one int64 column holding the arena's rows")


def _reorder_flag(err: torch.Tensor, dev) -> None:
    _check(err, torch.int64, 1, "err", dev)


def reorder_cut(ts: torch.Tensor, n_arena: int, begins, ends, w: int, cut: torch.Tensor) -> None:
    """Per chunk c, ``cut[c]`` = the first position of the ascending ``ts[begins[c], ends[c])``
    whose timestamp exceeds `w` (ends[c] when none does). `begins` / `ends` are host lists with
    0 <= begin <= end <= n_arena; `cut` is an int64 device column of at least as many words,
    written in place (no readback here)."""
    dev = ts.device
    _reorder_ts(ts, n_arena)
    k = len(begins)
    if len(ends) != k or not 1 <= k <= REORDER_MAX_CHUNKS:
        raise ValueError(f"reorder_cut: 1 to {REORDER_MAX_CHUNKS} chunks, one end per begin")
    if any(not 0 <= b <= e <= n_arena for b, e in zip(begins, ends)):
        raise ValueError("reorder_cut: a chunk outside the arena")
    if not I64_MIN <= w <= I64_MAX:
        raise ValueError("reorder_cut: the watermark must be an int64")
    _check(cut, torch.int64, k, "cut", dev)
    tab = torch.tensor([list(begins), list(ends)], dtype=torch.int64).to(dev)
    m = load()
    if _is_gpu(ts):
        m.gpu_reorder_cut(_p(ts), n_arena, _p(tab[0]), _p(tab[1]), k, w, _p(cut), _stream(ts))
    else:
        m.cpu_reorder_cut(_p(ts), n_arena, _p(tab[0]), _p(tab[1]), k, w, _p(cut))


def reorder_collect(ts: torch.Tensor, n_arena: int, begins, counts, lo: int, err: torch.Tensor):
    """The rows ``[begins[c], begins[c] + counts[c])`` of every chunk, in chunk order, as two
    int64 columns (``ts - lo``, arena index): the pairs a stable sort by the first puts in
    (ts, arrival) order. `err`: one int64 device word the kernels set on a guarded index."""
    dev = ts.device
    _reorder_ts(ts, n_arena)
    _reorder_flag(err, dev)
    k = len(begins)
    if len(counts) != k or not 1 <= k <= REORDER_MAX_CHUNKS:
        raise ValueError(f"reorder_collect: 1 to {REORDER_MAX_CHUNKS} chunks, one count per begin")
    if any(b < 0 or c < 0 or b + c > n_arena for b, c in zip(begins, counts)):
        raise ValueError("reorder_collect: a chunk outside the arena")
    dest = [0]
    for c in counts:
        dest.append(dest[-1] + c)
    total = dest[-1]
    if total >= 1 << 31:
        raise ValueError("reorder_collect: at most 2**31 - 1 rows")
    out = torch.empty((2, total), dtype=torch.int64, device=dev)
    if total == 0:
        return out[0], out[1]
    tab = torch.tensor([list(begins) + [0], dest], dtype=torch.int64).to(dev)
    m = load()
    if _is_gpu(ts):
        m.gpu_reorder_collect(_p(ts), n_arena, _p(tab[0]), _p(tab[1]), k, total, lo, _p(out[0]),
                              _p(out[1]), _p(err), _stream(ts))
    else:
        m.cpu_reorder_collect(_p(ts), n_arena, _p(tab[0]), _p(tab[1]), k, total, lo, _p(out[0]),
                              _p(out[1]))
    return out[0], out[1]


def reorder_gather(perm: torch.Tensor, src, n_src: int, dst, err: torch.Tensor) -> None:
    """``dst[c][i] = src[c][perm[i]]`` for the three columns (key id, ts, value bits). `src`
    columns hold at least `n_src` words, `dst` columns exactly ``perm.numel()``; every index must
    lie in [0, n_src) (an index outside writes nothing and sets `err` on the device, raises on the
    CPU)."""
    dev = perm.device
    n = _lookup_cols((perm,), ("perm",), dev)
    _reorder_flag(err, dev)
    if len(src) != 3 or len(dst) != 3 or n_src < 0:
        raise ValueError("reorder_gather: three source and three destination columns")
    for c in src:
        _check(c, torch.int64, n_src, "src", dev)
    _lookup_cols(tuple(dst) + (perm,), ("dst", "dst", "dst", "perm"), dev)
    if n == 0:
        return
    m = load()
    if _is_gpu(perm):
        m.gpu_reorder_gather(_p(perm), n, *(_p(c) for c in src), n_src, *(_p(c) for c in dst),
                             _p(err), _stream(perm))
    else:
        m.cpu_reorder_gather(_p(perm), n, *(_p(c) for c in src), n_src, *(_p(c) for c in dst))
