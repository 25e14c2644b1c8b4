"""Runners and comparisons shared by tests/test_text_model.py (C++ twins, `cuda=False`) and
tests/test_text_kernels.py (gfx950 kernels): the ingest, dictionary and row-format bindings are
called directly on buffers pre-filled with sentinels, and every output word is compared with
tests/text_model.py. Every comparison is exact.
"""
from __future__ import annotations

import re

import numpy as np
import torch

import text_cases as TC
import text_model as M
from mxstream.ops.ingest import DeviceDict, TextIngest
from mxstream.ops.native import load
from mxstream.ops.rowfmt import RowFormatter
from mxstream.runtime.columnar import DeviceColumnBatch
from text_model import FK_DOUBLE, FK_STR

SENT64 = 0x5A5A5A5A5A5A5A5A
SENT32 = 0x5A5A5A5A
SENT8 = 0xEE
FILL = 0x39  # '9' around the text: a read past either end of it would change a parsed number
GUARD = 8    # sentinel words kept after every output


class Expect:
    """What the model says about one case."""

    def __init__(self, c, in_parse_text: bool):
        self.lines = M.split_lines(c.data)
        self.n = len(self.lines)
        self.starts = M.line_starts(c.data)
        assert len(self.starts) == self.n
        self.rows = M.parse_batch(c.data, c.spec, c.sep, c.offset_s)
        self.bad = [isinstance(r, M.JavaError) for r in self.rows]
        self.first_bad = self.bad.index(True) if any(self.bad) else None
        self.needs = [M.line_needs_host(l, c.spec, c.sep, in_parse_text, c.offset_s) for l in self.lines]
        assert all(nh for nh, b in zip(self.needs, self.bad) if b)
        self.str_cols = [j for j, (_, k) in enumerate(c.spec) if k == FK_STR]

    def str_rows(self) -> list[list[bytes]]:
        """The string fields of every line before the first invalid one."""
        k = self.n if self.first_bad is None else self.first_bad
        return [[r[j] for j in self.str_cols] for r in self.rows[:k]]

    def field_pos(self, c, li: int, fi: int) -> int:
        """Byte offset in the batch of split field fi of line li."""
        parts = self.lines[li].split(c.sep.encode())
        return self.starts[li] + sum(len(p) for p in parts[:fi]) + fi


def placed(data: bytes, dev, shift: int = 0):
    """The batch on `dev`, `shift` bytes after a 16-byte boundary, FILL bytes on both sides.
    Returns (whole buffer, view of the batch, host copy of the whole buffer)."""
    host = np.full(16 + shift + len(data) + 48, FILL, dtype=np.uint8)
    host[16 + shift:16 + shift + len(data)] = np.frombuffer(data, dtype=np.uint8)
    big = torch.from_numpy(host.copy()).to(dev)
    assert big.data_ptr() % 16 == 0
    view = big[16 + shift:16 + shift + len(data)]
    assert view.data_ptr() % 16 == shift
    return big, view, host


def filled(n: int, dtype, value: int, dev) -> torch.Tensor:
    if dtype == torch.int64:
        value = sent_i64()
    elif dtype == torch.int32:
        value = sent_i32()
    return torch.full((n,), value, dtype=dtype, device=dev)


def stream_of(dev) -> int:
    return torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else 0


def sync(dev) -> None:
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)


def sent_i64() -> int:
    return int(np.uint64(SENT64).astype(np.int64))


def sent_i32() -> int:
    return int(np.uint32(SENT32).astype(np.int32))


def device_line_starts(view: torch.Tensor, nbytes: int, cap_entries: int, max_out: int = -1):
    """line_starts into a sentinel-filled index of cap_entries words. Returns (index, total)."""
    m, dev = load(), view.device
    idx = filled(cap_entries, torch.int64, SENT64, dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    if dev.type == "cuda":
        scratch = torch.zeros(max(1, m.gpu_filter_compact_scratch_bytes(max(nbytes, 1))),
                              dtype=torch.uint8, device=dev)
        m.gpu_line_starts(view.data_ptr(), nbytes, scratch.data_ptr(), idx.data_ptr(),
                          total.data_ptr(), stream_of(dev), max_out)
    else:
        assert max_out < 0
        m.cpu_line_starts(view.data_ptr(), nbytes, idx.data_ptr(), total.data_ptr())
    sync(dev)
    return idx.cpu().numpy(), int(total.item())


def check_line_starts(data: bytes, idx: np.ndarray, total: int, max_out: int = -1) -> None:
    want = M.line_starts(data)
    assert total == len(want)
    k = len(want) if max_out < 0 else min(max_out, len(want))
    assert idx[:k].tolist() == want[:k]
    assert (idx[k:] == sent_i64()).all()  # nothing written past the count / past max_out


# ---- ingest ---------------------------------------------------------------------------------
def run_ingest(c, dd: DeviceDict, shift: int = 0, assign: bool = True) -> dict:
    """ingest_parse (+ dict_assign_new, or dict_resolve alone) on sentinel-filled outputs."""
    m, dev = load(), dd.device
    cuda = dev.type == "cuda"
    e = Expect(c, False)
    n, nf, S, nbytes = e.n, len(c.spec), len(e.str_cols), len(c.data)
    big, view, host = placed(c.data, dev, shift)
    idx, total = device_line_starts(view, nbytes, n + GUARD)
    check_line_starts(c.data, idx, total)
    starts = torch.from_numpy(idx.copy()).to(dev)
    dd.reserve(n * S, nbytes)
    tiles = (n + 255) // 256
    np_ = max(n * S, 1)
    t = {"cols": filled(nf * n + GUARD, torch.int64, SENT64, dev),
         "ids": filled(max(S, 1) * n + GUARD, torch.int32, SENT32, dev),
         "status": filled(n + GUARD, torch.uint8, SENT8, dev),
         "spos": filled(np_ + GUARD, torch.int64, SENT64, dev),
         "slen": filled(np_ + GUARD, torch.int32, SENT32, dev),
         "sjh": filled(np_ + GUARD, torch.int32, SENT32, dev),
         "sslot": filled(np_ + GUARD, torch.int32, SENT32, dev),
         "shash": filled(np_ + GUARD, torch.int64, SENT64, dev),
         "tile_max": filled(tiles + GUARD, torch.int64, SENT64, dev)}
    ctl = torch.zeros(2, dtype=torch.int64, device=dev)
    ctl[1] = M.I64_MIN
    out = {k: v.data_ptr() for k, v in t.items()}
    out.update(nflag=ctl[0:1].data_ptr(), maxts=ctl[1:2].data_ptr())
    spec = {"fields": [f for f, _ in c.spec], "kinds": [k for _, k in c.spec], "ts_col": c.ts_col,
            "offset_s": c.offset_s, "sep": c.sep}
    st = stream_of(dev)
    m.ingest_parse(cuda, view.data_ptr(), nbytes, starts.data_ptr(), n, spec, out, dd.state(), st)
    if S:
        if assign:
            scratch = torch.zeros(max(1, m.gpu_filter_compact_scratch_bytes(max(nbytes, n * S))),
                                  dtype=torch.uint8, device=dev)
            newpos = filled(np_ + GUARD, torch.int64, SENT64, dev)
            m.dict_assign_new(cuda, view.data_ptr(), n, S, out, dd.state(), scratch.data_ptr(),
                              newpos.data_ptr(), st)
        else:
            m.dict_resolve(cuda, view.data_ptr(), n, S, out, dd.state(), st)
    sync(dev)
    got = {k: v.cpu().numpy() for k, v in t.items()}
    got["nflag"], got["maxts"] = (int(x) for x in ctl.tolist())
    got["nflag"] &= 0xFFFFFFFF
    got["cuda"] = cuda
    assert np.array_equal(big.cpu().numpy(), host), "the input text was written to"
    dd.note_counters(dd.ctr.tolist())
    return got


def check_ingest(c, got: dict, known: dict) -> None:
    """`known` (bytes -> id) is the model's dictionary before the batch; it is updated."""
    e = Expect(c, False)
    n, nf, S = e.n, len(c.spec), len(e.str_cols)
    status = got["status"]
    print(f"{c.name}: {n} lines, {int(status[:n].sum())} flagged, {sum(e.needs)} may be")
    assert set(status[:n].tolist()) <= {0, 1}
    for i in range(n):
        if not e.needs[i]:
            assert status[i] == 0, f"line {i} {e.lines[i]!r} is inside the fast path but flagged"
        if e.bad[i]:
            assert status[i] == 1, f"line {i} {e.lines[i]!r} is invalid but not flagged"
    assert got["nflag"] == int(status[:n].sum())
    cols = got["cols"]
    tile_max = [M.I64_MIN] * ((n + 255) // 256)
    for i in range(n):
        if status[i]:
            continue
        for j, (_, k) in enumerate(c.spec):
            if k != FK_STR:
                assert int(cols[j * n + i]) == e.rows[i][j], (i, j, e.lines[i])
        if c.ts_col >= 0:
            tile_max[i // 256] = max(tile_max[i // 256], e.rows[i][c.ts_col])
    # every tile's slot is written exactly once, by whichever of the two launches owns the tile
    # (the C++ twin keeps one running maximum and leaves the slots alone)
    if got["cuda"]:
        assert got["tile_max"][:len(tile_max)].tolist() == tile_max
    else:
        assert (got["tile_max"] == sent_i64()).all()
    assert got["maxts"] == max(tile_max)
    # string fields: described for every line that has them, flagged or not
    for i in range(n):
        parts = M.java_split(e.lines[i], c.sep.encode())
        for s, j in enumerate(e.str_cols):
            p, fi = i * S + s, c.spec[j][0]
            if fi >= len(parts):
                assert got["slen"][p] == -1
                continue
            assert got["slen"][p] == len(parts[fi])
            assert got["spos"][p] == e.field_pos(c, i, fi)
            assert got["sjh"][p] == M.java_hash(parts[fi]), (i, parts[fi])
    if S and e.first_bad is None:
        ids, _ = M.assign_ids(e.str_rows(), known)
        for i in range(n):
            for s in range(S):
                assert got["ids"][s * n + i] == ids[i][s], (i, s)
    # nothing past the outputs
    assert (cols[nf * n:] == sent_i64()).all()
    assert (status[n:] == SENT8).all()
    assert (got["tile_max"][len(tile_max):] == sent_i64()).all()
    if S:
        assert (got["ids"][S * n:] == sent_i32()).all()
        for k in ("slen", "sjh", "sslot"):
            assert (got[k][n * S:] == sent_i32()).all()
        for k in ("spos", "shash"):
            assert (got[k][n * S:] == sent_i64()).all()


def check_dictionary(dd: DeviceDict, known: dict) -> None:
    """Ids, bytes and Java hashes of the device dictionary equal the model's."""
    names = sorted(known, key=known.get)
    ctr = dd.ctr.tolist()
    assert ctr[0] == len(names) and ctr[2] == 0
    assert ctr[1] == sum(len(b) for b in names)
    off = dd.id_off[:len(names)].cpu().numpy()
    ln = dd.id_len[:len(names)].cpu().numpy()
    arena = dd.arena.cpu().numpy().tobytes()
    assert [arena[o:o + k] for o, k in zip(off.tolist(), ln.tolist())] == names
    assert dd.jhash_table().tolist() == [M.java_hash(b) for b in names]
    # the arena ranges tile [0, used) without overlap
    spans = sorted(zip(off.tolist(), ln.tolist()))
    pos = 0
    for o, k in spans:
        assert o == pos
        pos += k
    # every assigned slot of the table points at an id whose hash slot it is, once
    tab_id = dd.tab_id.cpu().numpy()
    assert sorted(tab_id[tab_id >= 0].tolist()) == list(range(len(names)))


# ---- end to end ------------------------------------------------------------------------------
def raised_kind(exc: BaseException) -> str:
    name = type(exc).__name__
    if name in (M.NFE, M.AIOOBE, M.DTPE):
        return name
    m = re.search(r"(\w+Exception)", str(exc))
    return m.group(1) if m else name


def raised_line(exc: BaseException):
    m = re.match(r"line (\d+):", str(exc))
    return int(m.group(1)) - 1 if m else None


def check_text_ingest(c, device, dd: DeviceDict | None = None, known: dict | None = None):
    """TextIngest.parse (kernels or twins, then the host patch) against the model."""
    e = Expect(c, False)
    ing = TextIngest(c.spec, c.sep, offset_s=c.offset_s, ts_field=c.ts_col, device=device, dictionary=dd)
    known = {} if known is None else known
    if e.first_bad is not None:
        try:
            ing.parse(c.data)
        except Exception as exc:  # noqa: BLE001 - the class is what is checked
            assert raised_kind(exc) == e.rows[e.first_bad].kind, (c.name, exc)
            assert raised_line(exc) in (None, e.first_bad)
            return ing
        raise AssertionError(f"{c.name}: line {e.first_bad} {e.lines[e.first_bad]!r} did not raise")
    res = ing.parse(c.data)
    assert res.n == e.n
    ids, _ = M.assign_ids(e.str_rows(), known)
    for j, (_, k) in enumerate(c.spec):
        col = res.cols[j].cpu().numpy()
        if k == FK_STR:
            s = e.str_cols.index(j)
            assert col.tolist() == [r[s] for r in ids]
        elif k == FK_DOUBLE:
            assert col.view(np.int64).tolist() == [r[j] for r in e.rows]
        else:
            assert col.tolist() == [r[j] for r in e.rows]
    if c.ts_col >= 0 and e.n:
        assert res.max_ts == max(r[c.ts_col] for r in e.rows)
    check_dictionary(ing.dict, known)
    return ing


# ---- row format -----------------------------------------------------------------------------
def run_format(dev, cols, kinds, dd, sub, prefixes, as_tuple: bool, shift: int = 0):
    """format_rows_len + format_rows_write, the output `shift` bytes after a 16-byte boundary.
    cols: numpy columns (int32 ids for strings). Returns (lengths, bad flag, bytes)."""
    m = load()
    gpu = dev.type == "cuda"
    n = len(cols[0])
    keep = [torch.from_numpy(np.ascontiguousarray(c)).to(dev) for c in cols]
    kind_of = {M.FK_STR: 0, M.FK_DOUBLE: 1}
    d = {"cols": [(kind_of.get(k, 2), t.element_size(), t.data_ptr()) for t, k in zip(keep, kinds)],
         "as_tuple": bool(as_tuple), "arena": 0, "id_off": 0, "id_len": 0, "n_ids": 0, "sub": 0,
         "sub0": 0, "par": 1, "npfx": 0, "pfx": 0, "pfx_off": 0}
    if dd is not None:
        d.update(arena=dd.arena.data_ptr(), id_off=dd.id_off.data_ptr(), id_len=dd.id_len.data_ptr(),
                 n_ids=int(dd.n_ids))
    if prefixes:
        enc = [p.encode() for p in prefixes]
        off = np.zeros(len(enc) + 1, dtype=np.int32)
        off[1:] = np.cumsum([len(b) for b in enc])
        pfx = torch.from_numpy(np.frombuffer(b"".join(enc), dtype=np.uint8).copy()).to(dev)
        poff = torch.from_numpy(off).to(dev)
        tsub = torch.from_numpy(np.ascontiguousarray(sub, dtype=np.int32)).to(dev)
        keep += [pfx, poff, tsub]
        d.update(npfx=len(enc), pfx=pfx.data_ptr(), pfx_off=poff.data_ptr(), sub=tsub.data_ptr())
    st = stream_of(dev)
    ln = filled(n + GUARD, torch.int64, SENT64, dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    m.format_rows_len(gpu, d, n, ln.data_ptr(), bad.data_ptr(), st)
    sync(dev)
    lens = ln.cpu().numpy()
    assert (lens[n:] == sent_i64()).all()
    end = torch.cumsum(ln[:n], 0)
    total = int(end[-1].item())
    big = filled(16 + shift + total + 48, torch.uint8, SENT8, dev)
    assert big.data_ptr() % 16 == 0
    if not int(bad.item()):
        m.format_rows_write(gpu, d, n, end.data_ptr(), big.data_ptr() + 16 + shift, st)
        sync(dev)
    raw = big.cpu().numpy()
    assert (raw[:16 + shift] == SENT8).all() and (raw[16 + shift + total:] == SENT8).all()
    del keep
    return lens[:n], int(bad.item()), raw[16 + shift:16 + shift + total].tobytes()


def model_format(values, kinds, names, sub, prefixes, as_tuple: bool) -> list[bytes]:
    """values: numpy columns as given to run_format; names: the dictionary's strings by id."""
    rows = []
    for i in range(len(values[0])):
        cells = [names[int(v[i])] if k == M.FK_STR else (float(v[i]) if k == M.FK_DOUBLE else int(v[i]))
                 for v, k in zip(values, kinds)]
        rows.append(M.format_row(cells, kinds, prefixes[int(sub[i])] if prefixes else "", as_tuple))
    return rows


def check_format(dev, cols, kinds, dd, names, sub, prefixes, as_tuple: bool, shift: int = 0) -> int:
    rows = model_format(cols, kinds, names, sub, prefixes, as_tuple)
    lens, bad, raw = run_format(dev, cols, kinds, dd, sub, prefixes, as_tuple, shift)
    assert bad == 0
    assert lens.tolist() == [len(r) for r in rows]
    assert raw == b"".join(rows)
    return len(raw)


def fmt_dict(dev):
    """The formatter's dictionary, built by dict_insert_ids from a table that has to grow."""
    names = TC.fmt_names()
    dd = DeviceDict(dev, cap=8, id_cap=4, arena_cap=16)
    dd.add_agreed(names)
    return dd, names


def format_checks(dev):
    """Sizes around the 256-row tile, tuple and bare rows, with and without subtask prefixes,
    the output at four alignments."""
    dd, names = fmt_dict(dev)
    check_dictionary(dd, {b: i for i, b in enumerate(names)})
    kinds = (M.FK_STR, M.FK_LONG, M.FK_DOUBLE)
    pfx = ["1> ", "2> ", "13> "]
    for n in TC.FMT_ROWS:
        ids, lv, dv, sub = TC.fmt_columns(n, n)
        for shift, prefixes in ((0, pfx), (1, None), (15, pfx)):
            check_format(dev, [ids, lv, dv], kinds, dd, names, sub, prefixes, True, shift)
        check_format(dev, [dv], (M.FK_DOUBLE,), None, names, sub, pfx, False, 1)
        check_format(dev, [lv], (M.FK_LONG,), None, names, sub, None, False, 15)
        check_format(dev, [ids], (M.FK_STR,), dd, names, sub, None, False, 0)
        check_format(dev, [lv.astype(np.int32), ids.astype(np.int64)], (M.FK_INT, M.FK_STR), dd,
                     names, sub, None, True, 7)
    return dd, names


def format_budget_checks(dev, dd, names):
    """One 256-row tile of exactly 32768 - pad bytes (through LDS) and one byte more (straight
    to memory), at pad 0, 1 and 15; then three tiles whose middle one goes straight to memory."""
    kinds = (M.FK_STR, M.FK_LONG, M.FK_DOUBLE)
    sub = np.zeros(256, np.int32)
    lv, dv = np.full(256, 7, np.int64), np.full(256, 1.5)
    for pad in (0, 1, 15):
        for over in (0, 1):
            total = TC.FMT_TILE_BYTES - pad + over
            ids = np.array(TC.fmt_exact_tile_ids(total, names, len("(,7,1.5)\n")), np.int32)
            assert check_format(dev, [ids, lv, dv], kinds, dd, names, sub, None, True, pad) == total
    by_len = {len(b): i for i, b in enumerate(names)}
    ids = np.array([3] * 256 + [by_len[130]] * 256 + [5] * 88, np.int32)
    ids[300], ids[511] = by_len[140], by_len[100]
    _, lv, dv, sub = TC.fmt_columns(ids.size, 77)
    for shift in (0, 1, 15):
        check_format(dev, [ids, lv, dv], kinds, dd, names, sub, ["1> ", "2> ", "3> "], True, shift)


def row_formatter_checks(dev, dd, names, also=None):
    """RowFormatter.format (lengths, scan, write, copy) against the model; also(cols, kinds,
    sub, prefixes, as_tuple, want): a further formatter to hold against the same bytes."""
    kinds = (M.FK_STR, M.FK_LONG, M.FK_DOUBLE)
    for n in TC.FMT_ROWS:
        ids, lv, dv, sub = TC.fmt_columns(n, n)
        for pfx, as_tuple, cols, kk in ((["1> ", "2> ", "3> "], True, [ids, lv, dv], kinds),
                                        ([""], True, [ids, lv, dv], kinds),
                                        (["1> ", "2> ", "3> "], False, [dv], (M.FK_DOUBLE,)),
                                        ([""], False, [lv], (M.FK_LONG,))):
            s = sub if any(pfx) else np.zeros(n, np.int32)
            want = b"".join(model_format(cols, kk, names, s, pfx, as_tuple))
            cb = DeviceColumnBatch(n, [torch.as_tensor(c).to(dev) for c in cols], kk, dd, None,
                                   sub_dev=torch.as_tensor(s).to(dev))
            got = RowFormatter().format(cb, pfx, as_tuple)
            assert got is not None and bytes(got) == want
            if also is not None:
                also(cols, kk, s, pfx, as_tuple, want)


# ---- whole checks, for either device --------------------------------------------------------------
def ingest_direct(c, dev, shift: int = 0):
    """One case through ingest_parse + dict_assign_new on a fresh dictionary."""
    dd, known = DeviceDict(dev), {}
    check_ingest(c, run_ingest(c, dd, shift), known)
    if Expect(c, False).first_bad is None:
        check_dictionary(dd, known)


def dictionary_growth_checks(dev):
    """300 strings into a dictionary of 8 slots, 4 ids and 16 arena bytes (dict_rehash and the
    growth of every array, several times), then a batch of known strings; directly, then
    through TextIngest."""
    dd, known = DeviceDict(dev, cap=8, id_cap=4, arena_cap=16), {}
    before = 0
    for c in TC.growth_batches():
        before = len(known)
        check_ingest(c, run_ingest(c, dd), known)
        check_dictionary(dd, known)
    assert len(known) == 300 == before  # the last batch added nothing
    dd2, known2 = DeviceDict(dev, cap=8, id_cap=4, arena_cap=16), {}
    for c in TC.growth_batches():
        check_text_ingest(c, dev, dd2, known2)


def agreed_ids_checks(dev):
    """dict_insert_ids (the agreed list of several ranks), then a batch resolved against it
    without assignment: ids are the list's order, not the batch's order of appearance."""
    c = TC.string_case()
    names = sorted({s for row in Expect(c, False).str_rows() for s in row}, key=lambda b: (len(b), b))
    dd = DeviceDict(dev, cap=8, id_cap=4, arena_cap=16)
    dd.add_agreed(names[:5])
    dd.add_agreed(names[5:])
    known = {b: i for i, b in enumerate(names)}
    check_dictionary(dd, known)
    check_ingest(c, run_ingest(c, dd, assign=False), known)
    check_dictionary(dd, known)  # nothing was added
