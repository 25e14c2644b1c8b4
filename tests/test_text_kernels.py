"""The gfx950 text kernels against the plain model (tests/text_model.py), on the cases of
tests/text_cases.py: ``line_start_mask_kernel`` and its compaction (``gpu_line_starts``),
``parse_text_kernel`` (``gpu_parse_text``, raw status array and flag counter),
``ingest_parse_kernel<false>`` / ``<true>`` (``ingest_parse``), the five dictionary kernels
(``dict_assign_new`` = new-string mask + assign + commit + resolve, ``dict_resolve``,
``dict_rehash``, ``dict_insert_ids``), ``fmt_len_kernel`` / ``fmt_write_kernel``
(``format_rows_len`` / ``format_rows_write``); then once more through ``parse_text_gpu``,
``TextIngest(device=gpu)`` and ``RowFormatter`` for the result after the host patch.

Per case: every line inside the documented fast path (``needs_host`` false) has status 0, so a
kernel cannot pass by flagging everything; the flag counter is the number of status-1 lines;
every column word, Java hash, key and id of a status-0 line equals the model bit for bit; the
end-to-end result equals the model, or raises the model's exception class for the first invalid
line; ``max_ts`` and (ingest) every tile's ``tile_max`` slot equal the model's maxima over the
unflagged lines; outputs keep their sentinels past the last word; the text is not written to.
No tolerance anywhere: the reference defines every operation exactly.

Which case takes which global-memory fallback (a 256-line tile's bytes plus its address
modulo 16 against the LDS budget):

* ``parse_text_kernel`` global path: ``tile24576-pad{0,1,15}-over1`` (one byte over; the
  ``-over0`` twins are the last size that stages in LDS), ``tiles24576-none-fit``,
  ``one-30000-byte-line``; mixed: ``tiles24576-mixed`` (LDS, global, LDS).
* ``ingest_parse_kernel<true>``: ``tile16384-pad{0,1,15}-over1``, ``tiles16384-none-fit``,
  ``one-30000-byte-line`` and the two ``tile24576-pad0`` shapes; mixed: ``tiles16384-mixed``,
  where the middle tile and the batch maximum belong to the second launch and every
  ``tile_max`` slot, status and column must still be written exactly once.
* ``fmt_write_kernel`` direct path: ``format_budget_checks``' tiles of 32768 - pad + 1 bytes
  (pad 0, 1, 15; 32768 - pad goes through LDS); mixed: its 600-row batch (LDS, direct, LDS).
* ``stage_line_tile``'s head / body / tail split: every shape above at pad 0, 1 and 15 (the
  batch sits pad bytes after a 16-byte boundary of a larger buffer), ``tile-shorter-than-head``
  (3 bytes at pad 1: nb < head), ``tiles{24576,16384}-offset`` (a second tile whose offset in the
  batch is 15 mod 16 while its address is aligned, 8 bytes under the budget: pad must come from
  the address, and ``tile_fits_lds`` and ``stage_line_tile`` must agree) and, inside the mixed
  batches, tiles that start wherever the lines before them end.

Not tested: a format batch above 8192 * 256 rows, the only shape at which ``fmt_len_kernel``
takes a second grid-stride round; no test-sized input reaches it.
"""
import numpy as np
import pytest
import torch

import text_cases as TC
import text_checks as K
import text_model as M
from mxstream.ops import text as T
from mxstream.ops.native import load

pytestmark = pytest.mark.gpu

PARSE_CASES = TC.parse_cases() + TC.all_invalid_in_one()
PARSE_TEXT_CASES = [c for c in PARSE_CASES if all(k <= M.FK_RAW_LONG for _, k in c.spec)]
PARSE_BUDGET = TC.budget_cases(TC.PARSE_TILE_BYTES)
INGEST_BUDGET = TC.budget_cases(TC.INGEST_TILE_BYTES) + TC.budget_cases(TC.PARSE_TILE_BYTES)[:2]


def _ids(cases):
    return [c.name for c in cases]


def _pad_ids(cases):
    return [f"{c.name}@{pad}" for c, pad in cases]


# ---- line starts ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", TC.LINE_START_SIZES)
def test_line_starts_equal_model(gpu_device, n):
    for seed in (0, 1):
        data = TC.line_start_bytes(n, seed)
        count = len(M.line_starts(data))
        for shift in TC.LINE_START_SHIFTS:
            big, view, host = K.placed(data, gpu_device, shift)
            idx, total = K.device_line_starts(view, n, count + K.GUARD)
            K.check_line_starts(data, idx, total)
            # fewer entries than lines: every line is counted, max_out starts are written
            for max_out in {0, 1, count // 2, count - 1} - {-1, count}:
                idx, total = K.device_line_starts(view, n, count + K.GUARD, max_out)
                K.check_line_starts(data, idx, total, max_out)
            assert np.array_equal(big.cpu().numpy(), host)


# ---- parse_text -------------------------------------------------------------------------------
def run_parse_text(c, dev, shift=0, extra_bound=0):
    """gpu_parse_text on sentinel-filled outputs; extra_bound > 0: the outputs' bound exceeds the
    line count, which the kernel then reads from the device (parse_text_gpu's arrangement)."""
    m = load()
    e = K.Expect(c, True)
    n, nf, nbytes = e.n, len(c.spec), len(c.data)
    big, view, host = K.placed(c.data, dev, shift)
    idx, total = K.device_line_starts(view, nbytes, n + extra_bound + K.GUARD)
    K.check_line_starts(c.data, idx, total)
    starts = torch.from_numpy(idx.copy()).to(dev)
    words = nf * (n + extra_bound) + K.GUARD
    cols = K.filled(words, torch.int64, K.SENT64, dev)
    jh = K.filled(words, torch.int32, K.SENT32, dev)
    status = K.filled(n + extra_bound + K.GUARD, torch.uint8, K.SENT8, dev)
    ctl = torch.zeros(2, dtype=torch.int64, device=dev)
    ctl[0] = n
    m.gpu_parse_text(view.data_ptr(), nbytes, starts.data_ptr(), n + extra_bound,
                     [f for f, _ in c.spec], [k for _, k in c.spec], c.sep, c.offset_s,
                     cols.data_ptr(), jh.data_ptr(), status.data_ptr(), K.stream_of(dev),
                     nlines_dev=ctl[0:1].data_ptr() if extra_bound else 0, nflag=ctl[1:2].data_ptr())
    K.sync(dev)
    assert np.array_equal(big.cpu().numpy(), host), "the input text was written to"
    return cols.cpu().numpy(), jh.cpu().numpy(), status.cpu().numpy(), int(ctl[1].item()) & 0xFFFFFFFF


def check_parse_text(c, cols, jh, status, nflag):
    e = K.Expect(c, True)
    n, nf = e.n, len(c.spec)
    print(f"{c.name}: {n} lines, {int(status[:n].sum())} flagged, {sum(e.needs)} may be")
    assert set(status[:n].tolist()) <= {0, 1}
    for i in range(n):
        if not e.needs[i]:
            assert status[i] == 0, f"line {i} {e.lines[i]!r} is inside the fast path but flagged"
        if e.bad[i]:
            assert status[i] == 1, f"line {i} {e.lines[i]!r} is invalid but not flagged"
    assert nflag == int(status[:n].sum())
    for i in range(n):
        if status[i]:
            continue
        for j, (_, kind) in enumerate(c.spec):
            if kind == M.FK_STR:
                assert int(cols[j * n + i]) == M.fnv1a64(e.rows[i][j]), (i, j, e.lines[i])
                assert int(jh[j * n + i]) == M.java_hash(e.rows[i][j]), (i, j, e.lines[i])
            else:
                assert int(cols[j * n + i]) == e.rows[i][j], (i, j, e.lines[i])
    for j, (_, kind) in enumerate(c.spec):  # only string columns have a Java hash
        if kind != M.FK_STR:
            assert (jh[j * n:(j + 1) * n] == K.sent_i32()).all()
    assert (cols[nf * n:] == K.sent_i64()).all() and (jh[nf * n:] == K.sent_i32()).all()
    assert (status[n:] == K.SENT8).all()


def check_parse_text_gpu(c, dev, data=None):
    """parse_text_gpu (kernel + host patch) against the model."""
    e = K.Expect(c, True)
    data = c.data if data is None else data
    if e.first_bad is not None:
        with pytest.raises(T.ParseError) as ei:
            T.parse_text_gpu(data, c.spec, c.sep, c.offset_s, dev)
        assert K.raised_kind(ei.value) == e.rows[e.first_bad].kind, (c.name, ei.value)
        assert K.raised_line(ei.value) == e.first_bad, (c.name, ei.value)
        return
    got = T.parse_text_gpu(data, c.spec, c.sep, c.offset_s, dev)
    for j, (_, kind) in enumerate(c.spec):
        want = [r[j] for r in e.rows]
        if kind == M.FK_STR:
            assert got[j][0].cpu().tolist() == [M.fnv1a64(b) for b in want], c.name
            assert got[j][1].cpu().tolist() == [M.java_hash(b) for b in want], c.name
        elif kind == M.FK_DOUBLE:
            assert got[j].dtype == torch.float64
            assert got[j].view(torch.int64).cpu().tolist() == want, c.name
        else:
            assert got[j].cpu().tolist() == want, c.name


@pytest.mark.parametrize("c", PARSE_TEXT_CASES, ids=_ids(PARSE_TEXT_CASES))
def test_parse_text_equals_model(gpu_device, c):
    check_parse_text(c, *run_parse_text(c, gpu_device))


@pytest.mark.parametrize("c", PARSE_TEXT_CASES, ids=_ids(PARSE_TEXT_CASES))
def test_parse_text_gpu_equals_model(gpu_device, c):
    check_parse_text_gpu(c, gpu_device)


@pytest.mark.parametrize("c,pad", PARSE_BUDGET, ids=_pad_ids(PARSE_BUDGET))
def test_parse_text_lds_budget(gpu_device, c, pad):
    check_parse_text(c, *run_parse_text(c, gpu_device, pad))


def test_parse_text_reads_the_device_line_count(gpu_device):
    """Outputs sized for a bound above the line count: the kernel takes the count (and the
    column stride) from the device, and workgroups past it leave everything alone."""
    for c in (TC.geometry_cases()[0], TC.mixed_tiles_case(TC.PARSE_TILE_BYTES), TC.string_case()):
        check_parse_text(c, *run_parse_text(c, gpu_device, 0, extra_bound=300))


def test_parse_text_gpu_redoes_a_batch_of_short_lines(gpu_device):
    """600 lines of 4 bytes: more lines than parse_text_gpu's first bound, so line_starts writes
    only the bound and the batch is redone with the exact size. Device and pinned input too."""
    c = TC.case("short-lines", "".join(f"{i % 10} {(i * 7) % 10}\n" for i in range(600)),
                [(1, M.FK_LONG), (0, M.FK_STR)])
    assert len(c.data) // 8 + 256 < 600
    check_parse_text_gpu(c, gpu_device)
    check_parse_text_gpu(c, gpu_device, torch.frombuffer(bytearray(c.data), dtype=torch.uint8).to(gpu_device))
    check_parse_text_gpu(TC.string_case(), gpu_device, T.pinned_text_batch(TC.string_case().data))


def test_invalid_tokens_raise_the_models_exception(gpu_device):
    for c in TC.invalid_cases():
        assert K.Expect(c, False).first_bad == 1, c.name
        check_parse_text_gpu(c, gpu_device)
        K.check_text_ingest(c, gpu_device)


# ---- ingest + dictionary ----------------------------------------------------------------------
@pytest.mark.parametrize("c", PARSE_CASES, ids=_ids(PARSE_CASES))
def test_ingest_equals_model(gpu_device, c):
    K.ingest_direct(c, gpu_device)


@pytest.mark.parametrize("c", PARSE_CASES, ids=_ids(PARSE_CASES))
def test_text_ingest_gpu_equals_model(gpu_device, c):
    K.check_text_ingest(c, gpu_device)


@pytest.mark.parametrize("c,pad", INGEST_BUDGET, ids=_pad_ids(INGEST_BUDGET))
def test_ingest_lds_budget(gpu_device, c, pad):
    K.ingest_direct(c, gpu_device, pad)


def test_ingest_mixed_tiles_end_to_end(gpu_device):
    for c in (TC.mixed_tiles_case(TC.INGEST_TILE_BYTES), TC.no_tile_fits_case(TC.INGEST_TILE_BYTES),
              TC.long_line_case()):
        K.check_text_ingest(c, gpu_device)
        check_parse_text_gpu(c, gpu_device)


def test_dictionary_grows_and_rehashes(gpu_device):
    K.dictionary_growth_checks(gpu_device)


def test_agreed_ids_then_resolve(gpu_device):
    K.agreed_ids_checks(gpu_device)


# ---- row format -------------------------------------------------------------------------------
def test_row_format_equals_model(gpu_device):
    dd, names = K.format_checks(gpu_device)
    K.format_budget_checks(gpu_device, dd, names)
    K.row_formatter_checks(gpu_device, dd, names)
