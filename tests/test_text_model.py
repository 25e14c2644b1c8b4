"""The host side of the text path against the plain model (tests/text_model.py), on the cases of
tests/text_cases.py: the host parser (``parse_lines`` + ``StringDict``, csrc/runtime.cpp), the
C++ twins of the ingest, dictionary, line-start and row-format kernels (called directly and
through ``TextIngest(device="cpu")`` / ``RowFormatter``), and ``java_format_bytes``.

The twins, the host parser and the gfx950 kernels share ``parse_long_ascii``,
``iso_local_datetime``, ``java_hash_utf8`` (csrc/mxs_common.h) and ``fast_parse_double``
(csrc/ingest.h); comparing them with one another cannot see a mistake in those. The model shares
no code with them. Values are compared bit for bit, errors by Java exception class and line.
tests/test_text_kernels.py sends the same cases to the kernels.
"""
import numpy as np
import pytest
import torch

import text_cases as TC
import text_checks as K
import text_model as M
from mxstream.ops import text as T
from mxstream.ops.native import load

CPU = torch.device("cpu")
PARSE_CASES = TC.parse_cases() + TC.all_invalid_in_one()
BUDGET_CASES = TC.budget_cases(TC.PARSE_TILE_BYTES) + TC.budget_cases(TC.INGEST_TILE_BYTES)


def _ids(cases):
    return [c.name for c in cases]


# ---- the model itself: anchors taken from Java, not from the project ----------------------------
def test_model_anchors():
    assert M.java_split("a b  ", " ") == ["a", "b"] and M.java_split("", " ") == [""]
    assert M.java_split("   ", " ") == [] and M.java_split(" a", " ") == ["", "a"]
    assert M.java_hash("hello") == 99162322 and M.java_hash("") == 0
    assert M.java_hash("\U0001F600") == 0xD83D * 31 + 0xDE00  # a surrogate pair
    assert M.java_hash(b"\xff") == 0xFFFD
    assert M.java_hash("polygenelubricants") == -(1 << 31)  # Integer.MIN_VALUE, a known example
    assert M.parse_iso("2019-07-18T20:14:16", 8 * 3600)[0] == 1563452056000
    assert M.parse_iso("1970-01-01T00:00", 0) == (0, 0, 0)
    assert M.parse_iso("2038-01-19T03:14:08", 0)[1:] == (-(1 << 31) * 1000, -(1 << 31))
    assert M.parse_iso("1969-12-31T23:59:59.250", 0)[0] == -750
    assert M.parse_long("-9223372036854775808") == M.I64_MIN
    assert M.f64_bits(M.parse_double(" 87.5d\t")) == M.f64_bits(87.5)
    for bad in ("1_0", "inf", "nan", " 1.5", "٣", "0x10"):
        with pytest.raises(M.JavaError):
            M.parse_double(bad)
    with pytest.raises(M.JavaError):
        M.parse_long("٣")
    assert M.fnv1a64(b"") == 0xCBF29CE484222325 - (1 << 64)
    assert not M.needs_host(b"123456789012345e22", M.FK_DOUBLE, True)
    assert M.needs_host(b"123456789012345e23", M.FK_DOUBLE, True)
    assert not M.needs_host(b"1.5e23", M.FK_DOUBLE, True)  # net exponent 22
    assert M.needs_host(b"1e00005", M.FK_DOUBLE, True) and M.needs_host(b"87.5d", M.FK_DOUBLE, True)
    assert M.needs_host(b"1e23", M.FK_DOUBLE, True) and not M.needs_host(b"1e22", M.FK_DOUBLE, True)
    assert not M.needs_host(b"0" * 21 + b"1", M.FK_DOUBLE, True)
    assert M.needs_host(b"1000000000000000", M.FK_DOUBLE, True)  # 16 digits, trailing zeros count
    assert M.needs_host("é".encode(), M.FK_STR, True) and not M.needs_host("é".encode(), M.FK_STR, False)
    assert M.format_row([b"h", 1.0, -5], (M.FK_STR, M.FK_DOUBLE, M.FK_LONG), "2> ", True) == b"2> (h,1.0,-5)\n"
    assert M.format_row([0.001], (M.FK_DOUBLE,), "", False) == b"0.001\n"


def test_scalar_bindings_equal_model(native):
    for row in K.Expect(TC.string_case(), False).str_rows():
        for s in row:
            assert native.java_string_hash(s) == M.java_hash(s), s
            assert T.fnv1a64(s) == M.fnv1a64(s)
    for t in TC.DOUBLE_EDGES + TC.random_decimal_texts(2000, seed=5):
        assert M.f64_bits(native.java_parse_double(t)) == M.f64_bits(M.parse_double(t)), t
    for t in TC.DOUBLE_INVALID:
        with pytest.raises(Exception, match="NumberFormatException"):
            native.java_parse_double(t)
    for t in TC.valid_dates():
        for off in (0, TC.H8, TC.HM5):
            assert native.iso_to_epoch_ms(t, off) == M.parse_iso(t, off)[0], t
    for t in TC.DATE_INVALID:
        with pytest.raises(Exception, match="DateTimeParseException"):
            native.iso_to_epoch_ms(t, 0)


# ---- the host parser ----------------------------------------------------------------------------
def _check_host(c, threads=1):
    m = load()
    e = K.Expect(c, False)
    d = m.StringDict()
    cols, nparsed, err_idx, err = m.parse_lines(c.data, c.spec, c.sep, d, c.offset_s, threads)
    k = e.n if e.first_bad is None else e.first_bad
    if e.first_bad is None:
        assert not err and err_idx < 0, err
    else:
        assert err_idx == k, (err_idx, err, e.lines[k])
        assert err.split(":")[0] == e.rows[k].kind, (err, e.lines[k])
    assert nparsed == k
    ids, known = M.assign_ids(e.str_rows()[:k])
    for j, (_, kind) in enumerate(c.spec):
        col = np.asarray(cols[j])[:k]
        if kind == M.FK_STR:
            s = e.str_cols.index(j)
            assert col.astype(np.int64).tolist() == [r[s] for r in ids]
        elif kind == M.FK_DOUBLE:
            assert col.view(np.int64).tolist() == [r[j] for r in e.rows[:k]]
        else:
            assert col.tolist() == [r[j] for r in e.rows[:k]]
    names = sorted(known, key=known.get)
    assert len(d) == len(names)
    assert d.jhash_table().tolist() == [M.java_hash(b) for b in names]
    try:
        assert d.strings() == [b.decode() for b in names]
    except UnicodeDecodeError:  # a key that is not UTF-8 has no str; its hash was compared above
        assert any(b.decode(errors="replace").encode() != b for b in names)


@pytest.mark.parametrize("c", PARSE_CASES, ids=_ids(PARSE_CASES))
def test_host_parser_equals_model(c):
    _check_host(c)


def test_host_parser_threads_equal_model():
    for c in (TC.number_cases()[0], TC.string_case(), TC.date_cases()[1]):
        _check_host(c, threads=4)


def test_invalid_tokens_raise_the_models_exception():
    for c in TC.invalid_cases():
        e = K.Expect(c, False)
        assert e.first_bad == 1, c.name  # the model rejects exactly the middle line
        _check_host(c)
        K.check_text_ingest(c, CPU)


# ---- the C++ twins, called directly ---------------------------------------------------------------
@pytest.mark.parametrize("c", PARSE_CASES, ids=_ids(PARSE_CASES))
def test_twin_ingest_equals_model(c):
    K.ingest_direct(c, CPU)


@pytest.mark.parametrize("c,pad", BUDGET_CASES, ids=[f"{c.name}@{pad}" for c, pad in BUDGET_CASES])
def test_twin_ingest_budget_shapes(c, pad):
    """The twin has no LDS tile; the shapes that split the kernels' tiles must not matter to it."""
    K.ingest_direct(c, CPU, pad)


@pytest.mark.parametrize("c", PARSE_CASES, ids=_ids(PARSE_CASES))
def test_text_ingest_cpu_equals_model(c):
    K.check_text_ingest(c, CPU)


@pytest.mark.parametrize("n", TC.LINE_START_SIZES)
def test_twin_line_starts_equal_model(n):
    for seed in (0, 1):
        data = TC.line_start_bytes(n, seed)
        for shift in TC.LINE_START_SHIFTS:
            _, view, _ = K.placed(data, CPU, shift)
            idx, total = K.device_line_starts(view, n, len(M.line_starts(data)) + K.GUARD)
            K.check_line_starts(data, idx, total)


def test_twin_dictionary_grows_and_rehashes():
    K.dictionary_growth_checks(CPU)


def test_twin_agreed_ids_then_resolve():
    K.agreed_ids_checks(CPU)


# ---- row format -----------------------------------------------------------------------------------
def _host_format(cols, kinds, names, sub, prefixes, as_tuple):
    keep, spec = [], []
    for c, k in zip(cols, kinds):
        a = np.ascontiguousarray(c, dtype=np.float64 if k == M.FK_DOUBLE else np.int64)
        spec.append(({M.FK_STR: 0, M.FK_DOUBLE: 1}.get(k, 2), a.ctypes.data))
        keep.append(a)
    s = np.ascontiguousarray(sub, dtype=np.int32)
    return load().java_format_bytes(spec, len(cols[0]), names, s.ctypes.data, prefixes, as_tuple, 1)


def test_twin_row_format_equals_model():
    dd, names = K.format_checks(CPU)
    K.format_budget_checks(CPU, dd, names)


def test_row_formatter_and_host_formatter_equal_model():
    dd, names = K.fmt_dict(CPU)
    strs = [b.decode() for b in names]

    def host(cols, kinds, sub, prefixes, as_tuple, want):
        assert _host_format(cols, kinds, strs, sub, prefixes, as_tuple) == want

    K.row_formatter_checks(CPU, dd, names, also=host)
