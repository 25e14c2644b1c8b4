"""Inputs of the text-path tests, shared by tests/test_text_model.py (CPU: host parser and C++
twins against tests/text_model.py) and tests/test_text_kernels.py (the gfx950 kernels against
the same model). Small, deterministic, seeded; every family is built for a place where a kernel
can go wrong (see the comments). Nothing here calls native code.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import text_model as M
from text_model import FK_DOUBLE, FK_INT, FK_ISO_SEC, FK_LONG, FK_RAW_LONG, FK_STR, FK_TS_INTSEC, FK_TS_MS

# One batch: `spec` = [(split index, kind)], `ts_col` = the ingest column whose maximum is the
# batch's max timestamp (-1: none). Lines may be invalid: the model says which and how.
Case = namedtuple("Case", "name data spec sep offset_s ts_col")


def case(name, data, spec, sep=" ", offset_s=0, ts_col=-1):
    if isinstance(data, str):
        data = data.encode()
    return Case(name, data, list(spec), sep, offset_s, ts_col)


SPEC_METRIC = [(0, FK_LONG), (1, FK_STR), (2, FK_STR), (3, FK_DOUBLE)]
SPEC_REORDER = [(3, FK_DOUBLE), (0, FK_LONG), (2, FK_STR), (1, FK_STR)]  # ingest_line_dev's rescan


def metric_lines(n: int, seed: int = 0) -> list[str]:
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        v = f"{int(rng.integers(0, 100000)) / 10 ** int(rng.integers(0, 4))}"
        out.append(f"{1563452000 + int(rng.integers(0, 5000))} 10.8.{i % 7}.{i % 11} cpu{i % 5} {v}")
    return out


# ---- line geometry --------------------------------------------------------------------------
GEOMETRY_SIZES = (1, 63, 64, 255, 256, 257, 511, 513)


def geometry_cases() -> list[Case]:
    out = []
    # The batch ends with '\n', with nothing, with "\r\n" (every line), with a '\r' and no '\n'.
    ends = [("nl", "\n", "\n"), ("none", "\n", ""), ("crlf", "\r\n", "\r\n"), ("cr-eof", "\n", "\r")]
    for n in GEOMETRY_SIZES:
        for name, join, tail in ends:
            lines = metric_lines(n, seed=n)
            out.append(case(f"geo{n}-{name}", join.join(lines) + tail, SPEC_METRIC, ts_col=0))
    # A '\r' alone on the last line is an empty line: the spec's fields are missing there.
    out.append(case("geo256-lone-cr", "\n".join(metric_lines(256, 256)) + "\n\r", SPEC_METRIC, ts_col=0))
    out.append(case("geo257-reorder", "\n".join(metric_lines(257, 3)) + "\n", SPEC_REORDER, ts_col=1))
    eight = [" ".join([str(i), f"k{i % 3}", f"{i}.25", str(-i), f"s{i % 4}", f"{i}e2", "7", "x", "tail"])
             for i in range(70)]
    out.append(case("geo70-eight-fields", "\n".join(eight) + "\n",
                    [(0, FK_LONG), (1, FK_STR), (2, FK_DOUBLE), (3, FK_INT), (4, FK_STR),
                     (5, FK_DOUBLE), (6, FK_RAW_LONG), (8, FK_STR)], ts_col=6))
    # The last field of the last line ends at the batch's final newline, whatever its kind (a
    # double would hide a kept '\n': parseDouble trims it).
    for kind, a, b in ((FK_STR, "a", "b"), (FK_LONG, "2", "5"), (FK_INT, "2", "5"), (FK_DOUBLE, "2", "5"),
                       (FK_TS_MS, "2019-07-18T20:14:16", "2019-07-18T20:14:17")):
        for name, nl in (("nl", "\n"), ("crlf", "\r\n"), ("none", "")):
            out.append(case(f"last-field-{kind}-{name}", f"1 {a}{nl or chr(10)}2 {b}{nl}",
                            [(0, FK_LONG), (1, kind)]))
    # Empty lines are lines ("" splits to [""]): first, last, in runs; only newlines; a lone '\r'.
    one = [(0, FK_STR)]
    out.append(case("empty-runs", "\n\na b\n\n\n\nc\n\n", one))
    out.append(case("empty-only-newlines", "\n" * 5, one))
    out.append(case("empty-first-byte", "\nq\n", one))
    out.append(case("empty-last-cr", "a\nb\n\r", one))
    out.append(case("empty-last-crlf", "a\nb\n\r\n", one))
    out.append(case("empty-one-newline", "\n", one))
    # The same lines asked for field 1: the first empty line is ArrayIndexOutOfBounds.
    out.append(case("empty-runs-missing-field", "a b\n\nc d\n", [(1, FK_STR)]))
    # Separators only -> []; a requested empty field between separators is present, after the
    # last non-empty field it is not.
    out.append(case("seps-only", "1 2\n   \n3 4\n", [(0, FK_LONG)]))
    out.append(case("empty-field-str", "1  3\n4 x 6\n", [(0, FK_LONG), (1, FK_STR), (2, FK_LONG)]))
    out.append(case("empty-field-long", "1 2 3\n4  6\n", [(1, FK_LONG)]))
    out.append(case("empty-field-double", "1 2 3\n4  6\n", [(1, FK_DOUBLE)]))
    out.append(case("trailing-seps-dropped", "1 2\n3  \n", [(0, FK_LONG), (1, FK_STR)]))
    out.append(case("leading-sep", " 1 2\n 3 4\n", [(0, FK_STR), (1, FK_LONG), (2, FK_LONG)]))
    return out


# ---- line starts ----------------------------------------------------------------------------
# kFcTile = 4096 positions per workgroup, 16 bytes per thread: both sides of every boundary.
LINE_START_SIZES = (1, 15, 16, 17, 4095, 4096, 4097, 2 * 4096 + 5)
LINE_START_SHIFTS = (0, 1, 7, 15)  # address of the buffer modulo 16: both load paths


def line_start_bytes(n: int, seed: int = 0) -> bytes:
    """n bytes, about one in six a newline, with newlines at bytes 4095 and 4096 where they
    exist, and a newline as the last byte for even seeds."""
    rng = np.random.default_rng(1000 + n + seed)
    b = rng.integers(0x61, 0x67, n).astype(np.uint8)
    b[b == 0x61] = 0x0A
    for p in (4095, 4096):
        if p < n:
            b[p] = 0x0A
    b[-1] = 0x0A if seed % 2 == 0 else 0x62
    return b.tobytes()


# ---- LDS budgets ----------------------------------------------------------------------------
PARSE_TILE_BYTES = 24 * 1024   # kTileLdsBytes (csrc/line_tile.h)
INGEST_TILE_BYTES = 16 * 1024  # kIngestTileBytes (csrc/ingest_hip.hip)
FMT_TILE_BYTES = 32 * 1024     # kFmtLds (csrc/format_hip.hip)
SPEC_BUDGET = [(0, FK_LONG), (1, FK_STR), (2, FK_DOUBLE)]


def _padded_line(i: int, ts: int, nbytes: int) -> str:
    """A line of exactly nbytes bytes (newline included): ts, a filler key, a double."""
    head, tail = f"{ts} k{i % 9}", f" {i % 100}.5\n"
    fill = nbytes - len(head) - len(tail)
    assert fill >= 0
    return head + "x" * fill + tail


def exact_tile(total: int, n: int = 256, ts0: int = 5000) -> bytes:
    """n lines of `total` bytes in all, the final newline included."""
    base, extra = divmod(total, n)
    return "".join(_padded_line(i, ts0 + i, base + (1 if i < extra else 0)) for i in range(n)).encode()


def budget_case(budget: int, pad: int, over: int) -> Case:
    """One 256-line tile of budget - pad (+ over) bytes; the test places it pad bytes after a
    16-byte boundary, so bytes + pad is the budget exactly, or one more."""
    return case(f"tile{budget}-pad{pad}-over{over}", exact_tile(budget - pad + over), SPEC_BUDGET, ts_col=0)


def mixed_tiles_case(budget: int) -> Case:
    """Three tiles, the middle one too long for LDS; the largest timestamp is in the middle."""
    long_len = budget // 256 + 6
    lines = [_padded_line(i, 9000 - abs(i - 300), 24) for i in range(256)]
    lines += [_padded_line(i, 9000 - abs(i - 300), long_len) for i in range(256, 512)]
    lines += [_padded_line(i, 9000 - abs(i - 300), 24) for i in range(512, 600)]
    return case(f"tiles{budget}-mixed", "".join(lines), SPEC_BUDGET, ts_col=0)


def offset_tile_case(budget: int) -> Case:
    """Two tiles; the second starts at byte 6143 of the batch and holds budget - 8 bytes. Placed
    one byte after a 16-byte boundary it is aligned (pad 0) and fits LDS, although its offset in
    the batch alone (6143 mod 16 = 15) would say otherwise: pad comes from the address."""
    first = [_padded_line(i, 3000 + i, 24 if i else 23) for i in range(256)]
    second = exact_tile(budget - 8, ts0=4000).decode()
    return case(f"tiles{budget}-offset", "".join(first) + second, SPEC_BUDGET, ts_col=0)


def no_tile_fits_case(budget: int) -> Case:
    long_len = budget // 256 + 6
    lines = [_padded_line(i, 100 + i, long_len) for i in range(512)]
    lines[511] = lines[511][:-1] + "1234567890123456789\n"  # a host line in a global tile
    return case(f"tiles{budget}-none-fit", "".join(lines), SPEC_BUDGET, ts_col=0)


def long_line_case() -> Case:
    lines = [_padded_line(i, 100 - i, 20) for i in range(10)]
    lines[5] = _padded_line(5, 777, 30000)
    return case("one-30000-byte-line", "".join(lines), SPEC_BUDGET, ts_col=0)


def tiny_tile_case() -> Case:
    return case("tile-shorter-than-head", "7 8", [(0, FK_LONG), (1, FK_LONG)], ts_col=1)


# ---- numbers --------------------------------------------------------------------------------
def random_decimal_texts(n: int = 20000, seed: int = 11) -> list[str]:
    """Decimals of 1-15 digits, the point anywhere (".5" and "1." included), exponents in
    +-25: both sides of the fast path's |exp10| <= 22 bound."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        nd = int(rng.integers(1, 16))
        digits = "".join(str(int(d)) for d in rng.integers(0, 10, nd))
        p = int(rng.integers(0, nd + 2))
        t = digits if p > nd else digits[:p] + "." + digits[p:]
        if rng.integers(0, 2):
            t += "eE"[int(rng.integers(0, 2))] + ["", "+", "-"][int(rng.integers(0, 3))] + str(int(rng.integers(0, 26)))
        out.append(["", "-", "+"][int(rng.integers(0, 3))] + t)
    return out


DOUBLE_EDGES = [
    "1.", ".5", "+.5e-3", "-0.0", "0" * 21 + "1", "1e22", "1e23", "9007199254740993", "4.9e-324",
    "1.7976931348623157e308", "87.5d", "NaN", "-Infinity", "123456789012345e7", "123456789012345e8",
    "\t1.5", "1.5\t", "\t-2.25e1\t", "1E5", "1.5F", "+NaN", "-NaN", "+Infinity", "Infinity", "1e00005",
    "1e0022", "0.000000000000000000000001", "0.0000000000000000000001", "1e400", "1e-400", "-1e400",
    "000000000000000000000012.5e0", "999999999999999", "1000000000000000", "0.1", "0.30000000000000004",
    "2.2250738585072014e-308", "100000000000000.0", "1.50", "5e-324", "2.4703282292062328e-324", "0e99999",
]
DOUBLE_INVALID = [
    "", "abc", "1e", "1e+", ".", "+", "-", "1_0", "inf", "nan", "infinity", "Inf", "NAN", "1.5.2", "--1",
    "1e5e5", "１", " 1.5", "1d5", "NaNd", "Infinit", "Infinityf", "e5", ".e5", "1,5", "1.5dd", "d",
    "+-1", "1e1.5", "\t",
]
LONG_EDGES = [
    "9223372036854775807", "-9223372036854775808", "+5", "-0", "007", "0", "+9223372036854775807",
    "0" * 20 + "123", "-" + "0" * 22 + "9223372036854775808", "9223372036854775799", "-9223372036854775799",
    "922337203685477580", "-922337203685477581",
]
LONG_INVALID = [
    "9223372036854775808", "-9223372036854775809", "9223372036854775810", "-9223372036854775810",
    "92233720368547758070", "1e5", "", "+", "-", "5.0", "\t5", "5\t", "0x10", "５", "1_0", "+-5", "5L",
]
INT_EDGES = ["2147483647", "-2147483648", "+2147483647", "0" * 10 + "2147483647", "-0", "214748364"]
INT_INVALID = ["2147483648", "-2147483649", "2147483650", "-2147483650", "21474836470", "9223372036854775807"]


def _token_lines(tokens) -> str:
    """`i|token|z` per token: the trailing field keeps an empty token a present field."""
    return "".join(f"{i}|{t}|z\n" for i, t in enumerate(tokens))


def number_cases() -> list[Case]:
    out = [case("random-decimals", "".join(f"{i} {t}\n" for i, t in enumerate(random_decimal_texts())),
                [(0, FK_LONG), (1, FK_DOUBLE)], ts_col=0)]
    out.append(case("double-edges", _token_lines(DOUBLE_EDGES), [(0, FK_LONG), (1, FK_DOUBLE)], "|"))
    out.append(case("long-edges", _token_lines(LONG_EDGES), [(1, FK_LONG), (1, FK_RAW_LONG)], "|", ts_col=0))
    out.append(case("int-edges", _token_lines(INT_EDGES), [(1, FK_INT), (0, FK_INT)], "|", ts_col=0))
    return out


def invalid_number_tokens() -> list[tuple[int, str]]:
    return ([(FK_DOUBLE, t) for t in DOUBLE_INVALID] + [(FK_LONG, t) for t in LONG_INVALID]
            + [(FK_INT, t) for t in INT_INVALID])


# ---- dates ----------------------------------------------------------------------------------
H8, HM5 = 8 * 3600, -5 * 3600
_MDAYS = (31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31)


def valid_dates() -> list[str]:
    out = []
    for y in (2019, 2020):
        for m in range(12):
            last = _MDAYS[m] + (1 if m == 1 and y == 2020 else 0)
            out.append(f"{y}-{m + 1:02d}-{last:02d}T23:59:59")
            out.append(f"{y}-{m + 1:02d}-01T00:00")
    out += ["1900-02-28T12:00:00", "1900-03-01T00:00:00", "2000-02-29T12:00:00", "2000-03-01T00:00",
            "2100-02-28T23:59:59", "2100-03-01T00:00:00", "1600-01-01T00:00", "1600-02-29T00:00:01",
            "1969-12-31T23:59:59.999", "1969-12-31T23:59:59.250", "1970-01-01T00:00", "1970-01-01T00:00:00.001",
            "0001-01-01T00:00:00", "0100-03-01T00:00:00", "9999-12-31T23:59:59.999999999",
            "2038-01-19T03:14:07", "2038-01-19T03:14:08", "2038-01-19T11:14:07", "2038-01-19T11:14:08",
            "2038-01-18T22:14:07", "2038-01-18T22:14:08", "1901-12-13T20:45:52", "1901-12-13T20:45:51",
            "2106-02-07T06:28:16", "2019-07-18T20:14", "2019-07-18T00:00:00.000"]
    out += ["2019-07-18T20:14:16." + "123456789"[:k] for k in range(1, 10)]
    out += ["2019-07-18T20:14:16." + "000000001"[9 - k:] for k in range(1, 10)]
    return out


DATE_INVALID = [
    "2019-02-29T00:00:00", "1900-02-29T00:00:00", "2100-02-29T00:00:00", "2019-13-01T00:00:00",
    "2019-00-01T00:00:00", "2019-04-31T00:00:00", "2019-04-00T00:00:00", "2019-07-18T24:00:00",
    "2019-07-18T20:60:00", "2019-07-18T20:14:60", "2019-07-18T20:14:16.", "2019-07-18T20:14:16.1234567890",
    "2019-07-18 20:14:16", "2019-7-18T20:14:16", "2019-07-18T20:14:6", "2019-07-18T20:14:", "2019-07-18T20",
    "2019-07-18", "", "2019-07-18T20:14:16Z", "2019-07-18T20:14:16+08:00", "2019/07/18T20:14:16",
    "2019-07-18T20-14-16", "19-07-18T20:14:16", "2019-07-18T2O:14:16", "2019-07-18T20:14.5",
    "2019-06-31T00:00", "2020-02-30T00:00",
]
SPEC_DATES = [(1, FK_TS_INTSEC), (1, FK_TS_MS), (0, FK_LONG)]


def date_cases() -> list[Case]:
    lines = _token_lines(valid_dates())
    out = [case(f"dates-offset{off}", lines, SPEC_DATES, "|", off, ts_col=1) for off in (0, H8, HM5)]
    out.append(case("dates-iso-sec", lines, [(1, FK_ISO_SEC), (1, FK_TS_MS)], "|", H8, ts_col=0))
    return out


# ---- strings --------------------------------------------------------------------------------
SPEC_STRINGS = [(1, FK_STR), (2, FK_STR), (0, FK_LONG)]


def string_case() -> Case:
    """Empty, one byte, 2- / 3- / 4-byte UTF-8, an invalid byte; "b" is first seen in field 2 of
    line 0 and then in field 1 of line 2, "a" the other way round: ids follow (line, field)."""
    rows = [(b"a", b"b"), (b"c", b"a"), (b"b", b"c"), (b"", b"z"), ("é".encode(), "主".encode()),
            ("\U0001F600".encode(), "x\U00010000y".encode()), (b"\xff", b"a"), ("主".encode(), "é".encode()),
            (b"q", b"\x80q"), ("主机-1".encode(), b"A"), (b"\x7f", "\U0010FFFF".encode()),
            ("\u07ff\u0800\uffff".encode(), b"a")]
    data = b"".join(str(i).encode() + b" " + a + b" " + b + b" t\n" for i, (a, b) in enumerate(rows))
    return case("strings", data, SPEC_STRINGS, ts_col=2)


def growth_batches() -> list[Case]:
    """300 distinct strings through a dictionary created with cap=8, id_cap=4, arena_cap=16:
    three batches that each force growth and a rehash, then the first again (no new ids)."""
    names = [f"host-{i:03d}-{'x' * (i % 17)}" for i in range(300)]
    out = []
    for b, (lo, hi) in enumerate([(0, 40), (20, 150), (100, 300), (0, 40)]):
        lines = [f"{i} {names[lo + (i * 7) % (hi - lo)]} {names[lo + (i * 3) % (hi - lo)]} t" for i in range(hi - lo + 30)]
        out.append(case(f"growth-{b}", "\n".join(lines) + "\n", SPEC_STRINGS, ts_col=2))
    return out


# ---- formatting -----------------------------------------------------------------------------
FMT_ROWS = (1, 255, 256, 257, 513)
FMT_DOUBLE_EDGES = [0.0, -0.0, 0.001, 9999999.5, 1.0, -1.5, 91.5, 0.999, 1234567.125, -0.001]
FMT_LONG_EDGES = [M.I64_MIN, M.I64_MAX, 0, -1, 1, 10, -10, 99, 100, M.I32_MIN, M.I32_MAX]


def fmt_decimals(rng, n: int) -> np.ndarray:
    """The `_decimals` family of tests/test_row_format.py: short decimals in plain notation."""
    ip = rng.integers(0, 10_000_000, n)
    fd = rng.integers(0, 7, n)
    frac = rng.integers(0, 10 ** 6, n) // 10 ** (6 - fd)
    txt = [f"{'-' if s else ''}{i}.{str(f).zfill(d) if d else '0'}"
           for s, i, f, d in zip(rng.integers(0, 2, n), ip, frac, fd)]
    v = np.array([float(t) for t in txt])
    v[~((np.abs(v) >= 1e-3) & (np.abs(v) < 1e7) | (v == 0))] = 0.5
    v[:min(n, len(FMT_DOUBLE_EDGES))] = FMT_DOUBLE_EDGES[:n]
    return v


def fmt_names() -> list[bytes]:
    """Dictionary strings for the row formatter: short ones, and one of every length 100..140
    (a 256-row tile of ~130-byte rows is what reaches the 32 KB LDS budget)."""
    short = [f"10.8.{i}.{i % 7}".encode() for i in range(40)] + [b"", "主机".encode()]
    return short + [(f"L{n}-".encode() + b"y" * n)[:n] for n in range(100, 141)]


def fmt_exact_tile_ids(total: int, names: list[bytes], overhead: int, n: int = 256) -> list[int]:
    """String ids of n rows whose lengths (string + overhead bytes each) sum to `total`."""
    by_len = {len(b): i for i, b in enumerate(names) if len(b) >= 100}
    base, extra = divmod(total, n)
    return [by_len[base - overhead + (1 if i < extra else 0)] for i in range(n)]


def fmt_columns(n: int, seed: int):
    """(short-name ids, longs, doubles, subtasks) of n rows; the edge values come first."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, 42, n).astype(np.int32)  # the short names
    lv = rng.integers(-(1 << 62), 1 << 62, n)
    lv[:min(n, len(FMT_LONG_EDGES))] = FMT_LONG_EDGES[:n]
    dv = fmt_decimals(rng, n)
    sub = rng.integers(0, 3, n).astype(np.int32)
    return ids, lv, dv, sub


# ---- the lists the two test modules run -----------------------------------------------------------
def parse_cases() -> list[Case]:
    return geometry_cases() + number_cases() + date_cases() + [string_case()]


def budget_cases(budget: int) -> list[tuple[Case, int]]:
    """(case, pad): the batch goes pad bytes after a 16-byte boundary."""
    out = [(budget_case(budget, pad, over), pad) for pad in (0, 1, 15) for over in (0, 1)]
    out += [(mixed_tiles_case(budget), pad) for pad in (0, 7)]
    out += [(no_tile_fits_case(budget), 0), (long_line_case(), 3), (offset_tile_case(budget), 1)]
    out += [(tiny_tile_case(), pad) for pad in (0, 1, 15)]
    return out


def invalid_cases() -> list[Case]:
    """valid, invalid, valid: the error belongs to line 1 and has the model's class."""
    good = {FK_DOUBLE: "1.5", FK_LONG: "15", FK_INT: "15"}
    tokens = invalid_number_tokens() + [(k, t) for t in DATE_INVALID for k in (FK_TS_MS, FK_TS_INTSEC)]
    return [case(f"invalid-{k}-{t!r}", "0|{0}|z\n1|{1}|z\n2|{0}|z\n".format(good.get(k, "2019-07-18T20:14:16"), t),
                 [(0, FK_LONG), (1, k)], "|", H8) for k, t in tokens]


def all_invalid_in_one() -> list[Case]:
    """Every invalid token of a kind in one batch, valid lines in between (raw kernel status)."""
    out = []
    for kind, good in ((FK_DOUBLE, "2.5"), (FK_LONG, "15"), (FK_INT, "15"), (FK_TS_MS, "2019-07-18T20:14:16")):
        toks = [t for k, t in invalid_number_tokens() if k == kind] if kind != FK_TS_MS else DATE_INVALID
        lines = [x for t in toks for x in (good, t)]
        out.append(case(f"all-invalid-{kind}", _token_lines(lines), [(0, FK_LONG), (1, kind)], "|", H8, ts_col=0))
    return out
