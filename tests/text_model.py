"""A plain model of the text path: what the line-start, parse, ingest, dictionary and row-format
kernels (csrc/kernels_hip.hip line_starts, csrc/parse_hip.hip, csrc/ingest_hip.hip,
csrc/format_hip.hip), their C++ twins and the host parser (csrc/runtime.cpp) must compute.

Pure Python: integers, ``float`` and the standard library only, nothing native and nothing of
the project's but ``mxstream/utils/javafmt.py`` (itself pure Python). It states the semantics of
the reference jobs' Java calls, not the project's code:

* ``String.split(sep)`` with a one-character, non-regex separator: every occurrence splits,
  trailing empty strings are removed, no match returns the input itself (``"".split(x) == [""]``).
* ``Double.parseDouble``: ``trim()`` (characters <= ' '), then the decimal grammar
  ``[+-]?(digits.?digits*|.digits)([eE][+-]?digits)?[dDfF]?`` or ``[+-]?(NaN|Infinity)``, ASCII
  digits only; the value is the correctly rounded double, which ``float(str)`` is too. ``NaN`` is
  the canonical NaN whatever its sign. Java also accepts hexadecimal literals
  (``0x1.8p1``); the model does not, and the cases keep them out: they are outside every fast
  path and the host's handling of them is not under test here.
* ``Long.parseLong`` / ``Integer.parseInt``: ``[+-]?[0-9]+``, then the range. (Java also takes
  non-ASCII decimal digits; the cases keep them out.)
* ``LocalDateTime.parse`` (ISO_LOCAL_DATE_TIME, strict resolver): ``yyyy-MM-ddTHH:mm[:ss[.f{1,9}]]``
  with a four-digit year (the cases keep signed / longer years, year 0000 and a lower-case 't',
  which Java's case-insensitive formatter takes, out); the date must
  exist (29 February only in leap years), hour <= 23, minute and second <= 59.
  ``toEpochSecond(offset)`` is the local epoch second minus the offset. The epoch day comes from
  ``datetime.date.toordinal()``.
* ``String.hashCode`` over UTF-16 code units; text arrives as UTF-8, an invalid byte decodes to
  U+FFFD (the cases use single invalid bytes only, where every decoder agrees on the count).
* ``Tuple.toString`` / ``Double.toString`` / ``Long.toString`` rows of print().

Line cutting is SocketTextStreamFunction's: lines end at '\\n', a trailing '\\r' is dropped, a
final '\\n' starts no line, an empty line is a line.
"""
from __future__ import annotations

import datetime
import re
import struct

from mxstream.utils.javafmt import java_double_str

FK_STR, FK_DOUBLE, FK_LONG, FK_TS_INTSEC, FK_TS_MS, FK_INT, FK_RAW_LONG, FK_ISO_SEC = range(8)

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
_M64 = (1 << 64) - 1

NFE = "NumberFormatException"
AIOOBE = "ArrayIndexOutOfBoundsException"
DTPE = "DateTimeParseException"


class JavaError(Exception):
    """The Java exception a parse raises; ``kind`` is its class name."""

    def __init__(self, kind: str, what: str = ""):
        super().__init__(f"{kind}: {what}")
        self.kind = kind


# ---- lines ----------------------------------------------------------------------------------
def line_starts(data: bytes) -> list[int]:
    return [i for i in range(len(data)) if i == 0 or data[i - 1] == 0x0A]


def split_lines(data: bytes) -> list[bytes]:
    """The lines of a batch as the parsers see them ('\\n' and one trailing '\\r' removed)."""
    if not data:
        return []
    lines = data.split(b"\n")
    if data.endswith(b"\n"):
        lines.pop()  # a final newline starts no line
    return [l[:-1] if l.endswith(b"\r") else l for l in lines]


def java_split(line, sep):
    if len(sep) != 1:
        raise ValueError("one-character separator")
    parts = line.split(sep)  # "" -> [""]: no match, the array holds the input
    if len(line) == 0:
        return parts
    while parts and len(parts[-1]) == 0:
        parts.pop()
    return parts


# ---- numbers --------------------------------------------------------------------------------
_DEC = re.compile(r"([+-]?)(?:([0-9]+)\.?([0-9]*)|\.([0-9]+))(?:[eE]([+-]?)([0-9]+))?([dDfF]?)")
_SPECIAL = re.compile(r"([+-]?)(NaN|Infinity)")


def java_trim(s: str) -> str:
    a, b = 0, len(s)
    while a < b and s[a] <= " ":
        a += 1
    while b > a and s[b - 1] <= " ":
        b -= 1
    return s[a:b]


def parse_double(s: str) -> float:
    t = java_trim(s)
    m = _DEC.fullmatch(t)
    if m:
        return float(t[:-1] if m.group(7) else t)
    m = _SPECIAL.fullmatch(t)
    if m:
        if m.group(2) == "NaN":
            return float("nan")
        return float("-inf") if m.group(1) == "-" else float("inf")
    raise JavaError(NFE, f'For input string: "{s}"')


def f64_bits(x: float) -> int:
    """The double's bit pattern as a signed 64-bit word (how the columns hold it)."""
    if x != x:
        return 0x7FF8000000000000  # Java's canonical NaN
    return struct.unpack("<q", struct.pack("<d", x))[0]


_LONG = re.compile(r"[+-]?[0-9]+")


def parse_long(s: str, lo: int = I64_MIN, hi: int = I64_MAX) -> int:
    if not _LONG.fullmatch(s):
        raise JavaError(NFE, f'For input string: "{s}"')
    v = int(s)
    if not lo <= v <= hi:
        raise JavaError(NFE, f'out of range: "{s}"')
    return v


_ISO = re.compile(r"([0-9]{4})-([0-9]{2})-([0-9]{2})T([0-9]{2}):([0-9]{2})"
                  r"(?::([0-9]{2})(?:\.([0-9]{1,9}))?)?")


def wrap_i32(v: int) -> int:
    """Java's (int) cast of a long."""
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >= 1 << 31 else v


def parse_iso(s: str, offset_s: int = 0) -> tuple[int, int, int]:
    """(FK_TS_MS, FK_TS_INTSEC, FK_ISO_SEC) values of LocalDateTime.parse(s) at the offset:
    exact epoch milliseconds; ``(int) epochSecond * 1000L``; ``(int) epochSecond``."""
    m = _ISO.fullmatch(s)
    if not m:
        raise JavaError(DTPE, f"Text '{s}' could not be parsed")
    y, mo, d, h, mi = (int(m.group(k)) for k in range(1, 6))
    sec = int(m.group(6) or 0)
    frac = m.group(7) or ""
    try:
        dt = datetime.datetime(y, mo, d, h, mi, sec)
    except ValueError:
        raise JavaError(DTPE, f"Text '{s}' could not be parsed") from None
    es = (dt.date().toordinal() - 719163) * 86400 + h * 3600 + mi * 60 + sec - offset_s
    ms = int((frac + "000")[:3])
    return es * 1000 + ms, wrap_i32(es) * 1000, wrap_i32(es)


# ---- strings --------------------------------------------------------------------------------
def utf8_to_java(b: bytes) -> str:
    return b.decode("utf-8", errors="replace")


def java_hash(s) -> int:
    """String.hashCode as a signed 32-bit int; ``s`` is a str, or UTF-8 bytes."""
    if isinstance(s, (bytes, bytearray)):
        s = utf8_to_java(bytes(s))
    u = s.encode("utf-16-be", errors="surrogatepass")
    h = 0
    for k in range(0, len(u), 2):
        h = (31 * h + ((u[k] << 8) | u[k + 1])) & 0xFFFFFFFF
    return h - (1 << 32) if h >= 1 << 31 else h


def fnv1a64(b: bytes) -> int:
    """The parse_text key of a string field: 64-bit FNV-1a of its bytes as a signed word, with
    -1 and -2 (the hash tables' reserved keys) moved down by two."""
    h = 0xCBF29CE484222325
    for c in b:
        h = ((h ^ c) * 0x100000001B3) & _M64
    if h >= _M64 - 1:
        h -= 2
    return h - (1 << 64) if h >= 1 << 63 else h


def assign_ids(rows: list[list[bytes]], known: dict | None = None) -> tuple[list[list[int]], dict]:
    """Dictionary ids of the string fields of every line (``rows[line][string field]``), in
    first-appearance order over (line, field), continuing ``known`` (bytes -> id)."""
    known = {} if known is None else known
    out = []
    for row in rows:
        ids = []
        for s in row:
            if s not in known:
                known[s] = len(known)
            ids.append(known[s])
        out.append(ids)
    return out, known


# ---- one line -------------------------------------------------------------------------------
def parse_field(field: bytes, kind: int, offset_s: int = 0):
    """The column value of one field: bytes for a string, else the int64 column word."""
    if kind == FK_STR:
        return field
    s = field.decode("latin-1")  # one char per byte: nothing non-ASCII is a digit or <= ' '
    if kind == FK_DOUBLE:
        return f64_bits(parse_double(s))
    if kind in (FK_LONG, FK_RAW_LONG):
        return parse_long(s)
    if kind == FK_INT:
        return parse_long(s, I32_MIN, I32_MAX)
    ms, intsec, isosec = parse_iso(s, offset_s)
    return {FK_TS_MS: ms, FK_TS_INTSEC: intsec, FK_ISO_SEC: isosec}[kind]


def parse_line(line: bytes, spec, sep: str = " ", offset_s: int = 0) -> list:
    """Values of the spec's fields, in spec order; raises the first field's JavaError."""
    parts = java_split(line, sep.encode())
    out = []
    for fi, kind in spec:
        if fi >= len(parts):
            raise JavaError(AIOOBE, str(fi))
        out.append(parse_field(parts[fi], kind, offset_s))
    return out


def parse_batch(data: bytes, spec, sep: str = " ", offset_s: int = 0) -> list:
    """Per line: the list of values, or the JavaError instance."""
    out = []
    for line in split_lines(data):
        try:
            out.append(parse_line(line, spec, sep, offset_s))
        except JavaError as e:
            out.append(e)
    return out


# ---- the kernels' fast-path contract ----------------------------------------------------------
def needs_host(field: bytes, kind: int, in_parse_text: bool, offset_s: int = 0) -> bool:
    """May the kernel hand this field's line to the host parser (status 1)? The contract of the
    headers of csrc/parse_hip.hip and csrc/ingest.h: every other line must get status 0."""
    try:
        parse_field(field, kind, offset_s)
    except JavaError:
        return True
    if kind == FK_STR:
        return in_parse_text and any(c >= 0x80 for c in field)
    if kind != FK_DOUBLE:
        return False
    m = _DEC.fullmatch(java_trim(field.decode("latin-1")))
    if not m or m.group(7):
        return True  # NaN, Infinity, a d/f suffix
    ip, fp = (m.group(2) or ""), (m.group(3) if m.group(2) is not None else m.group(4)) or ""
    sig = len((ip + fp).lstrip("0"))  # leading zeros do not count, trailing zeros do
    edigits = m.group(6) or ""
    if sig > 15 or len(edigits) > 4:
        return True
    e = int((m.group(5) or "") + edigits) if edigits else 0
    return not -22 <= e - len(fp) <= 22


def line_needs_host(line: bytes, spec, sep: str, in_parse_text: bool, offset_s: int = 0) -> bool:
    parts = java_split(line, sep.encode())
    return any(fi >= len(parts) or needs_host(parts[fi], kind, in_parse_text, offset_s)
               for fi, kind in spec)


# ---- print() rows ---------------------------------------------------------------------------
def format_row(values, kinds, prefix: str = "", as_tuple: bool = True) -> bytes:
    """One printed row, newline included. values: bytes (string), float (double) or int."""
    cells = []
    for v, k in zip(values, kinds):
        if k == FK_STR:
            cells.append(bytes(v))
        elif k == FK_DOUBLE:
            cells.append(java_double_str(float(v)).encode())
        else:
            cells.append(str(int(v)).encode())
    body = b"(" + b",".join(cells) + b")" if as_tuple else cells[0]
    return prefix.encode() + body + b"\n"
