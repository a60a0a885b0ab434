r"""Payload routes: an ordered client list of (name, regex) pairs decides which consumer a
decoded telegram concerns, as FHEM's dispatch does behind its equal-message drop.

A :class:`RouteTable` compiles the list with ``regex_dfa.compile_bank_dfas`` into one search DFA per route
over a shared byte-class alphabet and writes the blob the device walks (``sdx_route_lines``; the layout is
``csrc/sdx_route_layout.h``, the constants below mirror it).  For a payload: ``mask`` has bit r set iff
``re.search(pattern_r, payload)`` finds a match, ``route`` is the lowest set bit or -1.  A payload is
matched as its latin-1 text (``re`` on ``str``: ``\w`` and ``\s`` are the Unicode sets on code points
0..255, as regex_dfa writes them out); a payload holds no newline, so ``$`` as regex_dfa compiles it and
Python's agree.  :meth:`RouteTable.match` is the host restatement: it walks the same compiled tables, read back
out of the blob."""
from __future__ import annotations

import struct
from typing import Iterable, List, Sequence, Tuple, Union

from . import regex_dfa

MAGIC = 0x54525853        # SDX_ROUTE_MAGIC "SXRT"
VERSION = 1               # SDX_ROUTE_VERSION
ROUTES_MAX = 64           # SDX_ROUTE_MAX
STATES_MAX = 4096         # SDX_ROUTE_STATES_MAX
BLOB_MAX = 1 << 20        # SDX_ROUTE_BLOB_MAX
HDR_FMT = "<8I"           # sdx_route_hdr: magic, version, n_routes, n_class, trans_width, total_bytes, res[2]
DFA_FMT = "<4I"           # sdx_route_dfa: n_states, start, flags_off, trans_off
CLS_OFF = struct.calcsize(HDR_FMT)
DFA_OFF = CLS_OFF + 256

# A client list for this bank's preambles, on the model of FHEM's: P<id>#, W<id>#, u<id># in front of hex
# digits, and the bare letters of the older modules (i, s, TX, Ys, K, r, T, E, ...).  The first match wins.
# This project's data; its correctness criterion is Python's ``re``.
DEFAULT_ROUTES: List[Tuple[str, str]] = [
    ("IT", r"^i[A-Fa-f0-9]{6}"),
    ("IT_V3", r"^ih[A-Fa-f0-9]{8,}"),
    ("CUL_TCM97001", r"^s[A-Fa-f0-9]+"),
    ("SD_RSL", r"^P1#[A-Fa-f0-9]{8}"),
    ("SD_AS", r"^P2#[A-Fa-f0-9]{7,8}"),
    ("SD_WS07", r"^P7#[A-Fa-f0-9]{6}[AFaf][A-Fa-f0-9]{2,3}"),
    ("SD_WS09", r"^P9#F[A-Fa-f0-9]+"),
    ("Hideki", r"^P12#75[A-F0-9]{17,30}"),
    ("FLAMINGO", r"^P13\.?1?#[A-Fa-f0-9]+"),
    ("Dooya", r"^P16#[A-Fa-f0-9]+"),
    ("SD_WS_Maverick", r"^P47#[569A]{12}.*"),
    ("SD_GT", r"^P49#[A-Fa-f0-9]+"),
    ("FS10", r"^P61#[A-F0-9]+"),
    ("Siro", r"^P72#[A-Fa-f0-9]+"),
    ("SD_Keeloq", r"^P(?:87|88)#.*"),
    ("SD_Rojaflex", r"^P109#[A-Fa-f0-9]+"),
    ("SD_BELL", r"^P(?:15|32|41|42|57|79|96|98|112)#.*"),
    ("SD_UT", r"^P(?:14|20|24|26|29|30|34|46|56|68|69|76|78|81|83|86|90|91|91\.1|92|93|95|97|99|104|105|114|118|121"
              r"|127|128|130|132)#.*"),
    ("SD_WS", r"^W\d+x{0,1}#.*"),
    ("CUL_TX", r"^TX..........."),
    ("SOMFY", r"^Ys[0-9A-F]+"),
    ("CUL_WS", r"^K[A-Fa-f0-9]{5,}"),
    ("Revolt", r"^r[A-Fa-f0-9]{22}"),
    ("FHT80TF", r"^T[A-F0-9]{8}"),
    ("CUL_EM", r"^E0[1-3][A-Fa-f0-9]{16}"),
    ("FS20", r"^81..(?:04|0c)..0101a001"),
    ("FHT", r"^81..(?:04|09|0d)..(?:0101a001|0909a001)"),
    ("HMS", r"^h[A-Fa-f0-9]{12}"),
    ("IFB", r"^J............"),
    ("KOPP_FC", r"^kr\w{18,}"),
    ("LaCrosse", r"^\S+\s+9 "),
    ("PCA301", r"^\S+\s+24"),
    ("WMBUS", r"^b.*"),
    ("OREGON", r"^(?:3[8-9A-F]|[4-6][0-9A-F]|7[0-8]).*"),
]


def _payload_bytes(payload: Union[str, bytes, bytearray, memoryview]) -> bytes:
    return payload.encode("latin-1") if isinstance(payload, str) else bytes(payload)


class RouteTable:
    """An ordered list of up to 64 (name, pattern) pairs, compiled.  ``names``, ``patterns``, ``blob``
    (what sdx_route_table_create takes), ``match``.  A pattern outside regex_dfa's syntax raises
    NotImplementedError, as for the bank; more than 64 routes, a DFA of more than 4096 states or a blob
    over 1 MiB raise ValueError (the latter two naming the pattern)."""

    def __init__(self, pairs: Iterable[Tuple[str, str]]):
        pairs = [(str(n), p) for n, p in pairs]
        if not 1 <= len(pairs) <= ROUTES_MAX:
            raise ValueError(f"a route table holds 1 to {ROUTES_MAX} routes, not {len(pairs)}")
        for _, p in pairs:
            if not isinstance(p, str):
                raise TypeError(f"route pattern {p!r}: a str")
        self.names: List[str] = [n for n, _ in pairs]
        self.patterns: List[str] = [p for _, p in pairs]
        cls_of, n_class, dfas = regex_dfa.compile_bank_dfas(self.patterns, max_states=STATES_MAX)
        width = 1 if all(d[0] <= 256 for d in dfas) else 2
        recs, tables = [], bytearray()
        at = DFA_OFF + struct.calcsize(DFA_FMT) * len(dfas)

        def pad4():
            tables.extend(b"\0" * (-len(tables) % 4))
        for pat, (ns, start, trans, flags) in zip(self.patterns, dfas):
            pad4()
            f_off = at + len(tables)
            tables.extend(bytes(flags))
            pad4()
            t_off = at + len(tables)
            cells = [x for row in trans for x in row]
            tables.extend(bytes(cells) if width == 1 else struct.pack(f"<{len(cells)}H", *cells))
            recs.append(struct.pack(DFA_FMT, ns, start, f_off, t_off))
            if at + len(tables) > BLOB_MAX:
                raise ValueError(f"route pattern {pat!r}: the table's blob exceeds {BLOB_MAX} bytes")
        pad4()
        total = at + len(tables)
        if total > BLOB_MAX:
            raise ValueError(f"route pattern {self.patterns[-1]!r}: the table's blob exceeds {BLOB_MAX} bytes")
        self.blob: bytes = (struct.pack(HDR_FMT, MAGIC, VERSION, len(dfas), n_class, width, total, 0, 0) + bytes(cls_of) +
                            b"".join(recs) + bytes(tables))
        assert len(self.blob) == total
        self._walk = _read_blob(self.blob)

    def __len__(self) -> int:
        return len(self.names)

    def match(self, payload: Union[str, bytes]) -> Tuple[int, int]:
        """(route, mask) of a payload: the walk of sdx_route_lines' kernel over the blob's tables."""
        data = _payload_bytes(payload)
        cls_of, n_class, dfas = self._walk
        cl = [cls_of[b] for b in data]
        mask = 0
        for r, (start, flags, trans) in enumerate(dfas):
            st, i, n = start, 0, len(cl)
            f = flags[st]
            while not f & (regex_dfa.ACC_NOW | regex_dfa.DEAD) and i < n:
                st = trans[st * n_class + cl[i]]
                f = flags[st]
                i += 1
            if f & regex_dfa.ACC_NOW or (i == n and f & regex_dfa.ACC_END):
                mask |= 1 << r
        return ((mask & -mask).bit_length() - 1 if mask else -1), mask

    def pick(self, payloads: Sequence[Union[str, bytes]]) -> Tuple[int, int, int]:
        """(pick, route, mask) of a line's payloads in the reference's list order: pick = the
        index of the first payload some route matches, route and mask that payload's; (0, -1, 0) when none
        matches or the list is empty.  The host restatement of sdx_route_records."""
        for i, payload in enumerate(payloads):
            route, mask = self.match(payload)
            if route >= 0:
                return i, route, mask
        return 0, -1, 0

    def name_of(self, route: int):
        """The route's name, None for -1."""
        return self.names[route] if route >= 0 else None


def _read_blob(blob: bytes):
    """-> (cls_of, n_class, [(start, flags, trans)]) read back out of a blob this module wrote."""
    magic, version, n_routes, n_class, width, total, _, _ = struct.unpack_from(HDR_FMT, blob, 0)
    assert magic == MAGIC and version == VERSION and total == len(blob)
    cls_of = blob[CLS_OFF: CLS_OFF + 256]
    dfas = []
    for r in range(n_routes):
        ns, start, f_off, t_off = struct.unpack_from(DFA_FMT, blob, DFA_OFF + 16 * r)
        cells = ns * n_class
        trans = blob[t_off: t_off + cells] if width == 1 else struct.unpack_from(f"<{cells}H", blob, t_off)
        dfas.append((start, blob[f_off: f_off + ns], trans))
    return cls_of, n_class, dfas


def as_table(routes: Union["RouteTable", Sequence[Tuple[str, str]], None]):
    """A RouteTable from what the front end's ``routes`` arguments accept: a table, a list of pairs, None."""
    if routes is None or isinstance(routes, RouteTable):
        return routes
    return RouteTable(routes)
