"""route_match="any" without a GPU: RouteTable.pick against the definition over the recorded
message lists of the line goldens, the exports, the argument checks and the controller's topics.

The definition, restated in ``restate_pick``: pick = the index of the line's first message, in the reference's
list order, whose payload some route matches by ``re.search``; 0 when none does; route and mask are that
message's.  Its inputs are the reference-recorded ``e2e`` lists, never anything the code under test made."""
import asyncio
import json
import os
import re

import pytest

from pysignalduino_amd import routes, runtime
from pysignalduino_amd.controller import BatchingParserTask

import test_controller as C
import test_routes_host as RH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OVERLAP = [("hideki", r"75[A-F0-9]{6,}"), ("tail", r"[A-F]{4}00$"), ("ff", r"^P\d+#(?:..)*FF"), ("empty", r"^$"),
           ("p7", r"^P7#[A-F0-9]{6}$"), ("any_p", r"^P"), ("w", r"^W\d+x{0,1}#.*")]


def restate_pick(patterns, payloads):
    """(pick, route, mask) of a line's payloads (str) by the definition."""
    for i, s in enumerate(payloads):
        mask = sum(1 << r for r, p in enumerate(patterns) if re.search(p, s))
        if mask:
            return i, (mask & -mask).bit_length() - 1, mask
    return 0, -1, 0


@pytest.mark.parametrize("name", ["lines_golden.json.gz", "lines_float_golden.json.gz", "lines_general_golden.json.gz"])
@pytest.mark.parametrize("pairs", [routes.DEFAULT_ROUTES, OVERLAP], ids=["default", "overlap"])
def test_pick_equals_the_definition_on_the_goldens(golden, name, pairs):
    table = routes.RouteTable(pairs)
    lists = [[m[1] for m in c.get("e2e", [])] for c in golden(name)]
    memo = {}

    def exp(p):
        k = tuple(p)
        if k not in memo:
            memo[k] = restate_pick(table.patterns, p)
        return memo[k]
    bad = [(p[:4], table.pick(p), exp(p)) for p in lists if table.pick(p) != exp(p)]
    assert not bad, (len(bad), bad[:3])
    assert table.pick([]) == (0, -1, 0)
    bearing = [p for p in lists if p]
    assert len(bearing) > 50 and max(map(len, bearing)) >= 4
    if name == "lines_golden.json.gz" and pairs is routes.DEFAULT_ROUTES:
        # the corpus' figures: result-bearing, several messages, the longest list, unrouted by the
        # first message, and of those the lines a later message routes
        first = [table.match(p[0])[0] for p in bearing]
        picks = [table.pick(p) for p in bearing]
        assert (len(bearing), sum(len(p) > 1 for p in bearing), max(map(len, bearing))) == (1267, 536, 8)
        assert sum(r < 0 for r in first) == 186
        assert sum(pk > 0 for pk, _, _ in picks) == 67
        assert all(pk == 0 for (pk, _, _), r in zip(picks, first) if r >= 0)     # a routed first message stays
        ex = ["u40#C1DF2F0E98", "P72#7077CBC3A6", "P61#8F88343C58", "P1#7077CBC3A6"]
        assert [table.name_of(table.match(p)[0]) for p in ex] == [None, "Siro", "FS10", "SD_RSL"]
        assert table.pick(ex)[:2] == (1, table.names.index("Siro"))


def test_pick_is_bytes_or_str_and_carries_the_mask():
    table = routes.RouteTable(OVERLAP)
    assert table.pick(["zz", b"P7#ABCDEF", "W1#x"]) == (1,) + table.match("P7#ABCDEF")
    assert bin(table.pick(["zz", "P7#75ABCDEF00FF"])[2]).count("1") >= 3
    assert table.pick(["zz", "yy"]) == (0, -1, 0)
    assert table.pick([""]) == (0, 3, 8)          # ^$ takes an empty payload


def test_abi_declares_the_record_entries():
    hdr = open(os.path.join(ROOT, "include", "sdx.h")).read()
    for name in ("sdx_route_records", "sdx_route_skip"):
        assert name in runtime.EXPORTED and re.search(r"\b%s\(" % name, hdr), name
    assert "#define SDX_ABI_VERSION 14" in hdr and runtime.ABI_VERSION == 14     # only new entries: the version stays
    lib = runtime.load_library()
    assert lib.sdx_abi_version() == 14
    assert lib.sdx_route_records.argtypes is not None and lib.sdx_route_skip.argtypes is not None
    # no GPU is touched by a refused call: null table / null route_dev
    assert lib.sdx_route_records(None, None, None, 0, 0, None, None, None, None, None) == -1
    assert lib.sdx_route_skip(None, 0, 0, None, None, 0, None, None) == -1


def test_route_match_argument_errors():
    from pysignalduino_amd.frontend import SignalParser
    from pysignalduino_amd.stream import LineStream
    sp = SignalParser()
    with pytest.raises(ValueError, match="route_match"):
        sp.parse_lines_routed(["x"], routes.DEFAULT_ROUTES, route_match="last")
    with pytest.raises(ValueError, match="route_match"):
        sp.stream(routes=routes.DEFAULT_ROUTES, route_match="all")
    with pytest.raises(ValueError, match="needs routes"):
        sp.stream(route_match="any")
    with pytest.raises(ValueError, match="needs routes"):
        sp.parse_lines_routed(["x"], None, route_match="any")
    with pytest.raises(ValueError, match="needs routes"):
        LineStream(sp, route_match="any")
    ctl = C.Ctl(RH.RoutedParser(), callback=False)
    with pytest.raises(ValueError, match="route_match"):
        BatchingParserTask(ctl, publish="json", routes=RH.TABLE, route_match="each")
    with pytest.raises(ValueError, match="needs routes"):
        BatchingParserTask(ctl, publish="json", route_match="any")
    assert BatchingParserTask(ctl, publish="json", routes=RH.TABLE, route_match="any").route_match == "any"
    assert BatchingParserTask(ctl, publish="json", routes=RH.TABLE).route_match == "first"


# ---- controller: a picked telegram goes to its client's topic ------------------------------------------
PICK_TABLE = [("second", r"^1:M[SC];"), ("third", r"^2:"), ("mu0", r"^0:MU;D=\d*[05];$")]


def payloads_of(dec):
    """The scripted parser's message j of a line carries the payload '<j>:<line>'."""
    return [f"{j}:{ln}" for ln, j in dec]


class PickingParser(RH.RoutedParser):
    """test_routes_host.py's scripted parser with route_match: a line's messages are parse_line's list."""

    def __init__(self):
        super().__init__()
        self.matches = []

    def parse_lines_routed(self, lines, table, drop_unrouted=False, route_match="first"):
        self.matches.append(route_match)
        out = []
        for r in self.parse_lines(lines):
            if isinstance(r, Exception) or not r:
                out.append(r if isinstance(r, Exception) else None)
                continue
            pays = payloads_of(r)
            pk, rt, _ = table.pick(pays) if route_match == "any" else (0,) + table.match(pays[0])
            out.append(None if drop_unrouted and rt < 0 else (rt, json.dumps(r[pk])))
        return out

    def stream(self, chunk_lines, output="json", lag=3, routes=None, drop_unrouted=False, route_match="first"):
        assert output == "json"
        s = RH.RoutedStream(self, lag, routes, drop_unrouted)
        s.submit = lambda lines: _submit(s, lines, route_match)
        return s


def _submit(s, lines, route_match):
    s.q.append(RH._RoutedChunk(s.parser.parse_lines_routed(lines, s.table, s.drop, route_match=route_match), s.submitted))
    s.submitted += 1
    return s.submitted - 1


@pytest.mark.parametrize("stream", [True, False])
@pytest.mark.parametrize("drop", [False, True])
def test_controller_publishes_the_picked_telegram_to_its_topic(stream, drop):
    lines = ([f"MS;P0={i};" for i in range(150)] + ["boom", ""] + [f"MC;D={i};" for i in range(100)] +
             [f"MU;D={i};" for i in range(100)])
    table = routes.RouteTable(PICK_TABLE)
    exp, exp_first = [], []
    for ln in lines:
        if not ln or "boom" in ln:
            continue
        dec = C.FakeParser().parse_line(ln)
        if not dec:
            continue
        pk, rt, _ = restate_pick(table.patterns, payloads_of(dec))
        if not (drop and rt < 0):
            exp.append(("t/v1/state/messages" + ("/" + table.names[rt] if rt >= 0 else ""), json.dumps(dec[pk])))
        r0 = restate_pick(table.patterns, payloads_of(dec)[:1])[1]
        if not (drop and r0 < 0):
            exp_first.append(("t/v1/state/messages" + ("/" + table.names[r0] if r0 >= 0 else ""), json.dumps(dec[0])))
    picked_later = [e for e in exp if e[0].endswith("/second")]
    assert len(picked_later) > 50 and all(json.loads(t)[1] == 1 for _, t in picked_later)

    def run(**kw):
        p = PickingParser()
        ctl = C.Ctl(p, callback=False)
        task = BatchingParserTask(ctl, publish="json", max_batch=50, max_delay=0.005, stream=stream, routes=table,
                                  drop_unrouted=drop, route_topics=True, **kw)
        asyncio.run(C._drive(ctl, task, lines))
        assert ctl.cmd == [ln for ln in lines if ln]           # every line keeps its turn
        return ctl.mqtt_publisher.sent, set(p.matches)
    assert run(route_match="any") == (exp, {"any"})
    assert run() == (exp_first, {"first"}) and exp_first != exp
