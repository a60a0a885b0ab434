"""Payload routes, host side, on the CPU: the route table's compile step and its host walk
against Python's ``re``, the limits, the blob validator as a stand-alone program under the address / UB
sanitizers (tools/route_blob_check.cpp), the ABI's declarations, and the controller's topic logic on a
scripted parser (the stand-ins of tests/test_controller.py)."""
import asyncio
import json
import os
import re
import subprocess

import numpy as np
import pytest

from pysignalduino_amd import routes, runtime
from pysignalduino_amd.controller import BatchingParserTask

import test_controller as C

ROOT = os.path.dirname(runtime.HERE)
SECOND = [("hideki", r"75[A-F0-9]{6,}"), ("tail", r"[A-F]{4}00$"), ("ff", r"^P\d+#(?:..)*FF"), ("empty", r"^$"),
          ("ws", r"^W\d+x{0,1}#.*"), ("lazy", r"^u\d+#.+?0{3}"), ("alt", r"(?:AB|CD){2,3}$"), ("cls", r"^[^P\s]\w{3}\S")]


def bank_preambles():
    with open(os.path.join(runtime.HERE, "data", "sd_bank.json")) as fh:
        protos = json.load(fh)["protocols"]
    pre = sorted({p.get("preamble", "") for p in protos.values()})
    assert len(pre) > 100 and "P7#" in pre and "W33#" in pre
    return pre


def literal_head(pattern):
    """The literal characters a pattern begins with (behind ``^``): what a payload must start with to get far."""
    m = re.match(r"\^?((?:[A-Za-z0-9#]|\\\.)*)", pattern)
    return m.group(1).replace("\\.", ".")


def payload_like(pairs, seed):
    """Bank preambles plus 0-26 hex digits, the empty string, and -- behind every pattern's literal head --
    every length from 0 to 45 in upper and lower case: one character short of, at and past every {m} / {m,n}
    bound of the lists (the largest is 30), with the tails a ``$`` or a literal asks for."""
    rng = np.random.default_rng(seed)
    hexd = lambda k: "".join("0123456789ABCDEF"[int(x)] for x in rng.integers(0, 16, k))   # noqa: E731
    out = ["", " ", "\t9 ", "OK 9 1", "OK  24 x"]
    for pre in bank_preambles():
        for _ in range(6):
            out.append(pre + hexd(int(rng.integers(0, 27))))
    for _, pat in pairs:
        head = literal_head(pat)
        for ln in range(46):
            body = hexd(ln)
            out += [head + body, head + body.lower(), head + "A" * ln, head + body + "00", head + body + "FF",
                    "x" + head + body]
    bounds = {int(x) for _, pat in pairs for q in re.findall(r"\{(\d+)(?:,(\d*))?\}", pat) for x in q if x}
    assert bounds and max(bounds) <= 44
    return out


@pytest.mark.parametrize("name", ["default", "second"])
def test_match_equals_re_search(name):
    pairs = routes.DEFAULT_ROUTES if name == "default" else SECOND
    t = routes.RouteTable(pairs)
    assert t.names == [n for n, _ in pairs] and len(t) == len(pairs)
    assert len(t.blob) % 4 == 0 and len(t.blob) <= routes.BLOB_MAX and t.blob[16] == 1     # uint8 transitions
    rx = [re.compile(p) for _, p in pairs]
    strings = payload_like(pairs, seed=1)
    assert len(strings) > 2000
    hits = np.zeros(len(pairs), int)
    for s in strings:
        mask = sum(1 << r for r, x in enumerate(rx) if x.search(s))
        route = (mask & -mask).bit_length() - 1 if mask else -1
        assert t.match(s) == (route, mask), (s, t.match(s), route, hex(mask))
        assert t.match(s.encode("latin-1")) == (route, mask)
        for r in range(len(pairs)):
            hits[r] += (mask >> r) & 1
    assert (hits > 0).sum() >= len(pairs) - 6, hits      # the strings reach nearly every route (not the exotic heads)
    assert (hits < len(strings)).all()


def test_default_routes_shape():
    assert 30 <= len(routes.DEFAULT_ROUTES) <= routes.ROUTES_MAX
    assert len({n for n, _ in routes.DEFAULT_ROUTES}) == len(routes.DEFAULT_ROUTES)
    t = routes.RouteTable(routes.DEFAULT_ROUTES)
    assert t.match("P7#6B20B7F32")[0] == t.names.index("SD_WS07")
    assert t.match("W33#844E935AFF2")[0] == t.names.index("SD_WS")
    assert t.match("i0D1787")[0] == t.names.index("IT")
    assert t.match("210D4E334880") == (-1, 0)
    assert t.name_of(-1) is None and t.name_of(0) == "IT"
    # latin-1 bytes are matched as bytes; a newline-free payload makes $ unambiguous
    assert routes.RouteTable([("x", "^\xe9.$")]).match("\xe9\xff") == (0, 1)


def test_limits_and_unsupported_syntax(monkeypatch):
    with pytest.raises(ValueError, match="64"):
        routes.RouteTable([(f"r{i}", "^a") for i in range(65)])
    with pytest.raises(ValueError):
        routes.RouteTable([])
    assert len(routes.RouteTable([(f"r{i}", "^a%d" % i) for i in range(64)])) == 64
    for bad in (r"^P(?=7)", r"\bP7", r"(?P<n>a)", r"a\1", r"(?i)a"):
        with pytest.raises(NotImplementedError):
            routes.RouteTable([("ok", "^P"), ("bad", bad)])
    with pytest.raises(ValueError, match=r"a\.\{11\}b.*4096"):      # 2^12 states: named, and stopped at the limit
        routes.RouteTable([("ok", "^P"), ("wide", r"a.{11}b")])
    wide = routes.RouteTable([("win", r"A.{8}B"), ("p", "^P")])     # more than 256 states: uint16 transitions
    assert wide.blob[16] == 2 and wide.match("xxA12345678B") == (0, 1) and wide.match("PA1234567B") == (1, 2)
    monkeypatch.setattr(routes, "BLOB_MAX", 4096)
    with pytest.raises(ValueError, match=r"A\.\{8\}B.*4096 bytes"):
        routes.RouteTable([("p", "^P"), ("win", r"A.{8}B")])


def test_abi_declares_the_route_entries():
    hdr = open(os.path.join(ROOT, "include", "sdx.h")).read()
    for name in ("sdx_route_table_create", "sdx_route_table_destroy", "sdx_route_table_lds_routes", "sdx_route_lines"):
        assert name in runtime.EXPORTED and re.search(r"\b%s\(" % name, hdr), name
    assert "#define SDX_ABI_VERSION 14" in hdr and runtime.ABI_VERSION == 14     # only new entries: the version stays
    lib = runtime.load_library()
    assert lib.sdx_abi_version() == 14 and lib.sdx_route_table_lds_routes(None) == -1
    # the constants routes.py mirrors
    lay = open(os.path.join(runtime.HERE, "csrc", "sdx_route_layout.h")).read()
    for name, val in (("SDX_ROUTE_MAGIC", "0x%08Xu" % routes.MAGIC), ("SDX_ROUTE_VERSION", "%du" % routes.VERSION),
                      ("SDX_ROUTE_MAX", str(routes.ROUTES_MAX)), ("SDX_ROUTE_STATES_MAX", str(routes.STATES_MAX)),
                      ("SDX_ROUTE_BLOB_MAX", "(1u << 20)")):
        assert re.search(r"#define %s %s\s" % (name, re.escape(val)), lay), name
    from pysignalduino_amd import build
    assert any(s.endswith("sdx_route.hip") for s in build.SRCS) and any(d.endswith("sdx_route_layout.h") for d in build.DEPS)


def test_blob_validator_under_sanitizers(tmp_path):
    """tools/route_blob_check.cpp: sdx_route_validate over a good blob and systematically damaged ones --
    truncated at every section boundary, an out-of-range transition, class and start state, wrong magic --
    as a stand-alone host program built with -fsanitize=address,undefined.  Both transition widths."""
    src = os.path.join(ROOT, "tools", "route_blob_check.cpp")
    exe = str(tmp_path / "route_blob_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    src, "-o", exe], check=True)
    for name, pairs in (("default", routes.DEFAULT_ROUTES), ("second", SECOND),
                        ("wide", [("win", r"A.{8}B"), ("p", "^P")])):
        blob = tmp_path / (name + ".blob")
        blob.write_bytes(routes.RouteTable(pairs).blob)
        r = subprocess.run([exe, str(blob)], capture_output=True, text=True)
        assert r.returncode == 0 and "route_blob_check: ok" in r.stdout, (name, r.stdout, r.stderr[-2000:])
    bad = tmp_path / "bad.blob"
    bad.write_bytes(b"\0" * 64)
    assert subprocess.run([exe, str(bad)], capture_output=True).returncode != 0      # the program does refuse


# ---- controller: topics per route on a scripted parser ----------------------------------------------
TABLE = [("ms", r"^MS;"), ("even", r"[02468];$"), ("mc", r"^MC;")]


class RoutedParser(C.FakeParser):
    """The scripted parser of test_controller.py with the routed entries: a line's payload is the line
    itself, routed by the table's host walk (this test is about topics, not about matching)."""

    def parse_lines_routed(self, lines, table, drop_unrouted=False):
        out = []
        for ln, x in zip(lines, self.parse_lines_json(lines)):
            r = table.match(ln)[0] if isinstance(x, str) else -1
            out.append(x if not isinstance(x, str) else None if drop_unrouted and r < 0 else (r, x))
        return out

    def stream(self, chunk_lines, output="json", lag=3, routes=None, drop_unrouted=False):
        assert output == "json"
        return RoutedStream(self, lag, routes, drop_unrouted)


class _RoutedChunk(C._Chunk):
    def items_routed(self):
        return [(i, x[0] if isinstance(x, tuple) else -1, x[1] if isinstance(x, tuple) else x)
                for i, x in enumerate(self._t) if x is not None]


class RoutedStream(C.FakeStream):
    def __init__(self, parser, lag, table, drop):
        super().__init__(parser, lag)
        self.table, self.drop = table, drop

    def submit(self, lines):
        if self.table is None:
            return super().submit(lines)
        self.q.append(_RoutedChunk(self.parser.parse_lines_routed(lines, self.table, self.drop), self.submitted))
        self.submitted += 1
        return self.submitted - 1


def expected_publications(lines, table, drop, topics):
    sent = []
    for ln in lines:
        if not ln or "boom" in ln:
            continue
        dec = C.FakeParser().parse_line(ln)
        if not dec:
            continue
        r = table.match(ln)[0]
        if drop and r < 0:
            continue
        topic = "t/v1/state/messages" + ("/" + table.names[r] if topics and r >= 0 else "")
        sent.append((topic, json.dumps(dec[0])))
    return sent


@pytest.mark.parametrize("stream", [True, False])
@pytest.mark.parametrize("drop,topics", [(False, False), (False, True), (True, True), (True, False)])
def test_controller_route_topics(stream, drop, topics):
    lines = ([f"MS;P0={i};" for i in range(300)] + ["boom", ""] + [f"MC;D={i};" for i in range(200)] +
             [f"MU;D={i};" for i in range(200)])
    table = routes.RouteTable(TABLE)
    ctl = C.Ctl(RoutedParser(), callback=False)
    task = BatchingParserTask(ctl, publish="json", max_batch=50, max_delay=0.005, stream=stream, routes=table,
                              drop_unrouted=drop, route_topics=topics)
    asyncio.run(C._drive(ctl, task, lines))
    exp = expected_publications(lines, table, drop, topics)
    assert ctl.mqtt_publisher.sent == exp
    assert ctl.cmd == [ln for ln in lines if ln] and task.lines == len(ctl.cmd)      # every line keeps its turn
    used = {t for t, _ in exp}
    assert ("t/v1/state/messages/ms" in used) == topics and ("t/v1/state/messages/even" in used) == topics
    assert ("t/v1/state/messages" in used) == (not topics or not drop)     # unrouted texts: the base topic, or dropped
    _, ref, _ = C.reference_side_effects(C.FakeParser(), lines)
    assert (len(exp) < len(ref)) == drop


@pytest.mark.parametrize("stream", [True, False])
def test_controller_defaults_publish_as_before(stream):
    """Without routes the task never touches a routed entry: the scripted parser of test_controller.py,
    which has none, gives today's publications on today's topic."""
    lines = [f"MC;D={i};" for i in range(500)] + ["boom", ""] + [f"MS;P0={i};" for i in range(77)]
    ctl = C.Ctl(C.FakeParser(), callback=False)
    task = BatchingParserTask(ctl, publish="json", max_batch=50, max_delay=0.005, stream=stream)
    asyncio.run(C._drive(ctl, task, lines))
    _, sent, cmd = C.reference_side_effects(C.FakeParser(), lines)
    assert ctl.mqtt_publisher.sent == [("t/v1/state/messages", json.dumps(s[0])) for s in sent] and ctl.cmd == cmd


def test_controller_refuses_inconsistent_arguments():
    ctl = C.Ctl(RoutedParser(), callback=False)
    for kw in ({"drop_unrouted": True}, {"route_topics": True}):
        with pytest.raises(ValueError):
            BatchingParserTask(ctl, publish="json", **kw)
    with pytest.raises(ValueError):      # the routes come with the device's texts
        BatchingParserTask(C.Ctl(RoutedParser(), callback=False), publish="objects", routes=TABLE)
    assert BatchingParserTask(ctl, publish="json", routes=TABLE).routes.names == ["ms", "even", "mc"]


# ---- LineStream against a scripted engine (the stand-ins of test_repeats_host.py / test_stream_host.py) ------
import sys      # noqa: E402
import types    # noqa: E402

import test_repeats_host as R    # noqa: E402
import test_stream_host as H     # noqa: E402

from pysignalduino_amd import frontend, stream   # noqa: E402

STREAM_TABLE = [("a", r"^aa$"), ("g", r"^gg")]      # the scripted payloads: aa and gg (a host row) routed, bb not


class RouteEngine(R.RepeatEngine):
    """RepeatEngine + the route entries: route_lines is the definition over the lines the device sees."""

    def route_table(self, table):
        return types.SimpleNamespace(table=routes.as_table(table))

    def alloc_routes(self, n, mask=True, skip=True):
        n = max(n, 1)
        return {"route": H.FT(np.full(n, 9, np.int16)), "mask": H.FT(np.full(n, 9, np.int64)) if mask else None,
                "skip": H.FT(np.full(n, 9, np.uint8)) if skip else None}

    def route_lines(self, table, json_ins, n, route, mask=None, skip=None, repeat=None, drop_unrouted=False, stream=None):
        self.calls.append(("route", n, stream))
        lb = json_ins[0][1]
        route.a[:n] = -1
        if skip is not None:
            skip.a[:n] = 0 if repeat is None else (repeat.a[:n] != 0)
        for i, ln in self._text_lines(lb, n):
            r = table.table.match(R.line_key(ln)[2])[0]
            route.a[i] = r
            if skip is not None and drop_unrouted and r < 0:
                skip.a[i] = 1


@pytest.fixture
def routed_stub(monkeypatch):
    ft = H.fake_torch()
    ft.int16 = np.int16
    monkeypatch.setitem(sys.modules, "torch", ft)
    monkeypatch.setattr(frontend, "LineBatch", H.FakeLineBatch)

    def copy(dst, src, st=None):
        dst.a.view(np.uint8)[:] = src.a.view(np.uint8)

    def fill(dst, st=None, value=0):
        dst.a.view(np.uint8)[:] = value
    monkeypatch.setattr(runtime, "copy_async", copy)
    monkeypatch.setattr(runtime, "copy_d2h", copy)
    monkeypatch.setattr(runtime, "fill_async", fill)
    return RouteEngine()


def stream_definition(seq, table, collapse, drop):
    keys = [R.line_key(x) for x in seq]
    rep = R.restate(keys) if collapse else [0] * len(seq)
    route = [table.match(k[2])[0] if k else -1 for k in keys]
    texts = [R.line_text(x) if k and not m and (r >= 0 or not drop) else None for x, k, m, r in zip(seq, keys, rep, route)]
    return rep, route, texts


@pytest.mark.parametrize("collapse", [False, True])
@pytest.mark.parametrize("drop", [False, True])
def test_stream_routes_against_a_scripted_engine(routed_stub, collapse, drop):
    eng = routed_stub
    table = routes.RouteTable(STREAM_TABLE)
    ls = stream.LineStream(R.RepeatParser(eng), chunk_lines=16, chunk_bytes=4096, output="json", lag=2,
                           collapse_repeats=collapse, routes=table, drop_unrouted=drop)
    seq = R.scripted_lines()
    got = []
    for a in range(0, len(seq), 16):
        ls.submit(seq[a: a + 16])
    got = [r.detach() for r in ls.drain()]
    rep, route, texts = stream_definition(seq, table, collapse, drop)
    assert [x for r in got for x in r.route.tolist()] == route and got[0].route.dtype == np.int16
    assert [t for r in got for t in r.texts()] == texts
    if collapse:
        assert [m for r in got for m in r.repeat.tolist()] == rep        # routing does not change the repeats
    flat = [(16 * c + i, rt, x) for c, r in enumerate(got) for i, rt, x in r.items_routed()]
    assert flat == [(i, route[i], t) for i, t in enumerate(texts) if t is not None]
    assert any(t is None and k and not m for t, k, m in zip(texts, map(R.line_key, seq), rep)) == drop
    # one route pass per chunk, behind the chunk's repeat pass and in front of its JSON launches
    calls = [c[0] for c in eng.calls]
    assert calls.count("route") == len(got) == 6 and calls.count("mark") == (6 if collapse else 0)
    at = [i for i, c in enumerate(calls) if c == "route"]
    for i, nxt in zip(at, at[1:] + [len(calls)]):
        seg = calls[i + 1: nxt]          # the chunk's JSON launches, then the next chunk's demodulation (and repeat pass)
        assert seg[: seg.count("json")] == ["json"] * seg.count("json")
        assert not collapse or calls[i - 1] == "mark"
    assert calls.count("json") > 5


def test_stream_without_routes_launches_no_route_pass(routed_stub):
    eng = routed_stub
    ls = stream.LineStream(R.RepeatParser(eng), chunk_lines=16, chunk_bytes=4096, output="json", lag=2)
    seq = R.scripted_lines()
    ls.submit(seq[:16])
    r = ls.drain()[0]
    assert r.route is None and not any(c[0] == "route" for c in eng.calls)
    assert [t for t in r.texts()] == [R.line_text(x) for x in seq[:16]]
    with pytest.raises(ValueError):
        stream.LineStream(R.RepeatParser(eng), chunk_lines=16, chunk_bytes=4096, drop_unrouted=True)
