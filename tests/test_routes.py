"""Payload routes on the device: sdx_route_lines through the C ABI on planted launch outputs,
and the ``routes`` arguments of the front end and the stream.

Expected values come from ``restate`` below, the definition in Python: ``re.search`` per pattern over the
payload of the line's first result, the lowest matching route or -1.  Its inputs are never taken from the
code under test: the payloads the test itself planted, or the reference-recorded payload of the goldens
("e2e" of tests/golden/lines_golden.json.gz)."""
import re

import numpy as np
import pytest

from oracle import json_oracle as J

pytestmark = pytest.mark.gpu

OVERLAP = [("hideki", r"75[A-F0-9]{6,}"), ("tail", r"[A-F]{4}00$"), ("ff", r"^P\d+#(?:..)*FF"), ("empty", r"^$"),
           ("p7", r"^P7#[A-F0-9]{6}$"), ("any_p", r"^P"), ("w", r"^W\d+x{0,1}#.*")]


def restate(patterns, payload):
    """(route, mask) of one payload (bytes) by the definition; None (no result) -> (-1, 0)."""
    if payload is None:
        return -1, 0
    s = payload.decode("latin-1")
    mask = sum(1 << r for r, p in enumerate(patterns) if re.search(p, s))
    return ((mask & -mask).bit_length() - 1 if mask else -1), mask


@pytest.fixture(scope="module")
def eng():
    from pysignalduino_amd.sd_protocols import SDProtocols
    return SDProtocols()._ensure()


@pytest.fixture(scope="module")
def tables():
    from pysignalduino_amd.routes import DEFAULT_ROUTES, RouteTable
    cache = {}

    def get(name):
        if name not in cache:
            pairs = {"default": DEFAULT_ROUTES, "overlap": OVERLAP, "one": [("only", r"^P7#[A-F0-9]{6}$")],
                     "bit63": [(f"q{i}", r"^Q%d#[0-9]+$" % i) for i in range(63)] + [("last", r"^P\d+#")],
                     # 64 DFAs of about 1 KiB each: more than the kernel's LDS holds
                     "big": [(f"b{i}", r"^P%d#[0-9A-F]{%d,%d}Z?$" % (i, 20 + i % 7, 44 + i % 5)) for i in range(64)],
                     # an unanchored window: more than 256 states, so 16-bit transitions
                     "wide": [("win", r"A.{8}B"), ("p", r"^P")]}[name]
            cache[name] = RouteTable(pairs)
        return cache[name]
    return get


class Planted:
    """Launch outputs (descriptors, records, heap) of up to four kinds holding the given per-line results.
    items[i]: None, or (kind, payload[, trailer[, status[, later payloads]]]).  Every payload is followed in
    the heap by ``trailer`` (default b"A0F", hex digits): a walk that read past a payload's end would see a
    longer hex string -- another length against every counted pattern, another tail against every ``$``."""

    def __init__(self, eng, items):
        from pysignalduino_amd import runtime
        t = eng.torch
        self.eng, self.n = eng, len(items)
        n = self.n
        kinds = sorted({it[0] for it in items if it is not None} | {0})
        self.keep, self.ins = [], []
        dummy = t.zeros(32 * max(n, 1), dtype=t.uint8, device=eng.dev)
        for kd in kinds:
            desc = np.zeros(max(n, 1), runtime.DESC_DT)
            recs, heap = [], bytearray(b"\xA5")
            for i, it in enumerate(items):
                if it is None or it[0] != kd:
                    continue
                trailer = it[2] if len(it) > 2 and it[2] is not None else b"A0F"
                later = it[4] if len(it) > 4 else []
                desc[i] = (len(recs), 1 + len(later), it[3] if len(it) > 3 else runtime.ST_OK, 0)
                for payload in [it[1]] + list(later):
                    recs.append((len(heap), len(payload), 1, 0, i))
                    heap += payload + trailer
            rec = np.array(recs, runtime.RES_DT) if recs else np.zeros(1, runtime.RES_DT)
            dev = lambda a: t.from_numpy(np.frombuffer(a.tobytes() if hasattr(a, "tobytes") else bytes(a),  # noqa: E731
                                                       np.uint8).copy()).to(eng.dev)
            out = {"desc": dev(desc), "rec": dev(rec), "heap": dev(heap), "rec_cap": len(rec),
                   "cursor": t.zeros(4, dtype=t.int32, device=eng.dev)}
            self.keep.append(out)
            self.ins.append(eng.json_in(kd, out, {"meta": dummy}, n))


def planted_payloads(items):
    from pysignalduino_amd import runtime
    return [None if it is None or (len(it) > 3 and it[3] != runtime.ST_OK) else bytes(it[1]) for it in items]


def run(eng, table, items, mask=True, skip=True, repeat=None, drop=False):
    """-> (route, mask or None, skip or None) as lists; every buffer is filled with 9s first."""
    t = eng.torch
    p = Planted(eng, items)
    n = p.n
    b = eng.alloc_routes(n, mask=mask, skip=skip)
    for x in b.values():
        if x is not None:
            x.view(t.uint8).fill_(9)   # every entry must be written
    rep = None if repeat is None else t.from_numpy(np.asarray(repeat, np.uint8)).to(eng.dev)
    eng.route_lines(eng.route_table(table), p.ins, n, b["route"], b["mask"], b["skip"], repeat=rep, drop_unrouted=drop)
    host = lambda x: None if x is None else x[:n].cpu().numpy()   # noqa: E731
    m = host(b["mask"])
    return (host(b["route"]).tolist(), None if m is None else m.view(np.uint64).tolist(),
            None if b["skip"] is None else host(b["skip"]).tolist())


def check(eng, table, items):
    """route and mask of the planted chunk == the definition == RouteTable.match; without a mask the same route."""
    pays = planted_payloads(items)
    exp = [restate(table.patterns, p) for p in pays]
    assert [(-1, 0) if p is None else table.match(p) for p in pays] == exp
    route, mask, _ = run(eng, table, items)
    bad = [(i, pays[i][:40], r, hex(m), e) for i, (r, m, e) in enumerate(zip(route, mask, exp)) if (r, m) != e]
    assert not bad, bad[:5]
    assert run(eng, table, items, mask=False, skip=False)[0] == [e[0] for e in exp]
    return exp


def seeded_items(n, seed, none_every=5):
    """Payload-like strings over all four kinds: preambles + hex digits, some empty, some lines without a result."""
    rng = np.random.default_rng(seed)
    pre = ["P7#", "P12#75", "P61#", "W33#", "W113x#", "u40#", "i", "ih", "s", "TX", "Ys", "K", "r", "T", "E01", "", "21",
           "75", "P3#", "81"]
    out = []
    for i in range(n):
        if none_every and i % none_every == 3:
            out.append(None)
            continue
        body = "".join("0123456789ABCDEF"[int(x)] for x in rng.integers(0, 16, int(rng.integers(0, 27))))
        out.append((i % 4, (pre[int(rng.integers(0, len(pre)))] + body).encode()))
    return out


# ---- kernel level: planted launch outputs -----------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_chunk_sizes_and_all_kinds(eng, tables, n):
    items = seeded_items(n, seed=n, none_every=0 if n == 1 else 5)
    exp = check(eng, tables("default"), items)
    if n >= 63:
        assert len({r for r, _ in exp}) > 5 and {it[0] for it in items if it} == {0, 1, 2, 3}
    check(eng, tables("overlap"), items)


def test_chunk_without_results_and_raised_lines(eng, tables):
    from pysignalduino_amd import runtime
    t = tables("overlap")
    items = [None] * 70
    assert run(eng, t, items, drop=True) == ([-1] * 70, [0] * 70, [0] * 70)
    # a raised line's records are not a result; an overflowed one's neither
    items = [(0, b"P7#ABCDEF"), (0, b"P7#ABCDEF", None, runtime.ST_RAISED), None, (1, b"P7#ABCDEF", None, runtime.ST_OVF_OUT),
             (2, b"P7#ABCDEF", None, runtime.ST_OK, [b"W1#later"])]
    exp = check(eng, t, items)
    assert [e[0] for e in exp] == [4, -1, -1, -1, 4]


def test_payload_lengths(eng, tables):
    """0, 1, one short of, equal to and one past a fixed length, and the contract's longest payload; the
    bytes behind each payload would change the verdict if they were read."""
    t = tables("overlap")
    fixed = b"P7#ABCDEF"                               # ^P7#[A-F0-9]{6}$
    big = b"P1#" + b"E7" * 32763 + b"AAAA00"           # 65,535 bytes, decided by its last six ([A-F]{4}00$)
    assert len(big) == 65535
    items = [(0, b""), (3, b"", b"P"), (0, b"P"), (1, b"7"), (0, fixed[:-1]), (0, fixed), (0, fixed + b"0"),
             (1, fixed, b""), (2, b"P7#ABCDE", b"F"),                       # the missing digit stands behind the payload
             (0, b"75ABCDE", b"F"), (0, b"75ABCDEF"), (0, b"X75ABCDEF0"),   # {6,}: one short (the trailer would complete it)
             (1, b"DDDD00"), (1, b"DDDD00", b"0"), (1, b"DDD00"), (1, b"xDDDD00"), (2, b"DDDD0", b"0"),
             (0, b"P1#FF"), (0, b"P1#0FF"), (0, b"P1#00FF"), (0, b"P1#F", b"F"),
             (1, big), (1, big[:-1]), (1, big[:-1], b"0"), (2, big[:-2] + b"0A", b"00")]
    exp = check(eng, t, items)
    assert exp[0] == (3, 1 << 3) and exp[5][0] == 4 and exp[4][0] == 5 and exp[6][0] == 5
    assert exp[9][0] == -1 and exp[10][0] == 0 and exp[21][1] & 2 and not exp[22][1] & 2


def test_one_route_bit_63_and_overlap(eng, tables):
    items = seeded_items(130, seed=2) + [(0, b"P7#ABCDEF"), (1, b"Q5#12"), (0, b"P7#75ABCDEF00FF")]
    exp = check(eng, tables("one"), items)
    assert {e[0] for e in exp} == {-1, 0}
    exp = check(eng, tables("bit63"), items)
    assert (63, 1 << 63) in exp and (5, 1 << 5) in exp
    assert all(m in (0, 1 << 63) for r, m in exp[:130]) and any(m for r, m in exp[:130])
    exp = check(eng, tables("overlap"), items)
    r, m = exp[-1]
    assert bin(m).count("1") >= 3 and r == 0      # several bits, the lowest is the route


def test_tables_in_lds_and_beyond(eng, tables):
    small, big, wide = (eng.route_table(tables(k)) for k in ("default", "big", "wide"))
    assert small.lds_routes == len(small.table)          # wholly in LDS
    assert 0 < big.lds_routes < len(big.table) == 64      # the rest walks global memory
    assert len(tables("wide").blob) > 2 * 256 * 2 and tables("wide").blob[16] == 2     # 16-bit transitions
    rng = np.random.default_rng(4)
    items = []
    for i in range(64):        # every route of "big": inside its range, one short, one past, with and without Z
        lo, hi = 20 + i % 7, 44 + i % 5
        for ln, z in ((lo, b""), (lo - 1, b""), (hi, b"Z"), (hi + 1, b""), (int(rng.integers(lo, hi + 1)), b"")):
            body = bytes(b"0123456789ABCDEF"[int(x)] for x in rng.integers(0, 16, ln))
            items.append((i % 4, b"P%d#" % i + body + z, b"Z" if not z else b"0"))
    exp = check(eng, tables("big"), items)
    hit = {r for r, _ in exp}
    assert hit >= set(range(64)) and -1 in hit
    items = seeded_items(200, seed=6) + [(0, b"A12345678B"), (0, b"A1234567B"), (1, b"xxA12345678", b"B"),
                                         (2, b"PAAAAAAAAAAB"), (3, b"AAAAAAAAA" * 20)]
    exp = check(eng, tables("wide"), items)
    assert exp[200][0] == 0 and exp[201][0] == -1 and exp[202][0] == -1 and exp[203][1] == 3


def test_skip_is_repeat_or_unrouted(eng, tables):
    from pysignalduino_amd import runtime
    t = tables("default")
    items = seeded_items(300, seed=8) + [(0, b"zzz"), (1, b"zzz", None, runtime.ST_RAISED), None]
    pays = planted_payloads(items)
    route = [restate(t.patterns, p)[0] for p in pays]
    rng = np.random.default_rng(9)
    rep = (rng.integers(0, 3, len(items)) == 0).astype(np.uint8) * 5      # any non-zero value marks a repeat
    unrouted = [int(p is not None and r < 0) for p, r in zip(pays, route)]
    assert 0 < sum(unrouted) < len(items) and unrouted[-3:] == [1, 0, 0]
    for repeat, drop in ((None, False), (None, True), (rep, False), (rep, True)):
        got_route, _, skip = run(eng, t, items, repeat=repeat, drop=drop)
        assert got_route == route
        assert skip == [int((repeat is not None and repeat[i] != 0) or (drop and unrouted[i])) for i in range(len(items))]


def test_route_lines_refuses_bad_arguments(eng, tables):
    import ctypes
    from pysignalduino_amd import runtime
    t = eng.torch
    p = Planted(eng, [(0, b"x"), (1, b"x")])
    dt = eng.route_table(tables("one"))
    b = eng.alloc_routes(4)
    with pytest.raises(RuntimeError, match="given twice"):
        eng.route_lines(dt, [p.ins[0], p.ins[0]], 2, b["route"], b["mask"], b["skip"])
    with pytest.raises(RuntimeError, match="chunk's n"):
        eng.route_lines(dt, p.ins, 1, b["route"], b["mask"], b["skip"])
    with pytest.raises(ValueError):
        eng.route_lines(dt, p.ins, 2, b["route"][:1], b["mask"], b["skip"])
    lib = eng.lib
    arr = (runtime.SdxJsonIn * 2)(*p.ins)
    ptr = runtime._ptr
    call = lambda table, n, route, mask: lib.sdx_route_lines(eng.handle, table, arr, 2, n, None, 0, route, mask, None,   # noqa: E731
                                                             eng.stream_ptr())
    assert call(None, 2, ptr(b["route"]), ptr(b["mask"])) == -1                 # SDX_EINVAL
    assert call(dt.handle, 2, None, ptr(b["mask"])) == -1
    assert call(dt.handle, -1, ptr(b["route"]), ptr(b["mask"])) == -1
    assert call(dt.handle, 2, ptr(b["route"]) + 1, ptr(b["mask"])) == -1        # misaligned
    assert call(dt.handle, 2, ptr(b["route"]), ptr(b["mask"]) + 4) == -1
    assert call(dt.handle, 2, ptr(b["route"]), ptr(b["mask"])) == 0
    t.cuda.synchronize()
    # a damaged blob is refused on the host and nothing is uploaded
    good = tables("one").blob
    for blob in (good[:-4], b"\0" + good[1:], good[:48] + b"\xff" + good[49:]):     # size, magic, a cls_of entry
        h = ctypes.c_void_p()
        buf = ctypes.create_string_buffer(blob, len(blob))
        assert lib.sdx_route_table_create(ctypes.cast(buf, ctypes.c_void_p), len(blob), eng.device, ctypes.byref(h)) == -1
        assert not h.value


# ---- front end and stream: the goldens ----------------------------------------------------------------
def e2e_key(e2e):
    """(kind, protocol_id, payload) of the reference's decoded[0]; None when it decoded nothing."""
    return (e2e[0][3][1], e2e[0][0], e2e[0][1]) if e2e else None


def repeats_of(keys):
    """DESIGN.md §4k restated: 1 where a line's key equals the previous result-bearing line's."""
    mask, prev = [], None
    for k in keys:
        mask.append(int(k is not None and k == prev))
        prev = k if k is not None else prev
    return mask


def published(patterns, keys, texts, drop, collapse=False):
    """The definition: per line None or (route, text); published = result, no repeat, routed or not drop."""
    rep = repeats_of(keys) if collapse else [0] * len(keys)
    out = []
    for k, t, m in zip(keys, texts, rep):
        r = restate(patterns, None if k is None else k[2].encode("latin-1"))[0]
        out.append(None if k is None or m or (drop and r < 0) else (r, t))
    return out


@pytest.fixture(scope="module")
def gold(golden):
    """lines_golden.json.gz as recorded from the reference -> (lines, keys, texts); a key's payload is e2e[0]'s."""
    cases = golden("lines_golden.json.gz")
    return ([c["line"] for c in cases], [e2e_key(c.get("e2e", [])) for c in cases],
            [J.published(c.get("e2e", [])) for c in cases])


def kept_rows(got, keys):
    """The lines compared: all but those whose slot is a ContractError, at most 5 % (the bound test_lines.py holds
    this corpus to)."""
    from pysignalduino_amd.packing import ContractError
    out = [i for i, g in enumerate(got) if not isinstance(g, ContractError)]
    assert len(got) - len(out) <= 0.05 * len(got), (len(got) - len(out), len(got))
    return out


def test_parse_lines_routed_goldens(gold):
    from pysignalduino_amd.frontend import SignalParser
    from pysignalduino_amd.routes import DEFAULT_ROUTES, RouteTable
    lines, keys, texts = gold
    table = RouteTable(DEFAULT_ROUTES)
    sp = SignalParser()
    got = sp.parse_lines_routed(lines, table)
    rows = kept_rows(got, keys)
    exp = published(table.patterns, keys, texts, drop=False)
    bad = [(i, lines[i][:60], got[i], exp[i]) for i in rows if got[i] != exp[i]]
    assert not bad, (len(bad), bad[:3])
    routes_seen = {got[i][0] for i in rows if got[i] is not None}
    assert len(routes_seen - {-1}) >= 10 and -1 in routes_seen       # the recorded data gives 16 routes, 67 unrouted
    assert [int(sp.last_routes[i]) for i in rows] == [-1 if exp[i] is None else exp[i][0] for i in rows]
    # it sends exactly parse_lines_json's lines, with parse_lines_json's texts
    plain = sp.parse_lines_json(lines)
    assert [g[1] if isinstance(g, tuple) else g for g in (got[i] for i in rows)] == [plain[i] for i in rows]
    # a list of pairs is taken as well; drop_unrouted: published = result-bearing and routed
    dropped = sp.parse_lines_routed(lines, DEFAULT_ROUTES, drop_unrouted=True)
    exp = published(table.patterns, keys, texts, drop=True)
    assert [dropped[i] for i in rows] == [exp[i] for i in rows]
    assert sum(exp[i] is None and keys[i] is not None for i in rows) >= 1
    assert sp.parse_lines_routed([], table) == []


@pytest.mark.parametrize("output", ["json", "wire"])
def test_stream_chunk_goldens(gold, output):
    from pysignalduino_amd.frontend import SignalParser
    from pysignalduino_amd.routes import DEFAULT_ROUTES, RouteTable
    lines, keys, texts = gold
    table = RouteTable(DEFAULT_ROUTES)
    sp = SignalParser()
    n = len(lines)

    def one_chunk(**kw):
        ls = sp.stream(chunk_lines=n, chunk_bytes=max(1 << 21, 2 * sum(map(len, lines))), output=output, lag=1, **kw)
        ls.submit(lines)
        (r,) = ls.drain()
        return ls, r
    ls0, base = one_chunk()
    assert base.route is None                                   # routes=None: nothing is added
    ls1, r = one_chunk(routes=table)
    assert r.route.dtype == np.int16 and len(r.route) == n
    if output == "json":
        got = [None] * n
        for i, route, x in r.items_routed():
            got[i] = (route, x) if isinstance(x, str) else x
        rows = kept_rows(got, keys)
        exp = published(table.patterns, keys, texts, drop=False)
        assert [got[i] for i in rows] == [exp[i] for i in rows]
        t1, t0 = r.texts(), base.texts()
        assert [t1[i] for i in rows] == [t0[i] for i in rows]     # the texts are today's
        assert ls1.d2h_bytes == ls0.d2h_bytes + 2 * n           # only the routes travel beside today's results
        ls2, rd = one_chunk(routes=DEFAULT_ROUTES, drop_unrouted=True)
        got = [None] * n
        for i, route, x in rd.items_routed():
            got[i] = (route, x) if isinstance(x, str) else x
        exp = published(table.patterns, keys, texts, drop=True)
        assert [got[i] for i in rows] == [exp[i] for i in rows]
        assert rd.route.tolist() == r.route.tolist()
        assert ls2.d2h_bytes < ls1.d2h_bytes                    # the unrouted texts were never built
    else:
        from pysignalduino_amd.packing import ContractError
        rows = [i for i in range(n) if i not in r.host or not isinstance(r.host[i], ContractError)]
        assert n - len(rows) <= 0.05 * n
        exp = published(table.patterns, keys, texts, drop=False)
        assert [int(r.route[i]) for i in rows] == [-1 if exp[i] is None else exp[i][0] for i in rows]
        assert r.layout[2] == base.layout[2] and bytes(r.wire) == bytes(base.wire)      # the sections are unchanged
        assert ls1.d2h_bytes == ls0.d2h_bytes + 2 * n


@pytest.fixture(scope="module")
def repeated(gold, golden):
    """Golden lines the front end answers without ContractError, every result-bearing one 1 to 3 times in a row,
    with host-resolved rows (an LS_GENERAL line the batch API resolves, the corpus of test_repeats.py's
    test_stream_host_resolved_lines) inside and between the runs -> (lines, keys, texts)."""
    from pysignalduino_amd.frontend import SignalParser
    lines, keys, texts = gold
    pick = [i for i in range(len(lines)) if "\n" not in lines[i].strip("\n")]
    plain = SignalParser().parse_lines_json([lines[i] for i in pick])
    pick = [i for i, g in zip(pick, plain) if not isinstance(g, Exception)]
    gen = next(c for c in golden("lines_general_golden.json.gz")
               if c.get("e2e") and "P10=" in c["line"] and "\n" not in c["line"].strip("\n") and len(c["line"]) < 2000)
    G = (gen["line"].strip("\n"), e2e_key(gen["e2e"]), J.published(gen["e2e"]))
    rng = np.random.default_rng(12)
    bearing = [i for i in pick if keys[i] is not None]
    noise = [i for i in pick if keys[i] is None]
    seq = []
    for i in bearing[::3][:230]:
        item = (lines[i].strip("\n"), keys[i], texts[i])
        for _ in range(int(rng.integers(1, 4))):
            seq.append(item)
            x = int(rng.integers(0, 12))
            if x == 0:
                seq.append(G)
            elif x < 3:
                j = noise[int(rng.integers(0, len(noise)))]
                seq.append((lines[j].strip("\n"), None, None))
    seq[256] = G                 # a host row as a chunk's last line, repeated as the next chunk's first
    seq[257] = G
    return [s[0] for s in seq], [s[1] for s in seq], [s[2] for s in seq]


@pytest.mark.parametrize("drop", [False, True])
def test_routes_with_collapse_and_host_rows(repeated, drop):
    """collapse_repeats across chunks of 257 lines, with host-resolved rows: published = result, no repeat,
    routed or not drop; the repeat mask is the one without routes."""
    from pysignalduino_amd.frontend import SignalParser
    from pysignalduino_amd.routes import DEFAULT_ROUTES, RouteTable
    lines, keys, texts = repeated
    table = RouteTable(DEFAULT_ROUTES + [("general", r"^P\d+#")])
    assert len(lines) > 2 * 257 and sum(repeats_of(keys)) > 100
    exp = published(table.patterns, keys, texts, drop, collapse=True)
    unrouted = sum(restate(table.patterns, k[2].encode("latin-1"))[0] < 0 for k in keys if k is not None)
    assert unrouted >= 1
    sp = SignalParser()
    ls = sp.stream(chunk_lines=257, chunk_bytes=1 << 19, output="json", lag=2, collapse_repeats=True, routes=table,
                   drop_unrouted=drop)
    for a in range(0, len(lines), 257):
        ls.submit(lines[a: a + 257])
    got, mask, host_rows = [], [], 0
    for r in ls.drain():
        chunk = [None] * r.n
        for i, route, x in r.items_routed():
            chunk[i] = (route, x)
        got += chunk
        mask += r.repeat.tolist()
        host_rows += len(r.host)
    assert host_rows >= 5
    assert mask == repeats_of(keys)
    assert got == exp
    assert sp.parse_lines_routed(lines, table, drop_unrouted=drop, collapse_repeats=True) == exp
    assert sp.last_repeat_mask.tolist() == repeats_of(keys)
    # without collapse the device drops the unrouted texts itself
    assert sp.parse_lines_routed(lines, table, drop_unrouted=drop) == published(table.patterns, keys, texts, drop)
