"""route_match="any" on the device: sdx_route_records and sdx_route_skip through the C ABI on
planted launch outputs, the picked views through the existing first_only consumers, and the ``route_match``
arguments of the front end and the stream.

Expected values come from ``restate_pick`` (test_route_records_host.py), the definition in Python: the first
message of the line, in list order, that some pattern matches by ``re.search``.  Its inputs are never taken
from the code under test: the payloads the test itself planted, or the reference-recorded message lists of
the goldens ("e2e" of tests/golden/lines_golden.json.gz)."""
import ctypes

import numpy as np
import pytest

from oracle import json_oracle as J

import test_routes as TR
from test_route_records_host import restate_pick
from test_routes import eng, gold, repeated, tables  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

OK, RAISED, OVF_OUT, ABSENT = 0, 1, 3, 0xFF
TRAIL = b"A0F"     # hex digits behind every payload: another length against every counted pattern, another tail for '$'


class Plant:
    """Launch outputs (descriptors, records, heap) of the kinds that occur (kind 0 always).  lines[i]: a list of
    slots (kind, records[, status]); a record is a payload (proto 1) or (proto, payload[, trailer]).  Every payload
    is followed in the heap by its trailer (default TRAIL)."""

    def __init__(self, eng, lines):
        from pysignalduino_amd import runtime
        t = eng.torch
        self.eng, self.n, self.lines = eng, len(lines), lines
        n = self.n
        self.kinds = sorted({s[0] for ln in lines for s in ln} | {0})
        self.keep, self.ins, self.desc = [], [], []
        dummy = t.zeros(32 * max(n, 1), dtype=t.uint8, device=eng.dev)
        dev = lambda a: t.from_numpy(np.frombuffer(a.tobytes() if hasattr(a, "tobytes") else bytes(a),  # noqa: E731
                                                   np.uint8).copy()).to(eng.dev)
        for kd in self.kinds:
            desc = np.zeros(max(n, 1), runtime.DESC_DT)
            recs, heap = [], bytearray(b"\xA5")
            for i, ln in enumerate(lines):
                for s in ln:
                    if s[0] != kd:
                        continue
                    desc[i] = (len(recs), len(s[1]), s[2] if len(s) > 2 else OK, 2 if len(s) > 2 and s[2] == RAISED else 0)
                    for r in s[1]:
                        proto, payload, trailer = (1, r, TRAIL) if isinstance(r, bytes) else (tuple(r) + (TRAIL,))[:3]
                        recs.append((len(heap), len(payload), proto, 0, i))
                        heap += payload + trailer
            rec = np.array(recs, runtime.RES_DT) if recs else np.zeros(1, runtime.RES_DT)
            out = {"desc": dev(desc), "rec": dev(rec), "heap": dev(heap), "rec_cap": len(rec),
                   "cursor": t.zeros(4, dtype=t.int32, device=eng.dev)}
            self.keep.append(out)
            self.desc.append(desc[:n].copy())
            self.ins.append(eng.json_in(kd, out, {"meta": dummy}, n))

    def own(self, i):
        """(kind, records) whose list is line i's result: the lowest kind with ST_OK and records; or None."""
        for kd in self.kinds:
            for s in self.lines[i]:
                if s[0] == kd and (len(s) < 3 or s[2] == OK) and s[1]:
                    return kd, [r if isinstance(r, bytes) else r[1] for r in s[1]]
        return None

    def expect(self, patterns):
        """-> ([(pick, route, mask)], the views' descriptor arrays) by the definition."""
        res, views = [], [d.copy() for d in self.desc]
        for i in range(self.n):
            o = self.own(i)
            if o is None:
                res.append((0, -1, 0))
                continue
            res.append(restate_pick(patterns, [p.decode("latin-1") for p in o[1]]))
            v = views[self.kinds.index(o[0])]
            v[i] = (int(v[i]["rec_begin"]) + res[-1][0], 1, OK, 0)
        return res, views

    def run(self, table, mask=True):
        """-> ([(pick, route, mask or None)], the views as descriptor arrays, the device buffers); outputs pre-filled with 9s."""
        from pysignalduino_amd import runtime
        eng, n, t = self.eng, self.n, self.eng.torch
        b = eng.alloc_routes(n, mask=mask, skip=False, pick=True, views=len(self.ins))
        for x in [b["route"], b["mask"], b["pick"]] + b["views"]:
            if x is not None:
                x.view(t.uint8).fill_(9)   # every entry must be written
        eng.route_records(eng.route_table(table), self.ins, n, b["route"], b["pick"], b["views"], mask=b["mask"])
        route = b["route"][:n].cpu().numpy().tolist()
        pick = b["pick"][:n].cpu().numpy().view(np.uint16).tolist()
        m = b["mask"][:n].cpu().numpy().view(np.uint64).tolist() if mask else [None] * n
        views = [v[: 8 * n].cpu().numpy().view(runtime.DESC_DT) for v in b["views"]]
        return list(zip(pick, route, m)), views, b


def check(eng, table, lines):
    """pick, route, mask and views of the planted chunk == the definition == RouteTable.pick; without a mask the
    same picks and routes."""
    p = Plant(eng, lines)
    exp, exp_views = p.expect(table.patterns)
    for i in range(p.n):
        o = p.own(i)
        assert table.pick(o[1] if o else []) == exp[i]
    got, views, _ = p.run(table)
    bad = [(i, g, e) for i, (g, e) in enumerate(zip(got, exp)) if g != e]
    assert not bad, bad[:5]
    for kd, v, e in zip(p.kinds, views, exp_views):
        assert v.tobytes() == e.tobytes(), (kd, np.nonzero(v != e)[0][:5])
    got2, views2, _ = p.run(table, mask=False)
    assert [g[:2] for g in got2] == [e[:2] for e in exp]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(views2, exp_views))
    return p, exp


HIT = [b"P7#ABCDEF", b"P61#8F88343C58", b"W33#0123", b"s12345678", b"P1#7077CBC3", b"P72#7077CBC3A6", b"i123456", b"TX12345678901"]
MISS = [b"u40#C1DF2F0E98", b"u9#12", b"P3#zz", b"", b"x", b"u40#75", b"P7#ABCDE", b"P1#7077CBC"]   # the trailer would complete the last two


def mixed_lines(n, seed, none_every=7):
    """n lines over all four kinds with 1 to 5 records; by i % 4 the first match is at index 0, 1, n_rec - 1, nowhere."""
    rng = np.random.default_rng(seed)
    hit = lambda: HIT[int(rng.integers(0, len(HIT)))] + b"%X" % int(rng.integers(0, 256))   # noqa: E731
    miss = lambda: MISS[int(rng.integers(0, len(MISS)))]                                     # noqa: E731
    out = []
    for i in range(n):
        if none_every and i % none_every == 5:
            out.append([])
            continue
        k = 1 + int(rng.integers(0, 5))
        at = {0: 0, 1: min(1, k - 1), 2: k - 1, 3: k}[i % 4]
        recs = [miss() for _ in range(min(at, k))] + ([hit()] if at < k else [])
        recs += [(hit() if rng.integers(0, 2) else miss()) for _ in range(k - len(recs))]
        out.append([((i // 4) % 4, recs)])
    return out


# ---- kernel level: planted launch outputs -----------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_chunk_sizes_all_kinds_and_match_positions(eng, tables, n):
    lines = mixed_lines(n, seed=n, none_every=0 if n == 1 else 7)
    for name in ("default", "overlap"):
        p, exp = check(eng, tables(name), lines)
    if n >= 63:
        _, exp = check(eng, tables("default"), lines)
        assert {ln[0][0] for ln in lines if ln} == {0, 1, 2, 3}
        lens = [len(ln[0][1]) if ln else 0 for ln in lines]
        assert set(lens) >= {1, 2, 3, 4, 5}
        picks = [e[0] for e in exp]
        assert any(pk == 0 and r >= 0 for pk, r, _ in exp) and 1 in picks
        assert any(pk == k - 1 and k > 2 for pk, k in zip(picks, lens))           # the last record
        assert any(r < 0 and k > 1 for (_, r, _), k in zip(exp, lens))           # none of several


def test_long_lines(eng, tables):
    """300 records of which only the last matches; 4,096 of which none does.  Two-byte payloads; behind each
    stand bytes that would make it match (75 + ABCDEF0: 75[A-F0-9]{6,})."""
    t = tables("overlap")
    miss = (1, b"75", b"ABCDEF0")
    lines = [[(0, [b"P7#ABCDEF"])], [(1, [miss] * 299 + [(1, b"PA", b"")])], [(2, [miss] * 4096)], [(0, [miss, b"W1#"])]]
    p, exp = check(eng, t, lines)
    assert [e[:2] for e in exp] == [(0, 4), (299, 5), (0, -1), (1, 6)]


def test_lines_without_a_pick_keep_their_descriptors(eng, tables):
    t = tables("overlap")
    good = [b"zz", b"P7#ABCDEF"]
    lines = [[(0, good)], [(0, good, RAISED)], [], [(1, good, OVF_OUT)], [(2, good, ABSENT)], [(3, [])], [(3, good)],
             [(1, [], OK)]]
    p, exp = check(eng, t, lines)
    assert [e[:2] for e in exp] == [(1, 4), (0, -1), (0, -1), (0, -1), (0, -1), (0, -1), (1, 4), (0, -1)]
    got, views, _ = p.run(t)
    assert views[1][3]["status"] == OVF_OUT and views[1][3]["n_rec"] == 2 and views[2][4]["status"] == ABSENT
    assert views[0][1]["status"] == RAISED and views[0][1]["raise_kind"] == 2        # a byte copy
    # a chunk without any result
    p, exp = check(eng, t, [[]] * 70)
    assert exp == [(0, -1, 0)] * 70


def test_two_kinds_on_one_line_the_lowest_wins(eng, tables):
    t = tables("overlap")
    lines = [[(2, [b"zz", b"zz", b"W1#a"]), (1, [b"zz", b"P7#ABCDEF"])],      # kind 1 owns the line
             [(3, [b"P7#ABCDEF"]), (0, [b"zz", b"yy"])],                      # kind 0 owns it and is unrouted
             [(0, [b"P7#ABCDEF"], RAISED), (1, [b"x", b"y", b"W2#"])],        # kind 0 raised: kind 1 owns it
             [(1, [b"W5#"])]]
    p, exp = check(eng, t, lines)
    assert [e[:2] for e in exp] == [(1, 4), (0, -1), (2, 6), (0, 6)]
    _, views, _ = p.run(t)
    k = p.kinds.index
    assert tuple(views[k(2)][0]) == tuple(p.desc[k(2)][0]) and views[k(2)][0]["n_rec"] == 3       # the other kind: a copy
    assert views[k(1)][0]["n_rec"] == 1 and views[k(1)][0]["rec_begin"] == p.desc[k(1)][0]["rec_begin"] + 1
    assert tuple(views[k(3)][1]) == tuple(p.desc[k(3)][1])


def test_one_record_per_line_is_route_lines(eng, tables):
    items = TR.seeded_items(300, seed=3)
    for name in ("default", "overlap"):
        t = tables(name)
        route, mask, _ = TR.run(eng, t, items)
        lines = [[] if it is None else [(it[0], [it[1]])] for it in items]
        p = Plant(eng, lines)
        got, views, _ = p.run(t)
        assert [g[1] for g in got] == route and [g[2] for g in got] == mask and all(g[0] == 0 for g in got)
        assert all(v.tobytes() == d.tobytes() for v, d in zip(views, p.desc))     # the views are the inputs


def test_tables_in_lds_beyond_and_wide(eng, tables):
    small, big, wide = (eng.route_table(tables(k)) for k in ("default", "big", "wide"))
    assert small.lds_routes == len(small.table) and 0 < big.lds_routes < len(big.table) == 64
    rng = np.random.default_rng(4)
    lines = []
    for i in range(64):     # every route of "big" as the line's second or third record, behind records one short / one past
        lo, hi = 20 + i % 7, 44 + i % 5
        body = lambda ln: bytes(b"0123456789ABCDEF"[int(x)] for x in rng.integers(0, 16, ln))   # noqa: E731
        recs = [(1, b"P%d#" % i + body(lo - 1), b"0"), (1, b"P%d#" % i + body(hi + 1), b"Z")][: 1 + i % 2]
        lines.append([(i % 4, recs + [(1, b"P%d#" % i + body(int(rng.integers(lo, hi + 1))), b"Z")])])
        lines.append([(i % 4, recs)])
    p, exp = check(eng, tables("big"), lines)
    assert {e[1] for e in exp} >= set(range(64)) | {-1} and {e[0] for e in exp} == {0, 1, 2}
    lines = mixed_lines(130, seed=6) + [[(0, [b"xx", b"A12345678B"])], [(0, [b"A1234567B", (1, b"xxA12345678", b"B")])],
                                        [(2, [b"zz", b"", b"PAAAAAAAAAAB"])], [(3, [b"AAAAAAAAA" * 20, b"P"])]]
    p, exp = check(eng, tables("wide"), lines)
    assert tables("wide").blob[16] == 2
    assert [e[:2] for e in exp[130:]] == [(1, 0), (0, -1), (2, 0), (1, 1)] and exp[132][2] == 3


def test_views_through_serialize_json_skip(golden):
    """An MU launch of golden lines with several recorded messages: sdx_serialize_json_skip over the picked view gives
    the reference's text of message ``pick``; over the launch's own descriptors it gives message 0's."""
    from pysignalduino_amd import runtime
    from pysignalduino_amd.frontend import LineBatch, SignalParser, pack_lines
    from pysignalduino_amd.routes import DEFAULT_ROUTES, RouteTable
    table = RouteTable(DEFAULT_ROUTES)
    cases = [c for c in golden("lines_golden.json.gz") if c.get("e2e") and c["e2e"][0][3][1] == "MU"]
    exp = [restate_pick(table.patterns, [m[1] for m in c["e2e"]]) for c in cases]
    order = sorted(range(len(cases)), key=lambda i: -exp[i][0])[:150]      # the lines with a later pick first
    cases, exp = [cases[i] for i in order], [exp[i] for i in order]
    assert sum(e[0] > 0 for e in exp) >= 20
    lines = [c["line"] for c in cases]
    n = len(lines)
    sp = SignalParser()
    eng = sp.protocols._ensure()
    t = eng.torch
    data, offsets, bad = pack_lines(lines)
    lb = LineBatch(eng, data, offsets)
    lb.launch()
    sels, cnt = lb.selections()
    out = eng.alloc_out(n, 8 * n + 1024, 200 * n + 65536, eng.pulses_work_bytes(n))
    for sel, long_v in ((sels[runtime.SEL_MU_SHORT], False), (sels[runtime.SEL_MU_LONG], True)):
        if sel.numel():
            eng.launch_pulses(runtime.KIND_MU, lb.pulse_batch(), out, sel=sel, long_variant=long_v)
    lo = {"meta": lb.meta, "pat_val": lb.pat_val, "cp_slot": lb.cp_slot}
    ji = eng.json_in(runtime.KIND_MU, out, lo, n)
    b = eng.alloc_routes(n, mask=False, skip=True, pick=True, views=1)
    eng.route_records(eng.route_table(table), [ji], n, b["route"], b["pick"], b["views"])
    eng.route_skip([eng.json_in_view(ji, b["views"][0])], n, b["route"], b["skip"])
    st = out["desc"][: 8 * n].cpu().numpy().view(runtime.DESC_DT)["status"]
    ls = lb.status[:n].cpu().numpy()
    rows = [i for i in range(n) if st[i] == OK and ls[i] == runtime.LS_OK and i not in bad]
    assert len(rows) >= 0.9 * n
    got = list(zip(b["pick"][:n].cpu().numpy().view(np.uint16).tolist(), b["route"][:n].cpu().numpy().tolist()))
    assert [got[i] for i in rows] == [exp[i][:2] for i in rows]

    def texts(desc):
        jo = eng.alloc_json(n, 600 * n + 65536)
        eng.launch_json(runtime.KIND_MU, dict(out, desc=desc), lo, n, jo, first_only=True, skip=b["skip"])
        used = int(jo["cursor"].cpu().numpy()[0])
        off, ln = jo["off"][:n].cpu().numpy(), jo["len"][:n].cpu().numpy()
        blob = jo["json"][:used].cpu().numpy().tobytes()
        return [blob[o: o + k].decode("ascii") for o, k in zip(off.tolist(), ln.tolist())]
    picked, first = texts(b["views"][0]), texts(out["desc"])
    assert [picked[i] for i in rows] == [J.published(cases[i]["e2e"][exp[i][0]: exp[i][0] + 1]) for i in rows]
    assert [first[i] for i in rows] == [J.published(cases[i]["e2e"]) for i in rows]
    assert sum(picked[i] != first[i] for i in rows) >= 20


def test_views_through_mark_repeats(eng, tables):
    """sdx_mark_repeats over the views marks by the picked records' keys (kind, proto, payload)."""
    t = tables("overlap")
    u, v = (5, b"u40#AA"), (5, b"u40#BB")
    a, b2 = (7, b"P7#ABCDEF"), (8, b"P7#ABCDEF")       # the same bytes under another protocol: another key
    w = (7, b"W1#77")
    lines = [[(0, [u, a])], [(0, [u, a])],             # equal first records, equal picks: a repeat either way
             [(0, [u, w])],                            # equal first record, another pick: no repeat over the views
             [(0, [v, w])],                            # another first record, the same pick: a repeat over the views
             [(0, [u, b2])], [(1, [u, b2])],           # the protocol and the kind belong to the key
             [], [(1, [v, v, b2])],                    # a line without a result does not end the run
             [(0, [u])], [(0, [u, v])],                # unrouted lines: their first records
             [(0, [v, u])]]
    p = Plant(eng, lines)
    exp, _ = p.expect(t.patterns)
    got, views, bufs = p.run(t)
    assert [g[0] for g in got] == [e[0] for e in exp] == [1, 1, 1, 1, 1, 1, 0, 2, 0, 0, 0]

    def mark(ins):
        rep, scratch = eng.alloc_repeat(p.n)
        rep.fill_(9)
        eng.mark_repeats(ins, p.n, rep, scratch, eng.alloc_repeat_state())
        return rep[: p.n].cpu().numpy().tolist()

    def key(i, pk):
        o = p.own(i)
        if o is None:
            return None
        rec = next(s for s in lines[i] if s[0] == o[0])[1][pk]
        return (o[0], rec[0], rec[1])
    over_views = mark([eng.json_in_view(ji, vw) for ji, vw in zip(p.ins, bufs["views"])])
    over_first = mark(p.ins)
    assert over_views == TR.repeats_of([key(i, exp[i][0]) for i in range(p.n)]) == [0, 1, 0, 1, 0, 0, 0, 1, 0, 1, 0]
    assert over_first == TR.repeats_of([key(i, 0) for i in range(p.n)]) == [0, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0]


def test_route_skip_is_repeat_or_unrouted(eng, tables):
    t = tables("default")
    lines = mixed_lines(300, seed=8) + [[(0, [b"zzz", b"yy"])], [(1, [b"zzz"], RAISED)], []]
    p = Plant(eng, lines)
    exp, _ = p.expect(t.patterns)
    got, _, b = p.run(t)
    n = p.n
    rng = np.random.default_rng(9)
    rep = (rng.integers(0, 3, n) == 0).astype(np.uint8) * 5      # any non-zero value marks a repeat
    unrouted = [int(p.own(i) is not None and exp[i][1] < 0) for i in range(n)]
    assert 0 < sum(unrouted) < n and unrouted[-3:] == [1, 0, 0]
    tt = eng.torch
    skip = tt.empty(n, dtype=tt.uint8, device=eng.dev)
    vins = [eng.json_in_view(ji, v) for ji, v in zip(p.ins, b["views"])]
    for ins in (p.ins, vins):       # the launch's descriptors or the views: the same lines are result-bearing
        for repeat, drop in ((None, False), (None, True), (rep, False), (rep, True)):
            skip.fill_(9)
            eng.route_skip(ins, n, b["route"], skip, repeat=None if repeat is None else tt.from_numpy(repeat).to(eng.dev),
                           drop_unrouted=drop)
            assert skip.cpu().numpy().tolist() == [int((repeat is not None and repeat[i] != 0) or (drop and unrouted[i]))
                                                   for i in range(n)]


def test_entries_refuse_bad_arguments(eng, tables):
    from pysignalduino_amd import runtime
    t = eng.torch
    p = Plant(eng, [[(0, [b"x"])], [(1, [b"x"])]])
    dt = eng.route_table(tables("one"))
    b = eng.alloc_routes(4, pick=True, views=2)
    with pytest.raises(RuntimeError, match="given twice"):
        eng.route_records(dt, [p.ins[0], p.ins[0]], 2, b["route"], b["pick"], b["views"])
    with pytest.raises(RuntimeError, match="chunk's n"):
        eng.route_records(dt, p.ins, 1, b["route"], b["pick"], b["views"])
    with pytest.raises(ValueError):
        eng.route_records(dt, p.ins, 2, b["route"], b["pick"][:1], b["views"])
    with pytest.raises(ValueError):
        eng.route_records(dt, p.ins, 2, b["route"], b["pick"], b["views"][:1])
    with pytest.raises(ValueError):
        eng.route_skip(p.ins, 2, b["route"], b["skip"][:1])
    lib, ptr = eng.lib, runtime._ptr
    arr = (runtime.SdxJsonIn * 2)(*p.ins)
    for x in [b["route"], b["mask"], b["pick"], b["skip"]] + b["views"]:
        x.view(t.uint8).fill_(9)
    t.cuda.synchronize()
    views = lambda a, c: (ctypes.c_void_p * 2)(a, c)    # noqa: E731
    V = views(ptr(b["views"][0]), ptr(b["views"][1]))

    def rec(table=dt.handle, n=2, route=ptr(b["route"]), mask=ptr(b["mask"]), pick=ptr(b["pick"]), view=V, kinds=arr, k=2):
        return lib.sdx_route_records(eng.handle, table, kinds, k, n, route, mask, pick, view, eng.stream_ptr())
    refused = [rec(table=None), rec(route=None), rec(pick=None), rec(view=None), rec(n=-1), rec(kinds=None), rec(k=0), rec(k=5),
               rec(route=ptr(b["route"]) + 1), rec(pick=ptr(b["pick"]) + 1), rec(mask=ptr(b["mask"]) + 4),
               rec(view=views(ptr(b["views"][0]), None)), rec(view=views(ptr(b["views"][0]) + 2, ptr(b["views"][1])))]
    assert refused == [-1] * len(refused)

    def skp(n=2, route=ptr(b["route"]), skip=ptr(b["skip"]), kinds=arr, k=2):
        return lib.sdx_route_skip(kinds, k, n, route, None, 1, skip, eng.stream_ptr())
    refused = [skp(route=None), skp(skip=None), skp(n=-1), skp(kinds=None), skp(k=0), skp(route=ptr(b["route"]) + 1)]
    assert refused == [-1] * len(refused)
    t.cuda.synchronize()
    for x in [b["route"], b["mask"], b["pick"], b["skip"]] + b["views"]:      # nothing was launched: the 9s stand
        assert bool((x.view(t.uint8) == 9).all())
    assert rec() == 0 and skp() == 0
    t.cuda.synchronize()
    assert b["pick"][:2].cpu().numpy().tolist() == [0, 0]


# ---- front end and stream: the goldens ----------------------------------------------------------------
@pytest.fixture(scope="module")
def gold_any(golden):
    """lines_golden.json.gz -> per line the recorded message list, and by the definition over DEFAULT_ROUTES its
    (pick, route, mask), its key and its published text."""
    from pysignalduino_amd.routes import DEFAULT_ROUTES
    pats = [p for _, p in DEFAULT_ROUTES]
    cases = golden("lines_golden.json.gz")
    e2e = [c.get("e2e", []) for c in cases]
    res = [restate_pick(pats, [m[1] for m in e]) for e in e2e]
    keys = [TR.e2e_key(e[r[0]: r[0] + 1]) for e, r in zip(e2e, res)]
    texts = [J.published(e[r[0]: r[0] + 1]) for e, r in zip(e2e, res)]
    return res, keys, texts


def published_any(res, keys, texts, drop, collapse=False):
    rep = TR.repeats_of(keys) if collapse else [0] * len(keys)
    return [None if k is None or m or (drop and r[1] < 0) else (r[1], t) for r, k, t, m in zip(res, keys, texts, rep)]


def test_parse_lines_routed_any_goldens(gold, gold_any):
    from pysignalduino_amd.frontend import SignalParser
    from pysignalduino_amd.routes import DEFAULT_ROUTES, RouteTable
    lines, keys0, texts0 = gold
    res, keys, texts = gold_any
    table = RouteTable(DEFAULT_ROUTES)
    sp = SignalParser()
    got = sp.parse_lines_routed(lines, DEFAULT_ROUTES, route_match="any")
    rows = TR.kept_rows(got, keys)
    exp = published_any(res, keys, texts, drop=False)
    bad = [(i, lines[i][:60], got[i], exp[i]) for i in rows if got[i] != exp[i]]
    assert not bad, (len(bad), bad[:3])
    later = [i for i in rows if res[i][0] > 0]
    assert len(later) >= 50
    assert [int(sp.last_routes[i]) for i in rows] == [res[i][1] for i in rows]
    assert sp.last_picks.dtype == np.uint16 and [int(sp.last_picks[i]) for i in rows] == [res[i][0] for i in rows]
    # drop_unrouted publishes the lines a later message routes.  The same call on fewer lines (a line's answer does
    # not depend on its neighbours without collapse_repeats): every line with a later pick, and every eighth other
    sub = sorted(set(later) | set(rows[::8]))
    sub_lines = [lines[i] for i in sub]
    dropped = sp.parse_lines_routed(sub_lines, table, drop_unrouted=True, route_match="any")
    exp = published_any(res, keys, texts, drop=True)
    assert dropped == [exp[i] for i in sub]
    assert all(d is not None and d[0] >= 0 for d, i in zip(dropped, sub) if res[i][0] > 0)
    assert [int(x) for x in sp.last_picks] == [res[i][0] for i in sub]
    # "first" gives today's output for the same call, and names no pick
    first = sp.parse_lines_routed(sub_lines, table, drop_unrouted=True, route_match="first")
    assert sp.last_picks is None
    exp0 = TR.published(table.patterns, keys0, texts0, drop=True)
    assert first == [exp0[i] for i in sub]
    assert all(f is None for f, i in zip(first, sub) if res[i][0] > 0)
    assert sp.parse_lines_routed([], table, route_match="any") == [] and len(sp.last_picks) == 0


@pytest.mark.parametrize("output", ["json", "wire"])
def test_stream_chunk_any_goldens(gold, gold_any, output):
    from pysignalduino_amd.frontend import SignalParser
    from pysignalduino_amd.packing import ContractError
    from pysignalduino_amd.routes import DEFAULT_ROUTES, RouteTable
    lines, keys0, _ = gold
    res, keys, texts = gold_any
    table = RouteTable(DEFAULT_ROUTES)
    sp = SignalParser()
    n = len(lines)

    def one_chunk(**kw):
        ls = sp.stream(chunk_lines=n, chunk_bytes=max(1 << 21, 2 * sum(map(len, lines))), output=output, lag=1, **kw)
        ls.submit(lines)
        (r,) = ls.drain()
        return ls, r
    ls1, base = one_chunk(routes=table, route_match="first")
    assert base.pick is None
    ls2, r = one_chunk(routes=table, route_match="any")
    assert r.pick.dtype == np.uint16 and len(r.pick) == n and r.route.dtype == np.int16
    if output == "json":
        got = [None] * n
        for i, route, x in r.items_routed():
            got[i] = (route, x) if isinstance(x, str) else x
        rows = TR.kept_rows(got, keys)
        exp = published_any(res, keys, texts, drop=False)
        assert [got[i] for i in rows] == [exp[i] for i in rows]
        # the picks, 2 bytes per line, and nothing else travel beside the "first" run's results.  The text buffer
        # itself holds other texts (the picked messages'), so its own size, rounded to 4 as it is copied, is set aside
        pad = lambda rr: (len(rr.json) + 3) & ~3       # noqa: E731
        assert ls2.d2h_bytes - pad(r) == ls1.d2h_bytes - pad(base) + 2 * n
        ls3, rd = one_chunk(routes=DEFAULT_ROUTES, drop_unrouted=True, route_match="any")
        got = [None] * n
        for i, route, x in rd.items_routed():
            got[i] = (route, x) if isinstance(x, str) else x
        exp = published_any(res, keys, texts, drop=True)
        assert [got[i] for i in rows] == [exp[i] for i in rows]
        assert rd.route.tolist() == r.route.tolist() and rd.pick.tolist() == r.pick.tolist()
        assert ls3.d2h_bytes < ls2.d2h_bytes                    # the unrouted texts were never built
    else:
        rows = [i for i in range(n) if i not in r.host or not isinstance(r.host[i], ContractError)]
        assert n - len(rows) <= 0.05 * n
        assert [(int(r.pick[i]), int(r.route[i])) for i in rows] == [res[i][:2] for i in rows]
        assert r.layout[2] == base.layout[2] and bytes(r.wire) == bytes(base.wire)      # the sections are unchanged
        assert ls2.d2h_bytes == ls1.d2h_bytes + 2 * n
    assert sum(int(r.pick[i]) > 0 for i in rows) >= 50


@pytest.mark.parametrize("drop", [False, True])
def test_any_with_collapse_and_host_rows(repeated, golden, drop):
    """The ``repeated`` corpus of test_routes.py in chunks of 257 lines with collapse_repeats and route_match="any":
    the mask is repeats_of over the picked messages' keys; published = result, no repeat, routed or not drop."""
    from pysignalduino_amd.frontend import SignalParser
    from pysignalduino_amd.routes import DEFAULT_ROUTES, RouteTable
    lines, _, _ = repeated
    table = RouteTable(DEFAULT_ROUTES)
    by_line = {c["line"].strip("\n"): c.get("e2e", []) for name in ("lines_golden.json.gz", "lines_general_golden.json.gz")
               for c in golden(name)}
    e2e = [by_line[ln] for ln in lines]
    res = [restate_pick(table.patterns, [m[1] for m in e]) for e in e2e]
    keys = [TR.e2e_key(e[r[0]: r[0] + 1]) for e, r in zip(e2e, res)]
    texts = [J.published(e[r[0]: r[0] + 1]) for e, r in zip(e2e, res)]
    exp = published_any(res, keys, texts, drop, collapse=True)
    mask = TR.repeats_of(keys)
    assert len(lines) > 2 * 257 and sum(mask) > 100 and sum(r[0] > 0 for r in res) >= 10
    sp = SignalParser()
    ls = sp.stream(chunk_lines=257, chunk_bytes=1 << 19, output="json", lag=2, collapse_repeats=True, routes=table,
                   drop_unrouted=drop, route_match="any")
    for a in range(0, len(lines), 257):
        ls.submit(lines[a: a + 257])
    got, gmask, picks, host_rows = [], [], [], 0
    for r in ls.drain():
        chunk = [None] * r.n
        for i, route, x in r.items_routed():
            chunk[i] = (route, x)
        got += chunk
        gmask += r.repeat.tolist()
        picks += r.pick.tolist()
        host_rows += len(r.host)
    assert host_rows >= 5
    assert gmask == mask
    assert got == exp
    assert picks == [r[0] for r in res]
    assert sp.parse_lines_routed(lines, table, drop_unrouted=drop, collapse_repeats=True, route_match="any") == exp
    assert sp.last_repeat_mask.tolist() == mask and sp.last_picks.tolist() == [r[0] for r in res]
