"""Receiver profiles end to end: the recorded lines of the goldens from four receivers with four
profiles through the front end, the stream and the controller task.

Expected values: the reference-recorded "e2e" message lists of tests/golden/lines_golden.json.gz filtered by the
definition restated in test_profiles_host.py, and the reference's publication (oracle/json_oracle.py) of the first
message that is left.  Nothing expected is taken from the code under test."""
import asyncio
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import json_oracle as J
from oracle import sd_oracle as O

import test_routes as TR
from test_lines import _flat_msgs
from test_profiles_host import restate_filter
from test_route_records_host import restate_pick

pytestmark = pytest.mark.gpu

KINDS = ("MU", "MS", "MC", "MN")
BLACK = ["61", "15", "1", "40", "113"]


@pytest.fixture(scope="module")
def setup(golden):
    """lines, sources (g % 4), the four profiles as keyword dictionaries and as Profile objects, and per line the
    filtered message list, its published text and its key."""
    from pysignalduino_amd.profiles import Profile, ReceiverProfiles
    cases = golden("lines_golden.json.gz")
    P = O.OracleBank().p
    e2e = [c.get("e2e", []) for c in cases]
    ids = sorted({m[0] for e in e2e for m in e}, key=float)
    kws = [dict(whitelist=ids[::2]), dict(blacklist=BLACK), dict(skip_development=True), dict()]
    src = np.arange(len(cases), dtype=np.int32) % 4
    filt = [restate_filter(P, KINDS.index(e[0][3][1]), e, **kws[int(s)]) if e else [] for e, s in zip(e2e, src)]
    # the preconditions: the profiles do change this corpus (computed from the recorded lists: 316, 179, 60)
    changed = sum(f != e for f, e in zip(filt, e2e))
    emptied = sum(bool(e) and not f for f, e in zip(filt, e2e))
    new_first = sum(bool(f) and f[0] != e[0] for f, e in zip(filt, e2e))
    assert changed >= 200 and emptied >= 100 and new_first >= 40, (changed, emptied, new_first)
    rp = ReceiverProfiles([Profile(**kw) for kw in kws], [0, 1, 2, 3])
    return SimpleNamespace(lines=[c["line"] for c in cases], src=src, kws=kws, rp=rp, e2e=e2e, filt=filt, P=P,
                           texts=[J.published(f) for f in filt], keys=[TR.e2e_key(f) for f in filt])


@pytest.fixture(scope="module")
def sp():
    from pysignalduino_amd.frontend import SignalParser
    return SignalParser()


def test_parse_lines_objects(setup, sp):
    s = setup
    got = sp.parse_lines(s.lines, sources=s.src, profiles=s.rp)
    rows = TR.kept_rows(got, s.keys)
    bad = [(i, s.lines[i][:60], s.filt[i][:2], _flat_msgs(got[i])[:2]) for i in rows if _flat_msgs(got[i]) != s.filt[i]]
    assert not bad, (len(bad), bad[:3])
    assert sum(len(got[i]) for i in rows) < sum(len(s.e2e[i]) for i in rows)


def test_parse_lines_json_and_unchanged_defaults(setup, sp):
    from pysignalduino_amd.profiles import Profile, ReceiverProfiles
    s = setup
    got = sp.parse_lines_json(s.lines, sources=s.src, profiles=s.rp)
    rows = TR.kept_rows(got, s.keys)
    bad = [(i, s.lines[i][:60], got[i], s.texts[i]) for i in rows if got[i] != s.texts[i]]
    assert not bad, (len(bad), bad[:3])
    # the defaults: no profiles, and one profile that enables everything, give the reference's decoded[0]
    plain = sp.parse_lines_json(s.lines)
    every = sp.parse_lines_json(s.lines, profiles=ReceiverProfiles([Profile()]))
    assert [plain[i] for i in rows] == [J.published(s.e2e[i]) for i in rows]
    assert [(x if isinstance(x, (str, type(None))) else repr(x)) for x in every] == \
           [(x if isinstance(x, (str, type(None))) else repr(x)) for x in plain]
    objs = sp.parse_lines(s.lines, profiles=Profile())
    assert all(_flat_msgs(objs[i]) == s.e2e[i] for i in rows)
    # arguments: several receivers' profiles need ids; ids must lie inside the table
    with pytest.raises(ValueError):
        sp.parse_lines_json(s.lines[:8], profiles=s.rp)
    with pytest.raises(ValueError):
        sp.parse_lines(s.lines[:8], sources=[0, 1, 2, 3, 4, 0, 0, 0], profiles=s.rp)
    with pytest.raises(ValueError):
        sp.parse_lines_json(s.lines[:4], sources=[0, 0, 0, 0])          # without collapse_repeats or profiles
    with pytest.raises(ValueError):
        sp.parse_lines_json(s.lines[:4], profiles=Profile(whitelist=["nope"]))


def routed_expectation(s, table, drop=False):
    res = [restate_pick(table.patterns, [m[1] for m in f]) for f in s.filt]
    exp = [None if not f or (drop and r[1] < 0) else (r[1], J.published(f[r[0]: r[0] + 1])) for f, r in zip(s.filt, res)]
    return res, exp


def test_parse_lines_routed_any(setup, sp):
    from pysignalduino_amd.routes import DEFAULT_ROUTES, RouteTable
    s = setup
    table = RouteTable(DEFAULT_ROUTES)
    res, exp = routed_expectation(s, table)
    got = sp.parse_lines_routed(s.lines, table, route_match="any", sources=s.src, profiles=s.rp)
    rows = TR.kept_rows(got, s.keys)
    bad = [(i, s.lines[i][:60], got[i], exp[i]) for i in rows if got[i] != exp[i]]
    assert not bad, (len(bad), bad[:3])
    assert [int(sp.last_picks[i]) for i in rows] == [res[i][0] for i in rows]     # the picks index the filtered lists
    assert sum(res[i][0] > 0 for i in rows) >= 5


@pytest.mark.parametrize("chunk", [100, 1500])
def test_stream_submit_forms(setup, sp, chunk):
    from pysignalduino_amd.frontend import pack_lines
    s = setup
    n = len(s.lines)
    cuts = list(range(0, n, chunk)) + [n]
    big = max(1 << 20, 4 * max(sum(len(x) for x in s.lines[a:b]) for a, b in zip(cuts, cuts[1:])))

    def texts_of(ls, results):
        out = []
        for r in results:
            assert r.source is not None and len(r.source) == r.n
            out += r.texts()
        return out

    ls = sp.stream(chunk_lines=chunk, chunk_bytes=big, lag=2, profiles=s.rp)
    for a, b in zip(cuts, cuts[1:]):
        ls.submit(s.lines[a:b], sources=s.src[a:b])
    got = texts_of(ls, ls.drain())
    rows = TR.kept_rows(got, s.keys)
    bad = [(i, got[i], s.texts[i]) for i in rows if got[i] != s.texts[i]]
    assert not bad, (len(bad), bad[:3])

    ls = sp.stream(chunk_lines=chunk, chunk_bytes=big, lag=2, profiles=s.rp)
    for a, b in zip(cuts, cuts[1:]):
        data, offsets, bad_lines = pack_lines(s.lines[a:b])
        ls.submit_packed(data, offsets, lines=s.lines[a:b], bad=bad_lines, sources=s.src[a:b])
    got2 = texts_of(ls, ls.drain())
    assert [got2[i] for i in rows] == [s.texts[i] for i in rows]

    # submit_bytes: one read buffer per receiver, cut into chunks by the stream; the lines that are one
    # newline-terminated line each
    one = [i for i in rows if s.lines[i].endswith("\n") and s.lines[i].count("\n") == 1]
    assert len(one) > 3000
    ls = sp.stream(chunk_lines=chunk, chunk_bytes=big, lag=2, profiles=s.rp)
    order = []
    for sid in range(4):
        mine = [i for i in one if s.src[i] == sid]
        order += mine
        ls.submit_bytes("".join(s.lines[i] for i in mine).encode("latin-1"), source=sid)
    res = ls.drain()
    got3 = texts_of(ls, res)
    assert np.concatenate([r.source for r in res]).tolist() == [int(s.src[i]) for i in order]
    assert got3 == [s.texts[i] for i in order]


def test_stream_arguments(setup, sp):
    from pysignalduino_amd.profiles import Profile
    s = setup
    with pytest.raises(ValueError):
        sp.stream(chunk_lines=64, output="wire", profiles=s.rp)
    with pytest.raises(ValueError):
        sp.stream(chunk_lines=64, collapse_repeats=True, repeat_sources=3, profiles=s.rp)    # the table maps 4
    ls = sp.stream(chunk_lines=64, chunk_bytes=1 << 16, profiles=s.rp)
    with pytest.raises(ValueError):
        ls.submit(s.lines[:8])                                                             # no ids
    with pytest.raises(ValueError):
        ls.submit(s.lines[:8], sources=[0, 1, 2, 3, 4, 0, 1, 2])
    with pytest.raises(ValueError):
        ls.submit_bytes(b"MU;x\n")
    assert ls.drain() == []
    one = sp.stream(chunk_lines=64, chunk_bytes=1 << 16, profiles=Profile(blacklist=BLACK))    # one receiver: no ids needed
    one.submit(s.lines[:64])
    (r,) = one.drain()
    P = s.P
    exp = [J.published(restate_filter(P, KINDS.index(e[0][3][1]), e, blacklist=BLACK) if e else []) for e in s.e2e[:64]]
    rows = TR.kept_rows(r.texts(), s.keys[:64])
    assert [r.texts()[i] for i in rows] == [exp[i] for i in rows]


def test_repeats_per_source_on_the_filtered_lists(setup, sp):
    """Every result-bearing line twice in a row from its receiver: the repeat mask is repeats.py's host restatement
    run on the filtered lists -- a line whose first message a profile removes repeats by its NEW first message, and an
    emptied line neither starts nor breaks a run."""
    from pysignalduino_amd import repeats
    s = setup
    probe = sp.parse_lines_json(s.lines)
    from pysignalduino_amd.packing import ContractError
    pick = [i for i in range(len(s.lines)) if not isinstance(probe[i], ContractError)][:1500]
    idx = [i for i in pick for _ in range(2 if s.e2e[i] else 1)]
    lines, src = [s.lines[i] for i in idx], np.array([s.src[i] for i in idx], np.int32)

    def objs(lists):
        return [[SimpleNamespace(protocol_id=m[0], payload=m[1], raw=SimpleNamespace(message_type=m[3][1])) for m in f] for f in lists]

    exp_mask = repeats.collapse_objects(objs([s.filt[i] for i in idx]), sources=src).tolist()
    raw_mask = repeats.collapse_objects(objs([s.e2e[i] for i in idx]), sources=src).tolist()
    assert sum(exp_mask) > 300 and exp_mask != raw_mask
    exp = [None if m else s.texts[i] for i, m in zip(idx, exp_mask)]
    got = sp.parse_lines_json(lines, collapse_repeats=True, sources=src, profiles=s.rp)
    assert sp.last_repeat_mask.tolist() == exp_mask and got == exp
    ls = sp.stream(chunk_lines=400, chunk_bytes=1 << 21, lag=2, collapse_repeats=True, repeat_sources=4, profiles=s.rp)
    for a in range(0, len(lines), 400):
        ls.submit(lines[a: a + 400], sources=src[a: a + 400])
    res = ls.drain()
    assert np.concatenate([r.repeat for r in res]).tolist() == exp_mask
    assert [t for r in res for t in r.texts()] == exp


def test_batching_parser_task_publishes_the_filtered_messages(setup, sp):
    from pysignalduino_amd.controller import BatchingParserTask
    from pysignalduino_amd.packing import ContractError
    from pysignalduino_amd.profiles import Profile
    from test_controller import Ctl, _drive
    s = setup
    probe = sp.parse_lines_json(s.lines[:1200])
    lines = [ln for ln, g in zip(s.lines[:1200], probe) if not isinstance(g, ContractError) and ln]
    e2e = [e for e, g, ln in zip(s.e2e[:1200], probe, s.lines[:1200]) if not isinstance(g, ContractError) and ln]
    kw = s.kws[0]                                           # the whitelist, for the one receiver a controller reads
    exp = [J.published(restate_filter(s.P, KINDS.index(e[0][3][1]), e, **kw)) for e in e2e if e]
    exp = [t for t in exp if t is not None]
    for stream in (True, False):
        ctl = Ctl(sp, callback=False)
        task = BatchingParserTask(ctl, publish="json", max_batch=300, profiles=Profile(**kw), stream=stream)
        asyncio.run(_drive(ctl, task, lines, chunk=150))
        assert [t for _, t in ctl.mqtt_publisher.sent] == exp
    assert 0 < len(exp) < sum(bool(e) for e in e2e)
    with pytest.raises(ValueError):
        BatchingParserTask(Ctl(sp, callback=False), publish="json", profiles=s.rp)      # a controller reads one receiver


def test_mn_two_receivers_two_rfmodes(golden, sp):
    from pysignalduino_amd.profiles import Profile, ReceiverProfiles
    from test_mn import oracle_line
    obank = O.OracleBank()
    modes = ["Bresser_5in1", "Lacrosse_mode1"]
    cases = [c for c in golden("mn_golden.json.gz")["lines"] if c[0] in ("test", "synth") and c[2] is None][:1600]
    lines = [c[1] for c in cases]
    src = np.arange(len(lines), dtype=np.int32) % 2
    exp = [oracle_line(obank, ln.encode("latin-1"), modes[int(sid)]) for ln, sid in zip(lines, src)]
    full = [oracle_line(obank, ln.encode("latin-1"), None) for ln in lines]
    rp = ReceiverProfiles([Profile(rfmode=m) for m in modes], [0, 1])
    got = sp.parse_lines(lines, sources=src, profiles=rp)
    rows = [i for i, e in enumerate(exp) if isinstance(e, list) and not isinstance(got[i], Exception)]
    assert len(rows) > 0.95 * len(lines)
    bad = [(i, lines[i], exp[i], _flat_msgs(got[i])) for i in rows if _flat_msgs(got[i]) != exp[i]]
    assert not bad, (len(bad), bad[:2])
    assert all(sum(bool(exp[i]) for i in rows if src[i] == k) >= 10 for k in (0, 1))
    assert sum(bool(full[i]) and not exp[i] for i in rows) >= 100                    # what the other rfmodes decoded
    texts = sp.parse_lines_json(lines, sources=src, profiles=rp)
    assert [texts[i] for i in rows] == [J.published(exp[i]) for i in rows]
