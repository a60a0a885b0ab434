"""The json_all stream on the CPU: ChunkResult.texts_all / items_all / detach on hand-built arrays,
LineStream's json_all stage code on test_stream_host.py's stand-ins (a scripted engine that writes record-indexed
texts the way sdx_index_records + sdx_serialize_json_lines do), and the argument validation of LineStream and
BatchingParserTask.  The device work itself is tests/test_line_index.py's and tests/test_stream_all.py's business."""
import inspect
import json
import types

import numpy as np
import pytest

from pysignalduino_amd import runtime, stream
from pysignalduino_amd.packing import ContractError

from test_stream_host import FT, FakeEngine, FakeParser, FakeProtocols, KIND_OF, stubbed  # noqa: F401  (fixture)

KN = {runtime.LINE_MU: "MU", runtime.LINE_MS: "MS", runtime.LINE_MC: "MC", runtime.LINE_MN: "MN"}


# ---- ChunkResult on hand-built arrays --------------------------------------------------------------------------------
def hand_chunk():
    """5 lines; records: line 0 -> 0, 1 (the second of length 0), line 2 -> 2, 3, 4 (the last of length 0), line 4 -> 5."""
    texts = [b"aaa", b"", b"bbbb", b"cc", b"", b"d"]
    blob = b"".join(texts)
    buf = np.frombuffer(blob, np.uint8).copy()
    off = np.cumsum([0] + [len(x) for x in texts[:-1]]).astype(np.uint32)
    ln = np.array([len(x) for x in texts], np.uint32)
    r = stream.ChunkResult(7, 5, np.zeros(5, np.uint8), np.zeros(5, np.uint8))
    r.json, r.off, r.len = memoryview(buf), off, ln
    r.first = np.array([0, 2, 2, 5, 5, 6], np.uint32)
    return r, buf


def test_chunk_result_texts_all():
    r, _ = hand_chunk()
    assert r.texts_all() == [["aaa"], [], ["bbbb", "cc"], [], ["d"]]          # a record of length 0 is no text
    assert r.items_all() == [(0, ["aaa"]), (2, ["bbbb", "cc"]), (4, ["d"])]
    with pytest.raises(ValueError):
        r.texts()
    with pytest.raises(ValueError):
        r.items()
    err = ContractError("outside the contract")
    r.host = {1: ["h1", "h2"], 2: [], 3: err}                                 # a list, [] over device texts, an exception
    assert r.texts_all() == [["aaa"], ["h1", "h2"], [], err, ["d"]]
    assert r.items_all() == [(0, ["aaa"]), (1, ["h1", "h2"]), (3, err), (4, ["d"])]
    r.len[:] = 0
    r.host = {}
    assert r.texts_all() == [[], [], [], [], []] and r.items_all() == []


def test_chunk_result_without_records_and_plain_chunks():
    r = stream.ChunkResult(0, 3, np.zeros(3, np.uint8), np.zeros(3, np.uint8))
    r.json, r.off, r.len = memoryview(np.zeros(0, np.uint8)), np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    r.first = np.zeros(4, np.uint32)
    assert r.texts_all() == [[], [], []]
    r.host = {2: ["x"]}
    assert r.items_all() == [(2, ["x"])]
    plain = stream.ChunkResult(0, 1, np.zeros(1, np.uint8), np.zeros(1, np.uint8))
    plain.json, plain.off, plain.len = memoryview(np.frombuffer(b"t", np.uint8)), np.zeros(1, np.uint32), np.ones(1, np.uint32)
    assert plain.texts() == ["t"]
    with pytest.raises(ValueError):
        plain.texts_all()
    with pytest.raises(ValueError):
        plain.items_all()


def test_chunk_result_detach_copies_the_new_arrays():
    r, buf = hand_chunk()
    first, off, ln = r.first, r.off, r.len
    r.slot = object()
    want = r.texts_all()
    assert r.detach() is r and r.slot is None
    assert r.first is not first and r.off is not off and r.len is not ln and isinstance(r.json, bytes)
    buf[:] = ord("X")
    first[:], off[:], ln[:] = 0, 0, 0
    assert r.texts_all() == want


# ---- the stage code on scripted stand-ins ------------------------------------------------------------------------------
def texts_of_line(ln: bytes):
    """The scripted decode: b"MU;D=AB;N=3;" -> three texts with payloads AB, AB#1, AB#2 (N defaults to 1)."""
    f = dict(x.split(b"=", 1) for x in ln.split(b";") if b"=" in x)
    if ln[:2] not in KIND_OF or b"D" not in f:
        return []
    p = f[b"D"].decode()
    return [json.dumps({"protocol_id": "1", "payload": p if j == 0 else f"{p}#{j}"}) for j in range(int(f.get(b"N", b"1")))]


class AllEngine(FakeEngine):
    """FakeEngine + the json_all surface: index_records counts the records of the scripted parse's OK lines,
    launch_json_lines writes one text per record at first[line] + j, mark_repeats marks a device line whose (kind,
    payload) equals the previous DEVICE line's -- it does not see the lines the batch API resolves."""

    def __init__(self):
        super().__init__()
        self.dev_last = None
        self.force_ovf = False

    @staticmethod
    def json_in(kind, demod_out, lines_out, n, first_only=True):
        return types.SimpleNamespace(kind=kind, lb=lines_out["meta"].owner, n=n, first_only=first_only)

    @staticmethod
    def _device_lines(lb, n):
        for i in range(n):
            if lb.status.a[i] == runtime.LS_OK and lb.kind.a[i] in KN:
                yield i, lb.bytes.a[lb.offsets.a[i]: lb.offsets.a[i + 1]].tobytes()

    def alloc_line_index(self, n, rec_max, json_cap=None):
        idx = self.alloc_json(rec_max, json_cap)
        idx.update(first=FT(np.zeros(n + 1, np.int32)), scratch=FT(np.zeros(16, np.uint8)), rec_max=rec_max, n=n)
        return idx

    def alloc_dispatch(self, n, outs):
        return {"outs": [dict(o) for o in outs], "scratch": FT(np.zeros(16, np.uint8))}

    def dispatch_records(self, rules, json_ins, n, bufs, stream=None, rec_caps=None):
        assert isinstance(rules, runtime.SdxDispatchRules)
        self.calls.append(("dispatch", len(json_ins), n))
        return bufs["outs"]

    def alloc_repeat(self, n):
        return FT(np.zeros(max(n, 1), np.uint8)), FT(np.zeros(16, np.uint8))

    def alloc_repeat_state(self, timed=False, sources=None):
        return FT(np.zeros(16 + 240, np.uint8))     # never valid: the tracker follows the keys itself

    def mark_repeats(self, json_ins, n, repeat, scratch, state, stream=None):
        self.calls.append(("mark", n))
        repeat.a[:n] = 0
        for i, ln in self._device_lines(json_ins[0].lb, n):
            tx = texts_of_line(ln)
            if tx:
                key = (int(json_ins[0].lb.kind.a[i]), json.loads(tx[0])["payload"])
                repeat.a[i] = 1 if key == self.dev_last else 0
                self.dev_last = key

    def index_records(self, json_ins, n, idx, skip=None, stream=None):
        self.calls.append(("index", len(json_ins), n, skip is not None))
        assert all(j.first_only == 0 for j in json_ins)
        cnt = np.zeros(n, np.int64)
        for i, ln in self._device_lines(json_ins[0].lb, n):
            if skip is None or not skip.a[i]:
                cnt[i] = len(texts_of_line(ln))
        idx["first"].a[: n + 1] = np.concatenate([[0], np.cumsum(cnt)])

    def launch_json_lines(self, kind, demod_out, lines_out, n, idx):
        self.calls.append(("json_lines", kind))
        lb, first = lines_out["meta"].owner, idx["first"].a
        want = {v: k for k, v in KN.items()}[self.KN[kind]]
        for i, ln in self._device_lines(lb, n):
            if lb.kind.a[i] != want:
                continue
            for j, txt in enumerate(texts_of_line(ln)[: int(first[i + 1] - first[i])]):
                b, c = txt.encode(), int(idx["cursor"].a[0])
                idx["json"].a[c: c + len(b)] = np.frombuffer(b, np.uint8)
                idx["off"].a[first[i] + j], idx["len"].a[first[i] + j] = c, len(b)
                idx["cursor"].a[0] = c + len(b)
        if self.force_ovf:
            idx["cursor"].a[1] = 1


class AllParser(FakeParser):
    def __init__(self, eng):
        super().__init__(eng)
        self.protocols._bank = types.SimpleNamespace(mn_pids=["100"], mu_pids=["1"], ms_pids=[], mc_pids=[], protocols={"1": {}},
                                                     affixes=lambda kd: None)
        self.all_calls = []

    def parse_lines_json_all(self, lines, dispatch=None, **kw):
        self.all_calls.append((len(lines), dispatch, kw))
        return [texts_of_line(bytes(x)) for x in lines]


@pytest.fixture
def all_eng(stubbed, monkeypatch):   # noqa: F811
    eng = AllEngine()
    return eng


def _lines(n, seed):
    rng = np.random.default_rng(seed)
    kinds = [b"MU", b"MS", b"MC", b"MN", b"XX"]
    out = []
    for i in range(n):
        k = kinds[int(rng.integers(0, len(kinds)))]
        out.append(k + b";D=%d;N=%d;" % (i, int(rng.integers(0, 5))) + (b"GEN;" if rng.random() < 0.05 else b""))
    return out


@pytest.mark.parametrize("rules", [None, True])
def test_stream_state_machine_json_all(all_eng, rules):
    """Chunks of random sizes with polls in between, then a drain: every chunk once, in order, every line with the
    list of its own texts -- the batch API's list for the lines the device hands back --, the chunk's launches the
    index pass and one launch_json_lines per kind with lines, the dispatch pass exactly when there are rules."""
    eng = all_eng
    parser = AllParser(eng)
    ls = stream.LineStream(parser, chunk_lines=3000, chunk_bytes=3000 * 40, output="json_all", lag=2, rules=rules)
    chunks, got = [], []
    for j, n in enumerate((700, 0, 3000, 1, 1234)):
        ch = _lines(n, seed=j)
        chunks.append(ch)
        assert ls.submit(ch) == j
        if j % 2:
            got += [r.detach() for r in ls.poll()]
    got += [r.detach() for r in ls.drain()]
    assert [r.id for r in got] == list(range(len(chunks))) and not ls.inflight
    for ch, r in zip(chunks, got):
        assert r.n == len(ch) and len(r.first) == len(ch) + 1
        assert r.texts_all() == [texts_of_line(x) for x in ch]
        gen = [i for i, ln in enumerate(ch) if b"GEN" in ln]
        assert sorted(r.host) == gen
        assert r.items_all() == [(i, texts_of_line(x)) for i, x in enumerate(ch) if texts_of_line(x)]
    assert all(c[1] is (ls.rules if rules else None) for c in parser.all_calls) and parser.all_calls
    assert sum(c[0] == "index" for c in eng.calls) == len(chunks)
    assert sum(c[0] == "dispatch" for c in eng.calls) == (len(chunks) if rules else 0)
    assert any(c[0] == "json_lines" for c in eng.calls) and not any(c[0] == "json" for c in eng.calls)


def test_json_and_wire_streams_launch_and_allocate_what_they_did(all_eng):
    eng = all_eng
    for output in ("json", "wire"):
        ls = stream.LineStream(AllParser(eng), chunk_lines=500, chunk_bytes=500 * 40, output=output, lag=1)
        ls.submit([b"MU;D=1;", b"MC;D=2;"])
        ls.drain()
        assert not any(hasattr(s, f) for s in ls.slots for f in ("idx", "dp", "douts", "rec_max"))
    assert not any(c[0] in ("index", "json_lines", "dispatch", "mark") for c in eng.calls)


def test_overflow_flag_resolves_every_line_through_the_host(all_eng):
    eng = all_eng
    eng.force_ovf = True
    parser = AllParser(eng)
    ls = stream.LineStream(parser, chunk_lines=100, chunk_bytes=4000, output="json_all", lag=1)
    ch = [b"MU;D=A;N=2;", b"XX;D=B;", b"MS;D=C;", b"MN;D=E;N=3;", b"MC;D=F;N=0;"]
    ls.submit(ch)
    r = ls.drain()[0]
    assert sorted(r.host) == [0, 2, 3, 4]                       # every line a launch took; XX went to no launch
    assert parser.all_calls[0][0] == 4
    assert r.texts_all() == [texts_of_line(x) for x in ch]


def test_fix_repeats_around_a_host_resolved_line(all_eng):
    """The device does not see the line the batch API resolves: it marks line 2 as a repeat of line 0 although BB
    stands between them (republished from the host), and cannot mark host line 3, a repeat of line 2 (dropped)."""
    eng = all_eng
    parser = AllParser(eng)
    ls = stream.LineStream(parser, chunk_lines=100, chunk_bytes=4000, output="json_all", lag=1, collapse_repeats=True, rules=True)
    ch = [b"MU;D=AA;N=2;", b"MU;D=BB;GEN;", b"MU;D=AA;N=2;", b"MU;D=AA;GEN;", b"MU;D=CC;N=3;", b"MU;D=CC;", b"MU;D=CC;N=2;"]
    ls.submit(ch)
    r = ls.drain()[0]
    assert r.repeat.tolist() == [0, 0, 0, 1, 0, 1, 1]
    t = [texts_of_line(x) for x in ch]
    assert r.texts_all() == [t[0], t[1], t[2], [], t[4], [], []]
    assert r.host[2] == t[2] and r.host[3] == []
    assert np.diff(r.first.astype(np.int64)).tolist() == [2, 0, 0, 0, 3, 0, 0]     # the device skipped 2, 5 and 6
    assert [c for c in eng.calls if c[0] == "index"] == [("index", 4, 7, True)]
    # the next chunk's first line repeats the carried key; then a device line the host must drop
    ch2 = [b"MU;D=CC;", b"MU;D=DD;GEN;", b"MU;D=DD;N=2;"]
    ls.submit(ch2)
    r2 = ls.drain()[0]
    assert r2.repeat.tolist() == [1, 0, 1]
    assert r2.texts_all() == [[], texts_of_line(ch2[1]), []]
    assert r2.len[int(r2.first[2]): int(r2.first[3])].tolist() == [0, 0]           # its record range, zeroed


# ---- argument validation ---------------------------------------------------------------------------------------------
def test_line_stream_arguments(all_eng):
    p = AllParser(all_eng)
    mk = lambda **kw: stream.LineStream(p, chunk_lines=10, chunk_bytes=400, lag=1, **kw)   # noqa: E731
    for kw in (dict(output="json", rules=True), dict(output="wire", rules=True), dict(rules=True),
               dict(output="json_all", routes=[("a", "^A")]), dict(output="json_all", drop_unrouted=True),
               dict(output="json_all", route_match="any"), dict(output="json_all", rules="yes"),
               dict(output="json_all", rules=1), dict(output="text")):
        with pytest.raises(ValueError):
            mk(**kw)
    from pysignalduino_amd.dispatch import DispatchRules
    assert mk(output="json_all").rules is None
    assert isinstance(mk(output="json_all", rules=True).rules, DispatchRules)
    rl = DispatchRules(max_repeat=1, keep_equal=())
    assert mk(output="json_all", rules=rl).rules is rl
    with pytest.raises(ValueError):
        mk(output="json_all", rules=DispatchRules(keep_equal=["no such id"]))      # compiled against the bank at once


def test_signal_parser_stream_takes_rules_not_dispatch():
    from pysignalduino_amd.frontend import SignalParser
    params = inspect.signature(SignalParser.stream).parameters
    assert "rules" in params and "dispatch" not in params
    assert not any(p.kind is inspect.Parameter.VAR_KEYWORD for p in params.values())   # stream(dispatch=True): TypeError


def test_batching_parser_task_arguments():
    from pysignalduino_amd.controller import BatchingParserTask
    from pysignalduino_amd.dispatch import DispatchRules
    ctrl = types.SimpleNamespace(message_callback=None)
    for kw in (dict(publish="json", rules=True), dict(publish="objects", rules=True), dict(rules=True),
               dict(publish="json_all", routes=[("a", "^A")]), dict(publish="json_all", rules="yes"), dict(publish="xml")):
        with pytest.raises(ValueError):
            BatchingParserTask(ctrl, **kw)
    with pytest.raises(ValueError):
        BatchingParserTask(types.SimpleNamespace(message_callback=print), publish="json_all")
    t = BatchingParserTask(ctrl, publish="json_all", rules=True)
    assert t.all and t.use_stream and isinstance(t.rules, DispatchRules)
    t = BatchingParserTask(ctrl, publish="json_all", stream=False)
    assert t.all and not t.use_stream and t.rules is None
    assert not BatchingParserTask(ctrl, publish="json").all
