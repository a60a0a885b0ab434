"""Repeat suppression, host side, on the CPU: the fix-up of the device's mask around
host-resolved lines (repeats.RepeatTracker), LineStream's ordering of the chunks' repeat passes and its
_collect against a scripted engine (the stand-ins of tests/test_stream_host.py, which now also script
sdx_mark_repeats), and the controller's per-line effects.  Expected values: ``restate``, the serial
restatement of the definition, over keys the tests choose themselves; the controller's effects are those
of the reference loop (signalduino/controller.py:245-264) with the definition applied."""
import asyncio
import json
import re
import sys

import numpy as np
import pytest

from pysignalduino_amd import controller as ctl
from pysignalduino_amd import frontend, repeats, runtime, stream

import test_stream_host as H

NAMES = ("MU", "MS", "MC", "MN")


def restate(keys):
    mask, prev = [], None
    for k in keys:
        if k is None:
            mask.append(0)
            continue
        mask.append(int(k == prev))
        prev = k
    return mask


# ---- the ABI ------------------------------------------------------------------------------------------
def test_abi_declares_the_repeat_entries():
    import os
    hdr = open(os.path.join(os.path.dirname(runtime.HERE), "include", "sdx.h")).read()
    for name in ("sdx_mark_repeats", "sdx_serialize_json_skip", "sdx_repeat_state_bytes", "sdx_repeat_scratch_bytes",
                 "sdx_repeat_tile"):
        assert name in runtime.EXPORTED and re.search(r"\b%s\(" % name, hdr), name
    assert "#define SDX_ABI_VERSION 14" in hdr and runtime.ABI_VERSION == 14
    lib = runtime.load_library()
    assert lib.sdx_abi_version() == 14
    T = lib.sdx_repeat_tile()
    assert lib.sdx_repeat_state_bytes() >= 16 + 65535 and lib.sdx_repeat_state_bytes() % 16 == 0
    for n in (1, T, T + 1, 250_000):
        tiles = -(-n // T)
        assert lib.sdx_repeat_scratch_bytes(n) >= 16 + 16 * n + 8 * tiles and lib.sdx_repeat_scratch_bytes(n) % 16 == 0


def test_layout_helpers_under_sanitizers(tmp_path):
    """tools/repeat_layout_check.cpp: the size / offset helpers sdx_mark_repeats shares with its callers,
    as a stand-alone host program built with -fsanitize=address,undefined."""
    import os
    import subprocess
    src = os.path.join(os.path.dirname(runtime.HERE), "tools", "repeat_layout_check.cpp")
    exe = str(tmp_path / "repeat_layout_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "repeat_layout_check: ok" in r.stdout, r.stderr[-2000:]


# ---- RepeatTracker: a simulated device that does not see the host rows ----------------------------------
def simulate(keys, host, redo, cuts, mode):
    """keys[i]: a line's key or None; host: rows resolved by the batch API; redo: those of them the device
    saw all the same; cuts: chunk boundaries.  The device's mask is what sdx_mark_repeats computes over the
    lines it sees, its state carried over the chunks.  -> (the tracker's mask, lines fetched)."""
    tr = repeats.RepeatTracker()
    dev_prev = None
    out, fetched = [], []
    for a, b in zip([0] + cuts, cuts + [len(keys)]):
        n = b - a
        rep = np.zeros(n, np.uint8)
        for i in range(a, b):
            if keys[i] is None or (i in host and i not in redo):
                continue
            rep[i - a] = int(keys[i] == dev_prev)
            dev_prev = keys[i]
        seen = np.array([keys[i] is not None and (i not in host or i in redo) for i in range(a, b)], bool)
        has_key = seen & (rep == 0) if mode == "json" else seen     # json: a flagged line has no text
        host_keys = {i - a: keys[i] for i in range(a, b) if i in host}

        def fetch(i, a=a):
            fetched.append(a + i)
            return keys[a + i]
        out += tr.fix_chunk(rep, has_key, lambda i, a=a: keys[a + i], host_keys, [i - a for i in redo if a <= i < b],
                            fetch).tolist()
    return out, fetched


@pytest.mark.parametrize("mode", ["json", "wire"])
def test_tracker_corrects_the_device_mask(mode):
    A, B_, G = ("MU", "1", "aa"), ("MU", "2", "bb"), ("MS", "7", "gg")
    N = None
    #        0  1  2  3  4   5   6  7  8  9  10 11 12 13 14 15 16 17
    keys = [A, A, G, A, A, B_, B_, G, A, N, G, G, N, G, A, G, N, A]
    host = {i for i, k in enumerate(keys) if k is G}
    exp = restate(keys)
    for cuts in ([], [3], [2], [8, 11], [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17], [10, 12, 13]):
        got, fetched = simulate(keys, host, set(), cuts, mode)
        assert got == exp, cuts
        assert not fetched      # the device's predecessor key was always known to the host
    # the device's own mask is wrong exactly where the definition says so: line 3 repeats A for the device
    dev, _ = simulate(keys, set(), set(), [], mode)
    assert dev == exp           # nothing to correct without host rows
    no_host = restate([None if i in host else k for i, k in enumerate(keys)])
    assert no_host[3] == 1 and exp[3] == 0


@pytest.mark.parametrize("mode", ["json", "wire"])
def test_tracker_random_streams(mode):
    rng = np.random.default_rng(3)
    pool = [("MU", "1", "a"), ("MU", "1", "b"), ("MS", "1", "a"), ("MC", "4", "q")]
    for trial in range(200):
        n = int(rng.integers(1, 60))
        keys = [None if rng.random() < 0.3 else pool[int(rng.integers(0, 2 + trial % 3))] for _ in range(n)]
        for i in range(1, n):       # runs: repeat the previous line's key often
            if rng.random() < 0.5:
                keys[i] = keys[i - 1]
        host = {i for i in range(n) if rng.random() < 0.2}
        redo = {i for i in host if rng.random() < 0.3}
        cuts = sorted(set(int(x) for x in rng.integers(1, n + 1, int(rng.integers(0, 5))) if x < n))
        got, _ = simulate(keys, host, redo, cuts, mode)
        assert got == restate(keys), (trial, keys, host, redo, cuts)


def test_collapse_objects_is_the_definition():
    from types import SimpleNamespace as NS
    m = lambda kind, pid, p, extra=(): [NS(raw=NS(message_type=kind), protocol_id=pid, payload=p)] + list(extra)  # noqa: E731
    out = [m("MU", "1", "x"), [], m("MU", "1", "x", [1]), ValueError("c"), m("MS", "1", "x"), m("MS", "1", "x"), m("MS", "1", "y")]
    mask = repeats.collapse_objects(out)
    assert mask.tolist() == [0, 0, 1, 0, 0, 1, 0]
    assert out[2] == [] and out[5] == [] and out[0] and isinstance(out[3], ValueError)


def test_apply_mask_drops_and_republishes():
    """Lines 0 A (device), 1 G (host row), 2 A (device), 3 G (host row), 4 G (device), 5 A, 6 A (device).
    The device does not see the host rows: it skipped line 2 as a repeat of line 0 -- its true predecessor
    is the host row 1, so it is published after all -- and published line 4, which repeats the host row 3;
    line 3 is no repeat, lines 5 and 6 were decided correctly."""
    rep = np.array([0, 0, 1, 0, 0, 0, 1], np.uint8)      # the device's mask
    mask = np.array([0, 0, 0, 0, 1, 0, 1], np.uint8)     # the exact one
    dropped, republished = [], []
    repeats.apply_mask(mask, rep, {1: ("MU", "9", "gg"), 3: ("MU", "9", "gg")}, dropped.append, republished.append)
    assert republished == [2] and dropped == [4]
    # a host row that is a repeat is dropped; one without a result and one that is published are left alone
    dropped, republished = [], []
    mask = np.array([0, 1, 0, 0, 0, 0, 1], np.uint8)
    repeats.apply_mask(mask, rep, {1: ("MU", "1", "aa"), 3: None, 5: ("MU", "2", "b")}, dropped.append, republished.append)
    assert dropped == [1] and republished == [2]
    # nothing differs and there is no host row: nothing is touched
    repeats.apply_mask(rep, rep, {}, dropped.append, republished.append)
    assert dropped == [1] and republished == [2]


# ---- LineStream against a scripted engine -------------------------------------------------------------
def line_key(ln: bytes):
    """A scripted line b'MU;K=<proto>:<payload>;...' -> its key, None without a K field."""
    m = re.search(rb"K=(\d+):(\w*);", ln)
    return (ln[:2].decode(), m.group(1).decode(), m.group(2).decode()) if m else None


def line_text(ln: bytes):
    k = line_key(ln)
    return None if k is None else json.dumps({"protocol_id": k[1], "payload": k[2], "metadata": {"src": ln.decode()}})


class RepeatEngine(H.FakeEngine):
    """FakeEngine + the repeat entries: mark_repeats is the definition over the lines the device sees (its
    kind's OK lines), the state's head written as sdx_mark_repeats' state pass writes it; launch_json builds
    the line's JSON text and honours skip.  Stream / event traffic is logged in ``calls``."""

    def __init__(self):
        super().__init__()
        self.dev_prev = None

    def alloc_repeat_state(self):
        return H.FT(np.zeros(65552, np.uint8))

    def alloc_repeat(self, n):
        return H.FT(np.zeros(max(n, 1), np.uint8)), H.FT(np.zeros(64, np.uint8))

    def json_in(self, kind, demod_out, lines_out, n, first_only=True):
        return (kind, lines_out["meta"].owner)

    def _text_lines(self, lb, n, want=None):
        b, o = lb.bytes.a, lb.offsets.a
        for i in range(n):
            if lb.status.a[i] == runtime.LS_OK and (want is None or lb.kind.a[i] == want):
                ln = b[o[i]: o[i + 1]].tobytes()
                if line_key(ln) is not None:
                    yield i, ln

    def mark_repeats(self, json_ins, n, repeat, scratch, state, stream=None):
        self.calls.append(("mark", n, stream))
        lb = json_ins[0][1]
        repeat.a[:n] = 0
        for i, ln in self._text_lines(lb, n):
            k = line_key(ln)
            repeat.a[i] = int(k == self.dev_prev)
            self.dev_prev = k
            p = k[2].encode()
            state.a[:16].view(np.uint32)[:] = (1, NAMES.index(k[0]), int(k[1]), len(p))
            state.a[16: 16 + len(p)] = np.frombuffer(p, np.uint8)

    def launch_json(self, kind, demod_out, lines_out, n, jout, first_only=True, skip=None):
        self.calls.append(("json", kind))
        lb = lines_out["meta"].owner
        want = (runtime.LINE_MU, runtime.LINE_MS, runtime.LINE_MC, runtime.LINE_MN)[kind]
        for i, ln in self._text_lines(lb, n, want):
            if skip is not None and skip.a[i]:
                continue
            txt = line_text(ln).encode()
            c = int(jout["cursor"].a[0])
            jout["json"].a[c: c + len(txt)] = np.frombuffer(txt, np.uint8)
            jout["off"].a[i], jout["len"].a[i] = c, len(txt)
            jout["cursor"].a[0] = c + len(txt)


class RepeatParser(H.FakeParser):
    def __init__(self, eng):
        super().__init__(eng)
        pids = [str(i) for i in range(100)]
        self.protocols._bank.mu_pids = self.protocols._bank.ms_pids = self.protocols._bank.mc_pids = pids
        self.protocols._bank.mn_pids = pids

    def parse_lines_json(self, lines, collapse_repeats=False):
        self.host_calls.append(len(lines))
        return [line_text(bytes(x)) for x in lines]


@pytest.fixture
def rstub(monkeypatch):
    ft = H.fake_torch()
    log = []

    class St(H._St):
        def wait_event(self, e):
            log.append(("wait", id(self), e))

    class Ev(H._Ev):
        def record(self, stream=None):
            log.append(("record", id(stream), self))
    ft.cuda.Stream, ft.cuda.Event = St, Ev
    monkeypatch.setitem(sys.modules, "torch", ft)
    monkeypatch.setattr(frontend, "LineBatch", H.FakeLineBatch)

    def copy(dst, src, st=None):
        dst.a.view(np.uint8)[:] = src.a.view(np.uint8)

    def fill(dst, st=None, value=0):
        dst.a.view(np.uint8)[:] = value
    monkeypatch.setattr(runtime, "copy_async", copy)
    monkeypatch.setattr(runtime, "copy_d2h", copy)
    monkeypatch.setattr(runtime, "fill_async", fill)
    eng = RepeatEngine()
    eng.log = log
    return eng


def scripted_lines():
    """Device lines, noise, and GEN lines (LS_GENERAL: resolved by the batch API, invisible to the device)."""
    A, B_, G, N = b"MU;K=1:aa;", b"MS;K=2:bb;", b"MU;K=9:gg;GEN;", b"XX;noise;"
    seq = [A, A, G, A, A, B_, B_, G, A, N, G, G, N, G, A, G,    # chunk 0 (16 lines) ends in a host row
           G, A, A, N, N, N, N, N, N, N, N, N, N, N, N, A,      # chunk 1 starts with its repeat; ends inside a run
           N, N, N, N, N, N, N, N, N, N, N, N, N, N, N, N,      # chunk 2: no results
           A, G, N, N, N, N, N, N, N, N, N, N, N, N, N, G,      # chunk 3
           N, N, N, N, N, N, N, N, N, N, N, N, N, N, N, N,      # chunk 4: no results behind a host row
           G, A, B_, B_]                                        # chunk 5
    return seq


@pytest.mark.parametrize("lag", [1, 3])
def test_stream_collect_returns_the_exact_mask_and_texts(rstub, lag):
    eng = rstub
    parser = RepeatParser(eng)
    ls = stream.LineStream(parser, chunk_lines=16, chunk_bytes=4096, output="json", lag=lag, collapse_repeats=True)
    seq = scripted_lines()
    got = []
    for a in range(0, len(seq), 16):
        ls.submit(seq[a: a + 16])
        if a == 32:
            got += [r.detach() for r in ls.poll()]
    got += [r.detach() for r in ls.drain()]
    keys = [line_key(x) for x in seq]
    exp = restate(keys)
    mask = [m for r in got for m in r.repeat.tolist()]
    assert mask == exp
    texts = [t for r in got for t in r.texts()]
    assert texts == [None if m else line_text(x) for m, x in zip(exp, seq)]
    assert [i for r in got for i, _ in r.items()] == [i % 16 for i, (m, k) in enumerate(zip(exp, keys)) if k and not m]
    # the device alone was wrong where the definition needs the host row: line 3 (the A behind G) was skipped
    dev = restate([None if b"GEN" in x else k for x, k in zip(seq, keys)])
    assert dev[3] == 1 and exp[3] == 0
    # its text came from one batch-API call for that line, not from a re-run of the chunk
    assert max(parser.host_calls) <= 8


def test_stream_orders_the_repeat_passes_between_chunks(rstub):
    """Chunk k+1's sdx_mark_repeats waits, on its own demodulation stream, for an event recorded on chunk
    k's stream behind k's repeat pass; nothing else of chunk k+1 is enqueued before its demodulation."""
    eng = rstub
    ls = stream.LineStream(RepeatParser(eng), chunk_lines=16, chunk_bytes=4096, output="json", lag=2,
                           collapse_repeats=True)
    seq = scripted_lines()
    for a in range(0, 64, 16):
        ls.submit(seq[a: a + 16])
    ls.drain()
    marks = [i for i, c in enumerate(eng.calls) if c[0] == "mark"]
    assert len(marks) == 4
    sds = [id(s) for s in ls.sds]
    assert [id(eng.calls[i][2]) for i in marks] == [sds[0], sds[1], sds[0], sds[1]]   # alternating streams
    # per chunk: [step/mn launches ...] mark [json ...]: the demodulation is enqueued before the wait
    with_step = 0
    for k, i in enumerate(marks):
        lo = marks[k - 1] if k else -1
        between = [c[0] for c in eng.calls[lo + 1: i]]     # the previous chunk's json launches, then this chunk's
        if "step" in between:                              # (chunk 2 holds no device line: no launch at all)
            with_step += 1
            assert "json" not in between[between.index("step"):]
    assert with_step == 3
    # events: every record on a demodulation stream that a later wait on the OTHER stream names
    log = eng.log
    rep_waits = [(j, e) for j, (what, st, e) in enumerate(log) if what == "wait" and st in sds and
                 any(w == "record" and s2 in sds and s2 != st and e2 is e for w, s2, e2 in log[:j])]
    assert len(rep_waits) == 3      # chunks 1, 2, 3 each wait for their predecessor's state pass
    for j, e in rep_waits:
        rec = next(jj for jj, (w, s2, e2) in enumerate(log) if w == "record" and e2 is e)
        assert rec < j


def test_stream_default_launches_no_repeat_pass(rstub):
    eng = rstub
    ls = stream.LineStream(RepeatParser(eng), chunk_lines=16, chunk_bytes=4096, output="json", lag=2)
    seq = scripted_lines()
    ls.submit(seq[:16])
    r = ls.drain()[0]
    assert r.repeat is None and not any(c[0] == "mark" for c in eng.calls)
    assert [t for t in r.texts()] == [line_text(x) for x in seq[:16]]


# ---- controller ---------------------------------------------------------------------------------------
class _Msg:
    def __init__(self, kind, pid, payload):
        self.raw = type("R", (), {"message_type": kind})()
        self.protocol_id, self.payload = pid, payload


class ObjParser:
    """parse_lines over scripted lines; collapse within the call is the product's own collapse_objects."""

    def parse_lines(self, lines, collapse_repeats=False):
        out = []
        for ln in lines:
            k = line_key(ln)
            out.append(ValueError("contract") if b"ERR" in ln else [] if k is None else [_Msg(*k), _Msg(k[0], "x", "later")])
        if collapse_repeats:
            repeats.collapse_objects(out)
        return out


class _Pub:
    def __init__(self, log):
        self.log = log

    async def publish(self, msg):
        self.log.append(("pub", (msg.raw.message_type, msg.protocol_id, msg.payload)))


class _Ctl:
    def __init__(self, parser, lines, log):
        self.parser, self.log = parser, log
        self._raw_message_queue = asyncio.Queue()
        for ln in lines:
            self._raw_message_queue.put_nowait(ln)
        self._stop_event = asyncio.Event()
        self.mqtt_publisher = _Pub(log)
        self.todo = len(lines)

    async def message_callback(self, msg):
        self.log.append(("cb", (msg.raw.message_type, msg.protocol_id, msg.payload)))

    async def _handle_as_command_response(self, line):
        self.log.append(("cmd", line))
        self.todo -= 1
        if self.todo == 0:
            self._stop_event.set()


def reference_effects(lines, collapse):
    """The reference loop's effects per line (controller.py:252-258), a repeat publishing nothing."""
    keys = [None if b"ERR" in ln else line_key(ln) for ln in lines]
    mask = restate(keys) if collapse else [0] * len(lines)
    log = []
    for ln, k, m in zip(lines, keys, mask):
        if k is not None and not m:
            log += [("cb", k), ("pub", k)]
        log.append(("cmd", ln))
    return log


@pytest.mark.parametrize("max_batch", [1, 3, 64])
@pytest.mark.parametrize("collapse", [False, True])
def test_controller_objects_effects(max_batch, collapse):
    A, B_, N, E = b"MU;K=1:aa;", b"MS;K=1:aa;", b"XX;noise;", b"MU;K=1:aa;ERR;"
    lines = [A, A, N, A, E, A, B_, B_, N, N, B_, A, A, A, B_]
    log = []
    c = _Ctl(ObjParser(), lines, log)
    task = ctl.BatchingParserTask(c, max_batch=max_batch, max_delay=0.001, publish="objects",
                                  **({"collapse_repeats": True} if collapse else {}))
    asyncio.run(asyncio.wait_for(task.run(), 20))
    assert log == reference_effects(lines, collapse)
    if collapse:
        assert sum(1 for x in log if x[0] == "pub") < sum(1 for x in reference_effects(lines, False) if x[0] == "pub")
