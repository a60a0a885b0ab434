"""Repeat suppression with a time window, host side, on the CPU: collapse_objects with
times, RepeatTracker's (K, T) around host-resolved rows on scripted device masks, the checks of the times,
LineStream's per-chunk and per-buffer times against a scripted engine (the stand-ins of
tests/test_repeats_host.py, which here also script sdx_mark_repeats_timed), and the controller's stamps.
Expected values: ``restate``, the serial restatement of the recurrence, over keys and times the tests
choose themselves."""
import asyncio
import os
import subprocess

import numpy as np
import pytest

from pysignalduino_amd import controller as ctl
from pysignalduino_amd import frontend, repeats, runtime, stream

import test_stream_host as H
import test_repeats_host as RH
from test_repeats_host import rstub  # noqa: F401  (the fixture)

W = 2_000_000


def restate(keys, times, w):
    K, T, mask = None, None, []
    for k, t in zip(keys, times):
        rep = k is not None and K is not None and k == K and (w is None or t - T <= w)
        mask.append(int(rep))
        if k is not None:
            K, T = k, (T if rep else t)
    return mask


# ---- the ABI and the layout ---------------------------------------------------------------------------
def test_abi_declares_the_timed_entries():
    import re
    hdr = open(os.path.join(os.path.dirname(runtime.HERE), "include", "sdx.h")).read()
    for name in ("sdx_mark_repeats_timed", "sdx_repeat_timed_state_bytes", "sdx_repeat_timed_scratch_bytes"):
        assert name in runtime.EXPORTED and re.search(r"\b%s\(" % name, hdr), name
    lib = runtime.load_library()
    assert lib.sdx_abi_version() == runtime.ABI_VERSION            # additive: the version stays
    assert lib.sdx_repeat_timed_state_bytes() >= 24 + 65535 and lib.sdx_repeat_timed_state_bytes() % 16 == 0
    T = lib.sdx_repeat_tile()
    for n in (1, T, T + 1, 250_000):
        assert lib.sdx_repeat_timed_scratch_bytes(n) >= 16 + 41 * n + 20 * -(-n // T)
        assert lib.sdx_repeat_timed_scratch_bytes(n) % 16 == 0


def test_timed_layout_helpers_under_sanitizers(tmp_path):
    """tools/repeat_timed_layout_check.cpp: the size / offset helpers sdx_mark_repeats_timed shares with
    its callers, as a stand-alone host program built with -fsanitize=address,undefined."""
    src = os.path.join(os.path.dirname(runtime.HERE), "tools", "repeat_timed_layout_check.cpp")
    exe = str(tmp_path / "repeat_timed_layout_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "repeat_timed_layout_check: ok" in r.stdout, r.stderr[-2000:]


# ---- collapse_objects -----------------------------------------------------------------------------------
def _m(kind, pid, p):
    from types import SimpleNamespace as NS
    return [NS(raw=NS(message_type=kind), protocol_id=pid, payload=p)]


def test_collapse_objects_with_times():
    A, B = ("MU", "1", "x"), ("MS", "1", "x")
    keys = [A, None, A, A, B, B, A, A, None, A]
    times = [0, 100, 1_500_000, 2_500_000, 2_600_000, 4_600_000, 4_600_001, 6_600_001, 6_600_002, 6_600_002]
    out = [[] if k is None else _m(*k) for k in keys]
    mask = repeats.collapse_objects(out, times, W)
    assert mask.tolist() == restate(keys, times, W) == [0, 0, 1, 0, 0, 1, 0, 1, 0, 0]
    assert [bool(o) for o in out] == [k is not None and not m for k, m in zip(keys, mask)]
    # W = 0, and no window
    out = [_m(*A) for _ in range(4)]
    assert repeats.collapse_objects(out, [5, 5, 6, 6], 0).tolist() == [0, 1, 0, 1]
    out = [_m(*A) for _ in range(4)]
    assert repeats.collapse_objects(out).tolist() == [0, 1, 1, 1]
    # a carried (K, T): the calls continue one stream
    carry = [None, 0, None]
    got = []
    for a, b in ((0, 3), (3, 4), (4, 10)):
        got += repeats.collapse_objects([[] if k is None else _m(*k) for k in keys[a:b]], times[a:b], W, carry).tolist()
    assert got == restate(keys, times, W)
    with pytest.raises(ValueError, match="decrease"):
        repeats.collapse_objects([_m(*A)], [times[-1] - 1], W, carry)


def test_times_are_checked():
    A = ("MU", "1", "x")
    with pytest.raises(ValueError, match="decrease"):
        repeats.collapse_objects([_m(*A), _m(*A)], [5, 4], W)
    with pytest.raises(ValueError, match="times"):
        repeats.collapse_objects([_m(*A), _m(*A)], None, W)
    with pytest.raises(ValueError, match="2 times for 3"):
        repeats.check_times([1, 2], 3)
    with pytest.raises(ValueError, match="integer"):
        repeats.check_times([1.5, 2.5], 2)
    assert repeats.window_to_us(2.0) == 2_000_000 and repeats.window_to_us(0.0000014) == 1
    assert repeats.window_to_us(None) is None
    with pytest.raises(ValueError):
        repeats.window_to_us(-1)
    # the front end's argument check runs before anything is packed or launched
    wa = frontend.SignalParser._window_args
    with pytest.raises(ValueError, match="collapse_repeats"):
        wa(False, [1, 2], 2.0, 2)
    with pytest.raises(ValueError, match="times"):
        wa(True, None, 2.0, 2)
    with pytest.raises(ValueError, match="decrease"):
        wa(True, [2, 1], 2.0, 2)
    t, w = wa(True, [1, 2], 2.0, 2)
    assert t.dtype == np.int64 and t.tolist() == [1, 2] and w == W
    assert wa(True, None, None, 2) == (None, None)


# ---- RepeatTracker: a simulated device that does not see the host rows ----------------------------------
def simulate(keys, times, w, host, redo, cuts, mode, counts=None):
    """As test_repeats_host.simulate, the device running the recurrence with its own (K, T) over the lines
    it sees.  -> (the tracker's mask, lines fetched, the tracker)."""
    tr = repeats.RepeatTracker()
    dK, dT = None, None
    out, fetched = [], []
    for a, b in zip([0] + cuts, cuts + [len(keys)]):
        n = b - a
        rep = np.zeros(n, np.uint8)
        for i in range(a, b):
            if keys[i] is None or (i in host and i not in redo):
                continue
            r = dK is not None and keys[i] == dK and times[i] - dT <= w
            rep[i - a] = int(r)
            dK, dT = keys[i], (dT if r else times[i])
        seen = np.array([keys[i] is not None and (i not in host or i in redo) for i in range(a, b)], bool)
        has_key = seen & (rep == 0) if mode == "json" else seen     # json: a flagged line has no text
        host_keys = {i - a: keys[i] for i in range(a, b) if i in host}

        def fetch(i, a=a):
            fetched.append(a + i)
            return keys[a + i]

        def key_of(i, a=a):
            if counts is not None:
                counts.append(a + i)
            return keys[a + i]
        out += tr.fix_chunk(rep, has_key, key_of, host_keys, [i - a for i in redo if a <= i < b], fetch,
                            times=times[a:b], window_us=w).tolist()
    return out, fetched, tr


A, B_, G = ("MU", "1", "aa"), ("MU", "2", "bb"), ("MS", "7", "gg")
N = None


@pytest.mark.parametrize("mode", ["json", "wire"])
def test_tracker_host_row_inside_a_segment(mode):
    #        0  1  2  3  4  5   6   7
    keys = [A, A, G, A, A, A, B_, B_]
    s = 300_000
    times = [i * s for i in range(8)]
    host = {2}
    exp = restate(keys, times, W)
    assert exp == [0, 1, 0, 0, 1, 1, 0, 1]      # the A behind G is published and is the new anchor
    for cuts in ([], [2], [3], [4], [1, 2, 3, 4, 5, 6, 7]):
        got, fetched, _ = simulate(keys, times, W, host, set(), cuts, mode)
        assert got == exp and not fetched, cuts
    # the device, blind to G, keeps its anchor at line 0: it publishes line 7 s later where the definition,
    # anchored at line 3, does not -- the tracker follows both anchors until they meet
    keys = [A, A, G] + [A] * 12
    times = [i * s for i in range(15)]
    exp = restate(keys, times, W)
    dev = restate([None if i == 2 else k for i, k in enumerate(keys)], times, W)
    assert exp != dev and exp[7] == 1 and dev[7] == 0 and exp[10] == 0 and dev[10] == 1
    for cuts in ([], [5], [8], [3, 9]):
        got, _, _ = simulate(keys, times, W, {2}, set(), cuts, mode)
        assert got == exp, cuts


@pytest.mark.parametrize("mode", ["json", "wire"])
def test_tracker_rerun_row_and_resynchronisation(mode):
    # line 3 is a re-run row (the device may have seen it): what the device holds behind it is unknown
    # until it leaves a line unmarked; a marked line behind it has its key fetched (json)
    keys = [A, A, A, A, A, N, A, B_, B_] + [A, A, A] * 400
    times = [i * 250_000 for i in range(len(keys))]
    exp = restate(keys, times, W)
    for redo_seen in (True, False):
        host, redo = {3}, {3}
        counts = []
        if redo_seen:
            got, fetched, tr = simulate(keys, times, W, host, redo, [], mode, counts)
        else:       # the device did not see the row after all: simulate() decides by membership in redo
            tr = repeats.RepeatTracker()
            dev = restate([None if i == 3 else k for i, k in enumerate(keys)], times, W)
            seen = np.array([k is not None and i != 3 for i, k in enumerate(keys)], bool)
            rep = np.array(dev, np.uint8)
            has_key = seen & (rep == 0) if mode == "json" else seen
            fetched = []

            def key_of(i):
                counts.append(i)
                return keys[i]
            got = tr.fix_chunk(rep, has_key, key_of, {3: keys[3]}, [3], lambda i: (fetched.append(i), keys[i])[1],
                               times=times, window_us=W).tolist()
        assert got == exp
        assert (tr.dev_key, tr.dev_t) == (tr.true_key, tr.true_t) == (A, times[max(i for i, m in enumerate(exp) if not m)])
        # re-decided line by line only up to the next line both publish (B_ at 7), then whole stretches
        assert len(counts) <= 8 and max(counts[:-1]) <= 7, counts
        assert all(i == 4 for i in fetched)


@pytest.mark.parametrize("mode", ["json", "wire"])
def test_tracker_random_streams(mode):
    rng = np.random.default_rng(4)
    pool = [("MU", "1", "a"), ("MU", "1", "b"), ("MS", "1", "a"), ("MC", "4", "q")]
    for trial in range(300):
        n = int(rng.integers(1, 70))
        w = int(rng.choice([0, 10, 1000]))
        keys = [None if rng.random() < 0.3 else pool[int(rng.integers(0, 2 + trial % 3))] for _ in range(n)]
        for i in range(1, n):
            if rng.random() < 0.6:
                keys[i] = keys[i - 1]
        times = np.cumsum(rng.choice([0, w // 4, w // 2, w, w + 1, 3 * w + 1], n)).tolist()
        host = {i for i in range(n) if rng.random() < 0.15}
        redo = {i for i in host if rng.random() < 0.3}
        cuts = sorted(set(int(x) for x in rng.integers(1, n + 1, int(rng.integers(0, 5))) if x < n))
        got, _, _ = simulate(keys, times, w, host, redo, cuts, mode)
        assert got == restate(keys, times, w), (trial, keys, times, w, host, redo, cuts)


# ---- LineStream against a scripted engine -------------------------------------------------------------
class TimedEngine(RH.RepeatEngine):
    """RepeatEngine + the timed entries: mark_repeats_timed is the recurrence over the lines the device
    sees, with the times that were uploaded for the chunk."""

    def __init__(self):
        super().__init__()
        self.K, self.T = None, None

    def alloc_repeat_state(self, timed=False):
        self.state_timed = timed
        return H.FT(np.zeros(65560 if timed else 65552, np.uint8))

    def alloc_repeat_timed(self, n):
        return H.FT(np.zeros(max(n, 1), np.uint8)), H.FT(np.zeros(64, np.uint8))

    def mark_repeats_timed(self, json_ins, n, times, window_us, repeat, scratch, state, stream=None):
        self.calls.append(("mark_timed", n, stream, times.a[:n].copy(), window_us))
        lb = json_ins[0][1]
        repeat.a[:n] = 0
        for i, ln in self._text_lines(lb, n):
            k, t = RH.line_key(ln), int(times.a[i])
            r = self.K is not None and k == self.K and t - self.T <= window_us
            repeat.a[i] = int(r)
            self.K, self.T = k, (self.T if r else t)


@pytest.fixture
def tstub(rstub):  # noqa: F811
    eng = TimedEngine()
    eng.log = rstub.log
    return eng


@pytest.mark.parametrize("lag", [1, 3])
def test_stream_collect_with_a_window(tstub, lag):
    eng = tstub
    parser = RH.RepeatParser(eng)
    ls = stream.LineStream(parser, chunk_lines=16, chunk_bytes=4096, output="json", lag=lag, collapse_repeats=True,
                           repeat_window=2.0)
    assert eng.state_timed
    seq = RH.scripted_lines()
    rng = np.random.default_rng(8)
    times = np.cumsum(rng.choice([0, 400_000, 900_000, 2_000_001], len(seq))).tolist()
    got = []
    for a in range(0, len(seq), 16):
        ls.submit(seq[a: a + 16], times=times[a: a + 16])
    got += [r.detach() for r in ls.drain()]
    keys = [RH.line_key(x) for x in seq]
    exp = restate(keys, times, W)
    assert exp != RH.restate(keys)                                   # the window matters on this script
    assert [m for r in got for m in r.repeat.tolist()] == exp
    assert [t for r in got for t in r.texts()] == [None if m else RH.line_text(x) for m, x in zip(exp, seq)]
    marks = [c for c in eng.calls if c[0] == "mark_timed"]
    assert len(marks) == -(-len(seq) // 16) and not any(c[0] == "mark" for c in eng.calls)
    assert [int(x) for c in marks for x in c[3]] == times and all(c[4] == W for c in marks)   # the times travelled
    assert ls.h2d_bytes >= 8 * len(seq)


def test_stream_refuses_bad_times(tstub):
    eng = tstub
    parser = RH.RepeatParser(eng)
    seq = RH.scripted_lines()[:4]
    with pytest.raises(ValueError, match="collapse_repeats"):
        stream.LineStream(parser, chunk_lines=16, chunk_bytes=4096, repeat_window=2.0)
    ls = stream.LineStream(parser, chunk_lines=16, chunk_bytes=4096, output="json", lag=1, collapse_repeats=True,
                           repeat_window=2.0)
    with pytest.raises(ValueError, match="times"):
        ls.submit(seq)
    with pytest.raises(ValueError, match="3 times for 4"):
        ls.submit(seq, times=[1, 2, 3])
    with pytest.raises(ValueError, match="decrease"):
        ls.submit(seq, times=[1, 2, 4, 3])
    ls.submit(seq, times=[1, 2, 3, 10])
    with pytest.raises(ValueError, match="decrease"):
        ls.submit(seq, times=[9, 11, 12, 13])            # earlier than the previous chunk's last time
    with pytest.raises(ValueError, match="time"):
        ls.submit_bytes(b"MU;x;\n")
    with pytest.raises(ValueError, match="decrease"):
        ls.submit_bytes(b"MU;x;\n", time=9)
    assert not any(c[0] == "mark_timed" and c[1] != 4 for c in eng.calls)   # nothing of the refused calls was launched
    plain = stream.LineStream(parser, chunk_lines=16, chunk_bytes=4096, output="json", lag=1, collapse_repeats=True)
    with pytest.raises(ValueError, match="repeat_window"):
        plain.submit(seq, times=[1, 2, 3, 4])


def test_submit_bytes_assigns_each_line_its_buffers_time(tstub, monkeypatch):
    """A line gets the time of the read buffer that holds its terminating newline; a tail closed by
    close_bytes the last buffer's.  Stage A is cut off: the pieces and their times are recorded."""
    eng = tstub
    ls = stream.LineStream(RH.RepeatParser(eng), chunk_lines=3, chunk_bytes=4096, output="json", lag=1,
                           collapse_repeats=True, repeat_window=2.0)
    pieces = []

    def stage_a_bytes(s, carry, pinned_buf, arr, lo, hi, final):
        pieces.append((bytes(carry) + arr[lo:hi].tobytes(), s.n, s.times.tolist(), s.h_times.numpy()[: s.n].tolist()))

    def queued(s):
        s.reset()
        s.stage = 0
        return s.cid
    monkeypatch.setattr(ls, "_stage_a_bytes", stage_a_bytes)
    monkeypatch.setattr(ls, "_queued", queued)
    ls.submit_bytes(b"aa\nbb\ncc", time=100)            # two lines; 'cc' is carried
    ls.submit_bytes(b"c", time=150)                     # no newline: nothing ends here
    ls.submit_bytes(b"c\ndd\nee\nff\ngg\nhh", time=200)  # 'cccc' ends in this buffer; five lines: two pieces
    ls.submit_bytes(b"", time=300)                      # an empty read
    ls.close_bytes()                                    # 'hh': the last buffer's time
    assert len(pieces) >= 4 and all(p[1] == len(p[0].rstrip(b"\n").split(b"\n")) <= 3 for p in pieces)
    flat = [(ln, t) for p in pieces for ln, t in zip(p[0].rstrip(b"\n").split(b"\n"), p[2])]
    assert flat == [(b"aa", 100), (b"bb", 100), (b"cccc", 200), (b"dd", 200), (b"ee", 200), (b"ff", 200), (b"gg", 200),
                    (b"hh", 300)]
    assert all(p[2] == p[3] for p in pieces)            # in the slot's pinned buffer, for the upload


# ---- controller ---------------------------------------------------------------------------------------
class Clock:
    """Microseconds from a script; every reading is logged."""

    def __init__(self, values):
        self.values, self.read = list(values), []

    def __call__(self):
        self.read.append(self.values.pop(0))
        return self.read[-1]


def timed_effects(lines, times, w):
    keys = [None if b"ERR" in ln else RH.line_key(ln) for ln in lines]
    log = []
    for ln, k, m in zip(lines, keys, restate(keys, times, w)):
        if k is not None and not m:
            log += [("cb", k), ("pub", k)]
        log.append(("cmd", ln))
    return log


def test_controller_stamps_lines_as_they_leave_the_queue():
    Aq, Bq, Nn, E = b"MU;K=1:aa;", b"MS;K=1:aa;", b"XX;noise;", b"MU;K=1:aa;ERR;"
    lines = [Aq, Aq, Nn, Aq, E, Aq, Bq, Bq, Nn, Nn, Bq, Aq, Aq, Aq, Bq]
    stamps = np.cumsum([7, 900_000, 10, 900_000, 5, 900_000, 0, 2_000_000, 1, 1, 1, 2_000_001, 2_000_000, 1, 0]).tolist()
    assert restate([RH.line_key(x) for x in lines], stamps, W) != RH.restate([RH.line_key(x) for x in lines])
    # max_batch = 1: every line is taken by its own get(), one reading of the clock each
    log = []
    c = RH._Ctl(RH.ObjParser(), lines, log)
    clock = Clock(stamps)
    task = ctl.BatchingParserTask(c, max_batch=1, max_delay=0.001, publish="objects", collapse_repeats=True,
                                  repeat_window=2.0, clock=clock)
    asyncio.run(asyncio.wait_for(task.run(), 20))
    assert clock.read == stamps
    assert log == timed_effects(lines, stamps, W)
    # max_batch = 64, all lines queued: the first by get(), the rest taken together with one reading
    log = []
    c = RH._Ctl(RH.ObjParser(), lines, log)
    clock = Clock([50, 60])
    task = ctl.BatchingParserTask(c, max_batch=64, max_delay=0.001, publish="objects", collapse_repeats=True,
                                  repeat_window=2.0, clock=clock)
    asyncio.run(asyncio.wait_for(task.run(), 20))
    assert clock.read == [50, 60]
    assert log == timed_effects(lines, [50] + [60] * (len(lines) - 1), W)
    # the default clock is the monotonic one, in microseconds
    import time
    task = ctl.BatchingParserTask(c, collapse_repeats=True, repeat_window=2.0)
    a = time.monotonic_ns() // 1000
    assert a <= task.clock() <= time.monotonic_ns() // 1000
    with pytest.raises(ValueError, match="collapse_repeats"):
        ctl.BatchingParserTask(c, repeat_window=2.0)


def test_controller_json_hands_the_stamps_to_the_stream():
    lines = [b"MU;K=1:aa;", b"", b"MU;K=1:aa;", b"MS;K=2:bb;"]     # an empty line is dropped with its stamp
    seen = {}

    class Res:
        def __init__(self, cid, n):
            self.id, self.n = cid, n

        def texts(self):
            return [None] * self.n

    class FakeStream:
        def __init__(self):
            self.q = []

        def submit(self, ls_lines, times=None):
            seen.setdefault("submits", []).append((list(ls_lines), times))
            self.q.append(Res(len(seen["submits"]) - 1, len(ls_lines)))
            return self.q[-1].id

        def poll(self):
            out, self.q = self.q, []
            return out
        drain = poll

    class P:
        def stream(self, **kw):
            seen["kw"] = kw
            return FakeStream()
    class JsonCtl:   # no message_callback: publish='json' produces texts only
        def __init__(self):
            self.parser = P()
            self._raw_message_queue = asyncio.Queue()
            for ln in lines:
                self._raw_message_queue.put_nowait(ln)
            self._stop_event = asyncio.Event()
            self.mqtt_publisher = None
            self.todo = 3

        async def _handle_as_command_response(self, line):
            self.todo -= 1
            if self.todo == 0:
                self._stop_event.set()

    task = ctl.BatchingParserTask(JsonCtl(), max_batch=64, max_delay=0.001, publish="json", collapse_repeats=True,
                                  repeat_window=2.0, clock=Clock([10, 20, 30, 40]))
    asyncio.run(asyncio.wait_for(task.run(), 20))
    assert seen["kw"]["collapse_repeats"] is True and seen["kw"]["repeat_window"] == 2.0
    assert seen["submits"] == [([lines[0], lines[2], lines[3]], [10, 20, 20])]
