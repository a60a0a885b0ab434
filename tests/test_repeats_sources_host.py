"""Repeat suppression per receiver, host side: the ABI and the layout helpers of
sdx_mark_repeats_by_source, collapse_objects(sources=), the per-source trackers around host-resolved rows,
and LineStream's per-source ids, times and carried tails -- without a GPU (the numpy stand-ins of
test_stream_host.py).  Expected masks come from ``restate``: the recurrence with one [K, T] per source."""
import os
import subprocess

import numpy as np
import pytest

from pysignalduino_amd import frontend, repeats, runtime, stream

import test_stream_host as H
import test_repeats_host as RH
from test_repeats_host import rstub  # noqa: F401  (the fixture)

W = 2_000_000


def restate(keys, srcs, times, w):
    carry, mask = {}, []
    for k, s, t in zip(keys, srcs, times):
        K, T = carry.get(s, (None, None))
        rep = k is not None and K is not None and k == K and (w is None or t - T <= w)
        mask.append(int(rep))
        if k is not None:
            carry[s] = (k, T if rep else t)
    return mask


# ---- the ABI and the layout ---------------------------------------------------------------------------
def test_abi_declares_the_by_source_entries():
    import re
    hdr = open(os.path.join(os.path.dirname(runtime.HERE), "include", "sdx.h")).read()
    for name in ("sdx_mark_repeats_by_source", "sdx_repeat_sources_state_bytes", "sdx_repeat_sources_scratch_bytes"):
        assert name in runtime.EXPORTED and re.search(r"\b%s\(" % name, hdr), name
    lib = runtime.load_library()
    assert lib.sdx_abi_version() == runtime.ABI_VERSION == 14      # additive: the version stays
    slot = lib.sdx_repeat_timed_state_bytes()
    assert lib.sdx_repeat_sources_state_bytes(1) == slot           # S = 1: the timed entry's state buffer
    assert lib.sdx_repeat_sources_state_bytes(16) == 16 * slot < (1 << 20) + 1024
    assert lib.sdx_repeat_sources_state_bytes(4096) == 4096 * slot
    assert lib.sdx_repeat_sources_state_bytes(0) == lib.sdx_repeat_sources_state_bytes(4097) == 0
    assert runtime.REPEAT_SOURCE_ENTRY.itemsize == 32 and runtime.REPEAT_SLOT_HDR == 24
    for n, S in ((1, 1), (257, 3), (250_000, 4096)):
        size = lib.sdx_repeat_sources_scratch_bytes(n, S)
        assert size % 16 == 0 and size >= 16 + 32 * S + lib.sdx_repeat_timed_scratch_bytes(n)
    assert lib.sdx_repeat_sources_scratch_bytes(10, 0) == lib.sdx_repeat_sources_scratch_bytes(10, 4097) == 0


def test_by_source_layout_helpers_under_sanitizers(tmp_path):
    """tools/repeat_sources_layout_check.cpp: the size / offset helpers sdx_mark_repeats_by_source shares with
    its callers, as a stand-alone host program built with -fsanitize=address,undefined."""
    src = os.path.join(os.path.dirname(runtime.HERE), "tools", "repeat_sources_layout_check.cpp")
    exe = str(tmp_path / "repeat_sources_layout_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "repeat_sources_layout_check: ok" in r.stdout, r.stderr[-2000:]


# ---- collapse_objects, the argument checks ----------------------------------------------------------------
def _m(kind, pid, p):
    from types import SimpleNamespace as NS
    return [NS(raw=NS(message_type=kind), protocol_id=pid, payload=p)]


A, B_, G = ("MU", "1", "aa"), ("MU", "2", "bb"), ("MS", "7", "gg")
N = None


def test_collapse_objects_by_source():
    objs = lambda keys: [[] if k is None else _m(*k) for k in keys]   # noqa: E731
    # two receivers hear the same telegram; another receiver's telegram does not break a run
    assert repeats.collapse_objects(objs([A, A, A, A]), sources=[0, 1, 0, 1]).tolist() == [0, 0, 1, 1]
    assert repeats.collapse_objects(objs([A, B_, A]), sources=[0, 1, 0]).tolist() == [0, 0, 1]
    assert repeats.collapse_objects(objs([A, A, A, A])).tolist() == [0, 1, 1, 1]            # without ids: one stream
    keys = [A, A, N, A, B_, A, A, B_, A, A, A, N]
    srcs = [0, 1, 1, 0, 2, 1, 0, 2, 1, 0, 2, 0]
    times = [0, -50, -40, 1_500_000, 7, 1_999_950, 2_500_000, 2_000_007, 2_000_000, 2_600_000, 2_000_008, 2_700_000]
    for w in (W, 0, None):
        out = objs(keys)
        mask = repeats.collapse_objects(out, times, w, sources=srcs)
        assert mask.tolist() == restate(keys, srcs, times, w), w
        assert [bool(o) for o in out] == [k is not None and not m for k, m in zip(keys, mask)]
    assert restate(keys, srcs, times, W) == [0, 0, 0, 1, 0, 1, 0, 1, 0, 1, 0, 0]
    # a carried dict source -> [K, T, last time]: the calls continue every source's stream
    carry, got = {}, []
    for a, b in ((0, 2), (2, 3), (3, 9), (9, 12)):
        got += repeats.collapse_objects(objs(keys[a:b]), times[a:b], W, carry, sources=srcs[a:b]).tolist()
    assert got == restate(keys, srcs, times, W) and sorted(carry) == [0, 1, 2]
    with pytest.raises(ValueError, match="decrease"):
        repeats.collapse_objects(objs([A]), [times[8] - 1], W, carry, sources=[1])
    assert repeats.collapse_objects(objs([A]), [times[8] - 1], W, carry, sources=[3]).tolist() == [0]   # a new source


def test_ids_and_times_are_checked():
    cs, ct = repeats.check_sources, repeats.check_times
    assert cs([0, 2, 1], 3, 3).dtype == np.int32 and cs(np.array([4095], np.int64), 1).tolist() == [4095]
    for bad, n, S in (([0, 3], 2, 3), ([-1, 0], 2, 3), ([0.0, 1.0], 2, 3), ([0], 2, 3), ([[0, 1]], 2, 3),
                      ([0, 4096], 2, None), (None, 2, 3), (["0", "1"], 2, 3)):
        with pytest.raises(ValueError):
            cs(bad, n, S)
    src = np.array([0, 1, 0, 1], np.int32)
    assert ct([10, 1, 10, 2], 4, sources=src).tolist() == [10, 1, 10, 2]      # decreasing across sources only
    with pytest.raises(ValueError, match="decrease"):
        ct([10, 2, 11, 1], 4, sources=src)
    with pytest.raises(ValueError, match="decrease"):
        ct([10, 2, 11, 3], 4, {1: 3}, src)                                    # earlier than source 1's last time
    assert ct([10, 3, 11, 3], 4, {1: 3, 7: 99}, src) is not None
    with pytest.raises(ValueError, match="decrease"):
        ct([10, 1, 10, 2], 4)                                                 # without ids: over the merged lines
    # the front end's argument checks run before anything is packed or launched
    sa, wa = frontend.SignalParser._source_args, frontend.SignalParser._window_args
    with pytest.raises(ValueError, match="collapse_repeats"):
        sa(False, [0, 1], 2)
    assert sa(False, None, 2) is None and sa(True, [0, 1], 2).tolist() == [0, 1]
    t, w = wa(True, [10, 1, 10, 2], 2.0, 4, src)
    assert t.tolist() == [10, 1, 10, 2] and w == W
    with pytest.raises(ValueError, match="decrease"):
        wa(True, [10, 2, 11, 1], 2.0, 4, src)
    with pytest.raises(ValueError):
        runtime._n_sources(0)
    with pytest.raises(ValueError):
        runtime._n_sources(4097)


# ---- SourceTrackers: a simulated device that does not see the host rows ----------------------------------
def simulate(keys, srcs, times, w, host, redo, cuts, mode, S):
    """The device runs the per-source recurrence with its own (K, T) per source over the lines it sees (not the
    host rows, unless they are re-run rows) and leaves the compact table; the trackers repair the chunks."""
    tr = repeats.SourceTrackers()
    dev = {}
    out = []
    for a, b in zip([0] + cuts, cuts + [len(keys)]):
        n = b - a
        rep = np.zeros(n, np.uint8)
        table = np.zeros(S, runtime.REPEAT_SOURCE_ENTRY)
        table["last"] = -1
        for i in range(a, b):
            if keys[i] is None or (i in host and i not in redo):
                continue
            dK, dT = dev.get(srcs[i], (None, None))
            r = dK is not None and keys[i] == dK and (w is None or times[i] - dT <= w)
            rep[i - a] = int(r)
            dev[srcs[i]] = (keys[i], dT if r else times[i])
            table[srcs[i]]["last"] = i - a
        seen = np.array([keys[i] is not None and (i not in host or i in redo) for i in range(a, b)], bool)
        has_key = seen & (rep == 0) if mode == "json" else seen     # json: a flagged line has no text
        host_keys = {i - a: keys[i] for i in range(a, b) if i in host}
        kw = {} if w is None else {"times": np.asarray(times[a:b], np.int64), "window_us": w}
        out += tr.fix_chunk(np.asarray(srcs[a:b], np.int32), rep, has_key, lambda i, a=a: keys[a + i], host_keys,
                            [i - a for i in redo if a <= i < b], lambda i, a=a: keys[a + i], table=table, **kw).tolist()
    return out, tr


@pytest.mark.parametrize("mode", ["json", "wire"])
def test_trackers_repair_each_source_on_its_own(mode):
    #       0  1  2  3  4  5   6  7   8  9
    keys = [A, A, G, A, A, B_, A, B_, A, A]
    srcs = [0, 1, 0, 0, 1, 1, 0, 1, 1, 0]
    times = [i * 300_000 for i in range(10)]
    host = {2}           # source 0's G is resolved on the host: the device takes its line 3 for a repeat
    for w in (None, W):
        exp = restate(keys, srcs, times, w)
        assert exp == [0, 0, 0, 0, 1, 0, 1, 1, 0, 1]
        for cuts in ([], [2], [3], [4], [1, 2, 3, 4, 5, 6, 7, 8, 9]):
            got, tr = simulate(keys, srcs, times, w, host, set(), cuts, mode, 2)
            assert got == exp, (w, cuts)
            assert sorted(tr.trackers) == [0, 1] and tr.trackers[0].true_key == A and tr.trackers[1].true_key == A


@pytest.mark.parametrize("mode", ["json", "wire"])
def test_trackers_random_streams(mode):
    rng = np.random.default_rng(5)
    pool = [("MU", "1", "a"), ("MU", "1", "b"), ("MS", "1", "a"), ("MC", "4", "q")]
    for trial in range(300):
        n = int(rng.integers(1, 70))
        S = int(rng.choice([1, 2, 5]))
        w = [0, 10, 1000, None][trial % 4]
        keys = [None if rng.random() < 0.3 else pool[int(rng.integers(0, 2 + trial % 3))] for _ in range(n)]
        for i in range(1, n):
            if rng.random() < 0.6:
                keys[i] = keys[i - 1]
        srcs = rng.integers(0, S, n).tolist()
        ww = w or 10
        clock, times = {s: int(rng.integers(-5 * ww - 5, 5 * ww + 5)) for s in range(S)}, []
        for s in srcs:
            clock[s] += int(rng.choice([0, ww // 4, ww // 2, ww, ww + 1, 3 * ww + 1]))
            times.append(clock[s])
        host = {i for i in range(n) if rng.random() < 0.15}
        redo = {i for i in host if rng.random() < 0.3}
        cuts = sorted(set(int(x) for x in rng.integers(1, n + 1, int(rng.integers(0, 5))) if x < n))
        got, _ = simulate(keys, srcs, times, w, host, redo, cuts, mode, S)
        assert got == restate(keys, srcs, times, w), (trial, keys, srcs, times, w, host, redo, cuts)


# ---- LineStream against a scripted engine -------------------------------------------------------------
class SourcesEngine(RH.RepeatEngine):
    """RepeatEngine + the by-source entry: mark_repeats_by_source is the per-source recurrence over the lines
    the device sees, with the ids (and times) that were uploaded for the chunk; it leaves the compact table
    where the library leaves it."""

    def __init__(self):
        super().__init__()
        self.dev = {}

    def alloc_repeat_state(self, timed=False, sources=None):
        self.state_args = (timed, sources)
        return H.FT(np.zeros(64, np.uint8))

    def alloc_repeat_sources(self, n, sources):
        return H.FT(np.zeros(max(n, 1), np.uint8)), H.FT(np.zeros(16 + 32 * sources + 64, np.uint8))

    def repeat_sources_table(self, scratch, sources):
        return scratch[16: 16 + 32 * sources]

    def mark_repeats_by_source(self, json_ins, n, source, sources, times, window_us, repeat, scratch, state, stream=None):
        self.calls.append(("mark_src", n, stream, source.a[:n].copy(), None if times is None else times.a[:n].copy(),
                           window_us, sources))
        lb = json_ins[0][1]
        repeat.a[:n] = 0
        table = scratch.a[16: 16 + 32 * sources].view(runtime.REPEAT_SOURCE_ENTRY)
        table["last"] = -1
        for i, ln in self._text_lines(lb, n):
            k, s = RH.line_key(ln), int(source.a[i])
            t = 0 if times is None else int(times.a[i])
            K, T = self.dev.get(s, (None, None))
            r = K is not None and k == K and (times is None or t - T <= window_us)
            repeat.a[i] = int(r)
            self.dev[s] = (k, T if r else t)
            table[s]["last"] = i
            table[s]["valid"] = 1


@pytest.fixture
def sstub(rstub):  # noqa: F811
    eng = SourcesEngine()
    eng.log = rstub.log
    return eng


@pytest.mark.parametrize("window", [None, 2.0])
@pytest.mark.parametrize("lag", [1, 3])
def test_stream_collect_per_source(sstub, lag, window):
    eng = sstub
    parser = RH.RepeatParser(eng)
    kw = {} if window is None else {"repeat_window": window}
    ls = stream.LineStream(parser, chunk_lines=16, chunk_bytes=4096, output="json", lag=lag, collapse_repeats=True,
                           repeat_sources=3, **kw)
    assert eng.state_args == (False, 3)
    seq = RH.scripted_lines()
    rng = np.random.default_rng(8)
    srcs = rng.integers(0, 3, len(seq)).tolist()
    clock, times = {0: 0, 1: -10_000_000, 2: 10_000_000}, []
    for s in srcs:
        clock[s] += int(rng.choice([0, 400_000, 900_000, 2_000_001]))
        times.append(clock[s])
    for a in range(0, len(seq), 16):
        ls.submit(seq[a: a + 16], sources=srcs[a: a + 16], **({} if window is None else {"times": times[a: a + 16]}))
    got = [r.detach() for r in ls.drain()]
    keys = [RH.line_key(x) for x in seq]
    w = None if window is None else W
    exp = restate(keys, srcs, times, w)
    assert exp != RH.restate(keys) and exp != restate(keys, srcs, times, W if w is None else None)
    assert [m for r in got for m in r.repeat.tolist()] == exp
    assert [t for r in got for t in r.texts()] == [None if m else RH.line_text(x) for m, x in zip(exp, seq)]
    assert [s for r in got for s in r.source.tolist()] == srcs and all(r.source.dtype == np.int32 for r in got)
    marks = [c for c in eng.calls if c[0] == "mark_src"]
    assert len(marks) == -(-len(seq) // 16) and not any(c[0] in ("mark", "mark_timed") for c in eng.calls)
    assert [int(x) for c in marks for x in c[3]] == srcs and all(c[6] == 3 for c in marks)   # the ids travelled
    if window is None:
        assert all(c[4] is None for c in marks)
    else:
        assert [int(x) for c in marks for x in c[4]] == times and all(c[5] == W for c in marks)
    assert ls.h2d_bytes >= (4 if window is None else 12) * len(seq)


def test_stream_refuses_bad_ids(sstub):
    eng = sstub
    parser = RH.RepeatParser(eng)
    seq = RH.scripted_lines()[:4]
    with pytest.raises(ValueError, match="collapse_repeats"):
        stream.LineStream(parser, chunk_lines=16, chunk_bytes=4096, repeat_sources=2)
    for bad in (0, 4097):
        with pytest.raises(ValueError):
            stream.LineStream(parser, chunk_lines=16, chunk_bytes=4096, collapse_repeats=True, repeat_sources=bad)
    ls = stream.LineStream(parser, chunk_lines=16, chunk_bytes=4096, output="json", lag=1, collapse_repeats=True,
                           repeat_window=2.0, repeat_sources=2)
    with pytest.raises(ValueError, match="sources"):
        ls.submit(seq, times=[1, 2, 3, 4])
    with pytest.raises(ValueError, match="3 ids for 4"):
        ls.submit(seq, times=[1, 2, 3, 4], sources=[0, 1, 0])
    with pytest.raises(ValueError, match=r"\[0, 2\)"):
        ls.submit(seq, times=[1, 2, 3, 4], sources=[0, 1, 2, 0])
    with pytest.raises(ValueError, match="times"):
        ls.submit(seq, sources=[0, 1, 0, 1])
    with pytest.raises(ValueError, match="decrease"):
        ls.submit(seq, times=[5, 9, 4, 9], sources=[0, 1, 0, 1])
    ls.submit(seq, times=[5, 1, 6, 2], sources=[0, 1, 0, 1])          # decreasing across the sources only
    with pytest.raises(ValueError, match="decrease"):
        ls.submit(seq, times=[6, 1, 6, 2], sources=[0, 1, 0, 1])      # source 1 starts before its last time
    ls.submit(seq, times=[6, 2, 6, 2], sources=[0, 1, 0, 1])
    with pytest.raises(ValueError, match="source"):
        ls.submit_bytes(b"MU;x;\n", time=7)
    with pytest.raises(ValueError, match="source"):
        ls.submit_bytes(b"MU;x;\n", time=7, source=2)
    with pytest.raises(ValueError, match="decrease"):
        ls.submit_bytes(b"MU;x;\n", time=5, source=0)
    assert ls._last_times == {0: 6, 1: 2}                             # a refused call moves no source's clock
    ls.drain()
    assert [c[1] for c in eng.calls if c[0] == "mark_src"] == [4, 4]  # nothing of the refused calls was launched
    plain = stream.LineStream(parser, chunk_lines=16, chunk_bytes=4096, output="json", lag=1, collapse_repeats=True)
    with pytest.raises(ValueError, match="repeat_sources"):
        plain.submit(seq, sources=[0, 0, 0, 0])
    with pytest.raises(ValueError, match="repeat_sources"):
        plain.submit_bytes(b"MU;x;\n", source=0)


@pytest.mark.parametrize("window", [None, 2.0])
def test_submit_bytes_keeps_one_tail_and_one_clock_per_source(sstub, monkeypatch, window):
    """Read buffers of different receivers, handed over alternately, each ending inside a line: a tail is
    glued to the next buffer of ITS source; a line gets its source's id and the time of the buffer of that
    source that holds its newline.  Stage A is cut off: the pieces, their ids and times are recorded."""
    eng = sstub
    kw = {} if window is None else {"repeat_window": window}
    ls = stream.LineStream(RH.RepeatParser(eng), chunk_lines=3, chunk_bytes=4096, output="json", lag=1,
                           collapse_repeats=True, repeat_sources=3, **kw)
    pieces = []

    def stage_a_bytes(s, carry, pinned_buf, arr, lo, hi, final):
        pieces.append((bytes(carry) + arr[lo:hi].tobytes(), s.n, s.sources.tolist(), s.h_src.numpy()[: s.n].tolist(),
                       None if s.times is None else s.times.tolist()))

    def queued(s):
        s.reset()
        s.stage = 0
        return s.cid
    monkeypatch.setattr(ls, "_stage_a_bytes", stage_a_bytes)
    monkeypatch.setattr(ls, "_queued", queued)
    tm = (lambda t: {"time": t}) if window is not None else (lambda t: {})
    ls.submit_bytes(b"aa\nbb\ncc", source=0, **tm(100))      # 'cc' is carried for source 0
    ls.submit_bytes(b"xx\ny", source=2, **tm(40))            # source 2 is behind in time; 'y' is carried for it
    ls.submit_bytes(b"c", source=0, **tm(150))               # no newline: nothing ends here
    ls.submit_bytes(b"y\nzz", source=2, **tm(60))            # 'yy' = source 2's tail + this buffer
    ls.submit_bytes(b"c\ndd\nee\nff\ngg\nhh", source=0, **tm(200))   # 'cccc'; five lines: two pieces
    ls.submit_bytes(b"", source=2, **tm(70))                 # an empty read
    assert bytes(ls._carries[0]) == b"hh" and bytes(ls._carries[2]) == b"zz" and not ls._carry
    ls.close_bytes()                                         # every tail, in id order: 'hh', then 'zz'
    assert not ls._carries[0] and not ls._carries[2]
    assert ls.close_bytes() == [] and ls.close_bytes(source=1) == []
    assert all(p[1] == len(p[0].rstrip(b"\n").split(b"\n")) <= 3 for p in pieces)
    assert all(len(set(p[2])) == 1 and p[2] == p[3] for p in pieces)    # one source per chunk, in the pinned buffer
    flat = [(ln, p[2][0], p[4][j] if p[4] else None) for p in pieces for j, ln in enumerate(p[0].rstrip(b"\n").split(b"\n"))]
    t = (lambda x: x) if window is not None else (lambda x: None)
    assert flat == [(b"aa", 0, t(100)), (b"bb", 0, t(100)), (b"xx", 2, t(40)), (b"yy", 2, t(60)), (b"cccc", 0, t(200)),
                    (b"dd", 0, t(200)), (b"ee", 0, t(200)), (b"ff", 0, t(200)), (b"gg", 0, t(200)), (b"hh", 0, t(200)),
                    (b"zz", 2, t(70))]
    # close_bytes(source=) flushes one source's tail only
    ls.submit_bytes(b"p", source=1, **tm(1))
    ls.submit_bytes(b"q", source=2, **tm(80))
    n0 = len(pieces)
    ls.close_bytes(source=2)
    assert [p[0] for p in pieces[n0:]] == [b"q"] and bytes(ls._carries[1]) == b"p"
