"""LineStream.submit_bytes (pysignalduino_amd/stream.py): a transport's raw bytes in, split into lines on
the device, the unterminated tail carried from call to call -- what StreamReader.readline() does in the
reference (signalduino/transport.py:113-123).

CPU: cut_bytes (the host's only look at the bytes: rfind / count) against a plain loop, and the
submit_bytes state machine on the numpy stand-ins and the scripted engine of tests/test_stream_host.py,
whose split_lines is np.flatnonzero.  GPU: the real stream on the reference-recorded lines, fed in ragged
pieces, against submit(lines)."""
import numpy as np
import pytest

import test_stream_host as H
from pysignalduino_amd import stream

stubbed = H.stubbed     # the fixture: torch, LineBatch and the copies replaced by numpy stand-ins


# ---- cut_bytes ---------------------------------------------------------------------------------------------
def _random_buffer(rng, nlines, maxlen, tail):
    parts = []
    for _ in range(nlines):
        k = int(rng.integers(0, maxlen + 1))
        parts.append(bytes(int(x) if x != 10 else 11 for x in rng.integers(0, 256, k)) + b"\n")
    return b"".join(parts) + bytes(65 + int(x) % 26 for x in rng.integers(0, 26, tail))


def _newlines(buf, lo, hi):
    return [p for p in range(lo, hi) if buf[p] == 10]     # byte by byte: the test's own count


@pytest.mark.parametrize("maxlen,C,B", [(300, 7, 512), (40, 7, 64), (300, 1000, 301), (5, 3, 4096)])
def test_cut_bytes_against_a_plain_loop(maxlen, C, B):
    rng = np.random.default_rng(maxlen + C)
    for trial in range(12):
        buf = _random_buffer(rng, int(rng.integers(0, 120)), maxlen, tail=int(rng.integers(0, 30)) * (trial % 2))
        nls = _newlines(buf, 0, len(buf))
        end = nls[-1] + 1 if nls else 0
        for view in (buf, stream._NlView(np.frombuffer(buf, np.uint8))):
            carry = int(rng.integers(0, B - maxlen)) if trial % 3 == 0 else 0    # a carried line start: first piece only
            lo, pieces = 0, []
            while True:
                hi, n = stream.cut_bytes(view, lo, carry, C, B)
                if hi == lo:
                    assert n == 0
                    break
                assert hi > lo and buf[hi - 1] == 10                      # ends on a newline
                assert n == len(_newlines(buf, lo, hi)) and 1 <= n <= C    # the line capacity
                assert carry + hi - lo <= B                                # the byte capacity
                if n < C and hi < end and n == len(pieces) == 0:           # not halved: the next line did not fit
                    nxt = next(p for p in nls if p >= hi) + 1
                    assert carry + nxt - lo > B or len(_newlines(buf, lo, nxt)) > C
                pieces.append(buf[lo:hi])
                lo, carry = hi, 0
            assert b"".join(pieces) == buf[:end] and lo == end            # the input minus its tail


def test_cut_bytes_refuses_a_line_longer_than_the_chunk():
    line = b"x" * 100 + b"\n"
    assert stream.cut_bytes(line, 0, 0, 7, 101) == (101, 1)
    with pytest.raises(ValueError):
        stream.cut_bytes(line, 0, 0, 7, 100)
    with pytest.raises(ValueError):
        stream.cut_bytes(line, 0, 1, 7, 101)                   # the carried start counts
    with pytest.raises(ValueError):
        stream.cut_bytes(b"a\n" + b"y" * 65, 2, 0, 7, 64)      # no newline within the next 64 bytes
    assert stream.cut_bytes(b"a\n" + b"y" * 64, 2, 0, 7, 64) == (2, 0)   # a tail that still fits


# ---- the state machine on stand-ins -------------------------------------------------------------------------
@pytest.fixture
def eng(stubbed):
    """The scripted engine with sdx_split_lines by np.flatnonzero (``skew`` falsifies its count)."""
    e = stubbed
    e.skew = 0
    e.splits = []

    def split_work_ints(nbytes):
        return max(1, -(-int(nbytes) // 16384))

    def split_lines(bytes_t, nbytes, final, offsets_t, cap, count_t, scratch_t, stream=None):
        ends = np.flatnonzero(bytes_t.a[:nbytes] == 10) + 1
        last = int(ends[-1]) if len(ends) else 0
        if final and last < nbytes:
            ends, last = np.append(ends, nbytes), nbytes
        k = min(len(ends), cap)
        offsets_t.a[0] = 0
        offsets_t.a[1: k + 1] = ends[:k]
        count_t.a[:] = (len(ends) + e.skew, last)
        e.splits.append((nbytes, bool(final), cap))
    e.split_work_ints, e.split_lines = split_work_ints, split_lines
    return e


def _per_line(results, output):
    """Per line of the whole feed: (raw line without its terminator, kind, status, what the line yields)."""
    rows = []
    for r in results:
        texts = r.texts() if output == "json" else None
        raw = r.lines()
        assert len(raw) == r.n
        for i in range(r.n):
            if output == "json":
                t = texts[i]
                if isinstance(t, str) and not t.startswith("host:"):
                    kind, idx = t.split(":")
                    assert int(idx) == i          # the device text names the line's index in ITS chunk
                    t = kind
                elif isinstance(t, str):
                    t = t.rstrip("\n")
            else:
                t = [(a, b.rstrip("\n")) for a, b in r.host[i]] if i in r.host else None
            rows.append((raw[i].rstrip(b"\n"), int(r.kind[i]), int(r.status[i]), t))
    return rows


def _feed(ls, pieces, final_last=False):
    got, ids = [], []
    for j, p in enumerate(pieces):
        ids += ls.submit_bytes(p, final=final_last and j == len(pieces) - 1)
        got += [r.detach() for r in ls.poll()]
    got += [r.detach() for r in ls.drain()]
    assert [r.id for r in got] == ids == list(range(len(ids)))
    return got


@pytest.mark.parametrize("output", ["json", "wire"])
def test_submit_bytes_state_machine(eng, output):
    """The same bytes as one call, byte by byte and in seeded ragged calls: the same per-line results as
    submit(lines), the lines cut into chunks within both capacities (a halving included), no offsets H2D."""
    lines = H._lines(260, seed=5)
    data = b"\n".join(lines) + b"\n"
    mk = lambda: stream.LineStream(H.FakeParser(eng), chunk_lines=50, chunk_bytes=50 * 32, output=output, lag=2)  # noqa: E731
    ref = mk()
    ref_got = []
    for k in range(0, len(lines), 50):
        ref.submit(lines[k: k + 50])
        ref_got += [r.detach() for r in ref.poll()]
    ref_got += [r.detach() for r in ref.drain()]
    exp = _per_line(ref_got, output)
    assert [x[0] for x in exp] == lines and any(x[3] is not None for x in exp)

    rng = np.random.default_rng(9)
    cuts = np.sort(rng.integers(0, len(data), 40))
    ragged = [data[a:b] for a, b in zip([0, *cuts], [*cuts, len(data)])]
    for pieces in ([data], [data[i: i + 1] for i in range(len(data))], ragged,
                   [bytearray(data)], [memoryview(data)], [np.frombuffer(data, np.uint8)]):
        eng.splits.clear()
        ls = mk()
        got = _feed(ls, pieces)
        assert _per_line(got, output) == exp
        assert all(r.n <= 50 for r in got) and all(nb <= 50 * 32 and cap <= 50 for nb, _, cap in eng.splits)
        assert len(eng.splits) == len(got) and not ls._carry
        assert ls.h2d_bytes == len(data)                   # the bytes only: no offsets go up
    # one call: 1600 bytes hold more than 50 of these lines, so the first cut is halved
    one = _feed(mk(), [data])
    assert len(one) > -(-len(lines) // 50) and max(r.n for r in one) <= 50


def test_submit_bytes_carries_the_tail(eng):
    ls = stream.LineStream(H.FakeParser(eng), chunk_lines=50, chunk_bytes=1600, output="json", lag=1)
    assert ls.submit_bytes(b"MU;D") == [] and ls.submit_bytes(b"=1") == [] and ls.submit_bytes(b"2;") == []
    assert ls.submit_bytes(b"\nMS;D=3;\nMC") == [0]          # a tail carried over three calls, then two lines
    assert ls.submit_bytes(b";D=4;") == []
    assert bytes(ls._carry) == b"MC;D=4;"
    assert ls.close_bytes() == [1] and ls.close_bytes() == []    # EOF: the tail is the last line, once
    a, b = ls.drain()
    assert a.lines() == [b"MU;D=12;\n", b"MS;D=3;\n"] and a.texts() == ["MU:0", "MS:1"]
    assert b.lines() == [b"MC;D=4;"] and b.texts() == ["MC:0"] and b.line(0) == b"MC;D=4;"
    assert eng.splits[-1] == (7, True, 1)
    # final=True with a trailing newline: nothing is left to flush
    assert ls.submit_bytes(b"MN;D=5;\n", final=True) == [2] and not ls._carry
    # ... and without one, in the same call: the terminated lines, then the tail as a chunk of its own
    assert ls.submit_bytes(b"MN;D=6;\nMU;D=7;", final=True) == [3, 4]
    got = ls.drain()
    assert [r.lines() for r in got] == [[b"MN;D=5;\n"], [b"MN;D=6;\n"], [b"MU;D=7;"]]
    # a line longer than chunk_bytes: refused, the chunk cut in front of it stays queued
    with pytest.raises(ValueError):
        ls.submit_bytes(b"MS;D=8;\n" + b"x" * 1601)
    (r,) = ls.drain()
    assert r.lines() == [b"MS;D=8;\n"] and not ls._carry
    with pytest.raises(ValueError):
        ls.submit_bytes(b"y" * 1000) or ls.submit_bytes(b"y" * 601)      # the carried start counts
    assert len(ls._carry) == 1000


def test_submit_bytes_checks_the_device_count(eng):
    ls = stream.LineStream(H.FakeParser(eng), chunk_lines=50, chunk_bytes=1600, output="json", lag=2)
    eng.skew = 1
    assert ls.submit_bytes(b"MU;D=1;\nMS;D=2;\n") == [0]
    with pytest.raises(RuntimeError, match="found 3 lines, the host counted 2"):
        ls.drain()
    eng.skew = 0
    assert not ls.inflight and ls.submit_bytes(b"MU;D=1;\n") == [1]      # the stream goes on
    (r,) = ls.drain()
    assert r.texts() == ["MU:0"]


# ---- GPU -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("output", ["json", "wire"])
def test_gpu_submit_bytes_equals_submit_lines(output, golden):
    """The reference-recorded lines tiled past GROUP_MIN, as raw bytes in ragged pieces (1 byte, 4096, a
    size that ends mid-line) through a stream small enough to force several chunks and a halving: every
    line's result equals submit(lines)'s, and ChunkResult.lines() gives the input back."""
    from pysignalduino_amd.frontend import SignalParser, lines_of
    from pysignalduino_amd.sd_protocols import SDProtocols
    base = [c["line"].encode("latin-1") for c in golden("lines_golden.json.gz")]
    # 12 tiles: half of them (what a halved cut holds) pass GROUP_MIN in both short classes, as the 5 tiles
    # of tests/test_stream.py's golden test do.  Most recorded lines end in a '\n' of their own, so every
    # other line of the feed is empty
    data = b"\n".join(base * 12).rstrip(b"\n")
    lines = lines_of(data)[0]
    n, nb = len(lines), len(data)
    assert data[-1] != 10 and n > 12 * len(base)   # the feed ends in an unterminated line
    sp = SignalParser(SDProtocols(mc_mode="fixed"))
    ref = sp.stream(chunk_lines=n, chunk_bytes=nb, output=output, lag=2)
    ref.submit(lines)
    (want,) = [r.detach() for r in ref.drain()]
    # chunk_bytes holds all the bytes but chunk_lines only half the lines: the big call's first cut is halved
    C = n // 2 + 1
    ls = sp.stream(chunk_lines=C, chunk_bytes=nb, output=output, lag=2)
    sizes = [1, 4096, 1000, nb]
    got, lo = [], 0
    for k in sizes:
        if k == 1000:
            assert data[lo + k - 1] != 10          # a piece that ends mid-line
        ls.submit_bytes(data[lo: lo + k], final=lo + k >= nb)
        lo += k
        got += [r.detach() for r in ls.poll()]
    got += [r.detach() for r in ls.drain()]
    assert len(got) >= 4 and sum(r.n for r in got) == n and n // 3 < max(r.n for r in got) <= C
    assert [ln for r in got for ln in r.lines()] == [ln + b"\n" for ln in lines[:-1]] + [lines[-1]]
    kind = np.concatenate([r.kind for r in got])
    status = np.concatenate([r.status for r in got])
    assert np.array_equal(kind, want.kind) and np.array_equal(status, want.status)
    if output == "json":
        exp, have = want.texts(), [t for r in got for t in r.texts()]
        assert len(exp) == len(have)
        for i, (e, g) in enumerate(zip(exp, have)):
            assert (type(g) is type(e)) if isinstance(e, Exception) else e == g, (i, e, g)
        assert sum(isinstance(e, str) for e in exp) > 2000
        return
    # wire: per line its (protocol id, payload) list, from the decoded records of the line's kind or, for
    # the lines the batch API took, from its objects (which of the two a line takes may differ with the
    # chunking: a kind whose results overflow a chunk's buffers goes to the batch API for that chunk)
    bk = sp.protocols._bank
    pid = {"MU": bk.mu_pids, "MS": bk.ms_pids, "MC": bk.mc_pids, "MN": bk.mn_pids}

    def per_line(r):
        rows = [[] for _ in range(r.n)]
        for j, nm in enumerate(r.names):
            d, rec, heap = r.decode(j)
            hs = heap.tobytes().decode("latin-1")
            for i in np.nonzero(d["n_rec"])[0].tolist():
                b, k = int(d[i]["rec_begin"]), int(d[i]["n_rec"])
                rows[i] += [(str(pid[nm][int(x["proto"])]), hs[int(x["payload_off"]): int(x["payload_off"]) + int(x["payload_len"])])
                            for x in rec[b: b + k]]
        for i, h in r.host.items():
            rows[i] = type(h) if isinstance(h, Exception) else [(m.protocol_id, m.payload) for m in h]
        return rows
    exp, have = per_line(want), [x for r in got for x in per_line(r)]
    assert exp == have
    assert sum(bool(e) for e in exp) > 2000
