"""Repeat suppression with a time window on the device: sdx_mark_repeats_timed and the
``repeat_window`` / ``times`` arguments of the front end and the stream.

The expected masks come from ``restate`` below, a serial restatement of the recurrence.  Its inputs are
never taken from the code under test: the keys and times the test planted into hand-built launch outputs,
or -- end to end -- the reference-recorded (kind, protocol_id, payload) of the goldens and times the test
chose."""
import numpy as np
import pytest

from oracle import json_oracle as J

pytestmark = pytest.mark.gpu

W = 2_000_000


def restate(keys, times, w, carry=None):
    """keys[i]: the line's key or None, times[i]: its time, w: the window (None: no window) -> the mask.
    carry: [K, T] of the stream so far, updated in place."""
    K, T = carry if carry is not None else (None, None)
    mask = []
    for k, t in zip(keys, times):
        rep = k is not None and K is not None and k == K and (w is None or t - T <= w)
        mask.append(int(rep))
        if k is not None:
            K, T = k, (T if rep else t)
    if carry is not None:
        carry[:] = [K, T]
    return mask


def e2e_key(e2e):
    """(kind, protocol_id, payload) of the reference's decoded[0]; None when it decoded nothing."""
    return (e2e[0][3][1], e2e[0][0], e2e[0][1]) if e2e else None


# ---- kernel level: hand-built launch outputs ------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    from pysignalduino_amd.sd_protocols import SDProtocols
    return SDProtocols()._ensure()


class Planted:
    """Launch outputs (descriptors, records, heap) of up to four kinds holding the given per-line results.
    items[i]: None, or (kind, proto, payload); every payload is followed by a byte that differs from line
    to line, so a compare that ran past a payload's end would see it."""

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
                desc[i] = (len(recs), 1, runtime.ST_OK, 0)
                recs.append((len(heap), len(it[2]), it[1], 0, i))
                heap += it[2] + bytes([(7 * i + 1) & 0xFF])
            rec = np.array(recs, runtime.RES_DT) if recs else np.zeros(1, runtime.RES_DT)
            dev = lambda a: t.from_numpy(np.frombuffer(a.tobytes() if hasattr(a, "tobytes") else bytes(a),  # noqa: E731
                                                       np.uint8).copy()).to(eng.dev)
            out = {"desc": dev(desc), "rec": dev(rec), "heap": dev(heap), "rec_cap": len(rec),
                   "cursor": t.zeros(4, dtype=t.int32, device=eng.dev)}
            self.keep.append(out)
            self.ins.append(eng.json_in(kd, out, {"meta": dummy}, n))

    def mark_timed(self, state, times, w):
        t = self.eng.torch
        rep, scratch = self.eng.alloc_repeat_timed(self.n)
        rep.fill_(9)   # every entry must be written
        tdev = t.from_numpy(np.asarray(times, np.int64).copy()).to(self.eng.dev)
        self.eng.mark_repeats_timed(self.ins, self.n, tdev, w, rep, scratch, state)
        return rep[: self.n].cpu().numpy().tolist()

    def mark(self, state):
        rep, scratch = self.eng.alloc_repeat(self.n)
        rep.fill_(9)
        self.eng.mark_repeats(self.ins, self.n, rep, scratch, state)
        return rep[: self.n].cpu().numpy().tolist()


def keys_of(items):
    return [None if it is None else (it[0], it[1], bytes(it[2])) for it in items]


def check_chunks(eng, chunks, w):
    """chunks: [(items, times), ...] of one stream through sdx_mark_repeats_timed with one carried state
    == restate over all lines."""
    state = eng.alloc_repeat_state(timed=True)
    got = []
    for items, times in chunks:
        assert len(items) == len(times)
        got += Planted(eng, items).mark_timed(state, times, w) if items else []
    keys = keys_of([it for items, _ in chunks for it in items])
    times = [int(t) for _, ts in chunks for t in ts]
    exp = restate(keys, times, w)
    assert got == exp, (w, [(i, g, e) for i, (g, e) in enumerate(zip(got, exp)) if g != e][:10])
    return got


A, B, C = (0, 1, b"aaaaaaaa"), (0, 1, b"bbbbbbbb"), (1, 1, b"aaaaaaaa")


def test_window_edges(eng):
    assert check_chunks(eng, [([A, A], [0, W])], W) == [0, 1]              # a gap of exactly W is a repeat
    assert check_chunks(eng, [([A, A], [0, W + 1])], W) == [0, 0]          # W + 1 is published
    assert check_chunks(eng, [([A, A, A], [0, 1_500_000, 2_500_000])], W) == [0, 1, 0]   # anchored at the published line
    assert check_chunks(eng, [([A, A, A, A], [5, 5, 5, 5])], 0) == [0, 1, 1, 1]           # W = 0, equal times
    assert check_chunks(eng, [([A, A, A, A], [5, 6, 7, 8])], 0) == [0, 0, 0, 0]           # W = 0, increasing times
    # a key change inside the window is published and re-anchors T: the A at 3.0 s and the one at 3.3 s
    # count from the A at 1.2 s, published behind B, not from the first A
    assert check_chunks(eng, [([A, B, A, A, A], [0, 1_000_000, 1_200_000, 3_000_000, 3_300_000])], W) == [0, 0, 0, 1, 0]
    # times far from zero and negative, the difference taken exactly
    big = (1 << 62)
    assert check_chunks(eng, [([A, A, A], [-big, -big + W, big])], W) == [0, 1, 0]


def test_wide_window_is_mark_repeats(eng):
    rng = np.random.default_rng(2)
    pool = [A, B, C, None, None]
    items = [pool[int(i)] for i in rng.integers(0, len(pool), 700)]
    for i in range(1, len(items)):
        if rng.random() < 0.6:
            items[i] = items[i - 1]
    times = np.cumsum(rng.integers(0, 1000, len(items))).tolist()
    p = Planted(eng, items)
    plain = p.mark(eng.alloc_repeat_state())
    assert sum(plain) > 100
    for w in (times[-1] - times[0], times[-1] - times[0] + 1, 1 << 62):
        assert p.mark_timed(eng.alloc_repeat_state(timed=True), times, w) == plain


def _interleave(n, head_at, gap_at):
    """n lines of key A / B with None at every 5th line (never at a listed position): a key change at
    each of head_at, a gap of W + 1 in front of each of gap_at, gaps of W / 4 elsewhere."""
    items, times, t, cur = [], [], 0, 0
    for i in range(n):
        if i in head_at:
            cur ^= 1
        t += W + 1 if i in gap_at else W // 4
        items.append(None if (i % 5 == 4 and i not in head_at and i not in gap_at) else (A, B)[cur])
        times.append(t)
    return items, times


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 513])
def test_scan_boundaries(eng, n):
    edges = [0, 63, 64, 255, 256, 511, 512]
    cases = [_interleave(n, set(), set()),
             _interleave(n, set(edges), set()),                       # heads by key on lanes 0 / 63, tile edges
             _interleave(n, set(), set(edges)),                       # heads by gap there
             _interleave(n, {x - 1 for x in edges if x}, {x + 1 for x in edges}),
             _interleave(n, {62, 254}, {66, 258})]
    # anchors (published lines inside a segment) on those lanes: one key, the gaps chosen so that the
    # window runs out exactly there
    for e in edges:
        if 0 < e < n:
            times = [0 if i < e - 1 else W // 2 + 1 if i == e - 1 else W + 1 + (i - e) for i in range(n)]
            cases.append(([A if i % 7 != 3 or i in (e - 1, e) else None for i in range(n)], times))
    for items, times in cases:
        check_chunks(eng, [(items, times)], W)
        check_chunks(eng, [(items, times)], 0)


def test_long_segments(eng):
    # one 700-line segment over three tiles that publishes about every 7th line, between two other keys
    gap = W // 6 - 1
    items = [B] * 40 + [A if i % 11 != 5 else None for i in range(700)] + [B] * 30
    times = np.cumsum([gap] * len(items)).tolist()
    got = check_chunks(eng, [(items, times)], W)
    assert 90 <= got[40:740].count(0) - sum(it is None for it in items) <= 110
    # 3,000 lines of a single key, every gap W / 3
    n = 3000
    times = [i * (W // 3) for i in range(n)]
    got = check_chunks(eng, [([A] * n, times)], W)
    assert got.count(0) == 750
    # the same with equal times in long stretches: an orbit that jumps over whole tiles
    times = [(i // 600) * W for i in range(n)]
    assert check_chunks(eng, [([A] * n, times)], W).count(0) == 3


def test_carried_state(eng):
    rng = np.random.default_rng(9)
    pool = [A, A, A, B, None]
    items = [pool[int(i)] for i in rng.integers(0, len(pool), 40)]
    items[10:22] = [A] * 12                                               # a segment the cuts fall into
    times = np.cumsum(rng.choice([0, W // 4, W // 2, W, W + 1], 40)).tolist()
    times[10:22] = [times[9] + (i + 1) * (W // 3) for i in range(12)]
    times[22:] = [x - times[22] + times[21] + W // 3 for x in times[22:]]
    assert all(b >= a for a, b in zip(times, times[1:]))
    for cut in range(0, 41):
        check_chunks(eng, [(items[:cut], times[:cut]), (items[cut:], times[cut:])], W)
        check_chunks(eng, [(items[:cut], times[:cut]), ([None] * 3, [times[max(cut - 1, 0)]] * 3),
                           (items[cut:], times[cut:])], W)
    # a fresh state has no K; a used one carries K and T; T stays when a chunk published nothing
    st = eng.alloc_repeat_state(timed=True)
    assert Planted(eng, [A, A]).mark_timed(st, [10, 20], W) == [0, 1]
    assert Planted(eng, [A]).mark_timed(st, [W], W) == [1]
    assert Planted(eng, [A]).mark_timed(st, [W + 10], W) == [1]         # T is still 10
    assert Planted(eng, [A]).mark_timed(st, [W + 11], W) == [0]
    assert Planted(eng, [A]).mark_timed(eng.alloc_repeat_state(timed=True), [W + 12], W) == [0]


@pytest.mark.parametrize("seed", range(20))
def test_random(eng, seed):
    rng = np.random.default_rng(100 + seed)
    n = int(rng.integers(1, 2001))
    w = int(rng.choice([W, 12, 1_000_003]))
    pool = [A, B, C]
    items = []
    for i in range(n):
        if rng.random() < 0.3:
            items.append(None)
        elif items and rng.random() < 0.8:
            items.append(next((x for x in reversed(items) if x is not None), A))
        else:
            items.append(pool[int(rng.integers(0, 3))])
    times = np.cumsum(rng.choice([0, w // 4, w // 2, w, w + 1, 3 * w], n)).tolist()
    cuts = sorted(set(int(x) for x in rng.integers(0, n + 1, int(rng.integers(0, 3)))))
    bounds = [0] + cuts + [n]
    check_chunks(eng, [(items[a:b], times[a:b]) for a, b in zip(bounds, bounds[1:])], w)


def test_refuses_bad_arguments(eng):
    p = Planted(eng, [A, A])
    t = eng.torch
    rep, scratch = eng.alloc_repeat_timed(2)
    rep.fill_(9)
    st = eng.alloc_repeat_state(timed=True)
    times = t.zeros(2, dtype=t.int64, device=eng.dev)
    with pytest.raises(RuntimeError, match="libsdx error -1: .*null buffer"):     # SDX_EINVAL
        eng.mark_repeats_timed(p.ins, 2, None, W, rep, scratch, st)
    with pytest.raises(RuntimeError, match="window_us"):
        eng.mark_repeats_timed(p.ins, 2, times, -1, rep, scratch, st)
    pad = t.zeros(st.numel() + 16, dtype=t.uint8, device=eng.dev)
    with pytest.raises(RuntimeError, match="aligned"):
        eng.mark_repeats_timed(p.ins, 2, times, W, rep, scratch, pad[8:])
    t.cuda.synchronize()
    assert rep[:2].cpu().numpy().tolist() == [9, 9]      # nothing was launched
    assert not st[:24].cpu().numpy().any()



# ---- end to end: goldens in bursts -------------------------------------------------------------------
CH = 97   # the stream's chunk: smaller than most bursts' distance, so runs and windows cross chunks


@pytest.fixture(scope="module")
def corpus(golden):
    """Golden lines the current front end answers without ContractError.  Every telegram arrives four
    times within the window (0.3 s apart, noise lines between some) and the same telegram once more 5 s
    later; general-path lines (resolved on the host) stand inside some bursts
    -> (lines, keys, texts, times)."""
    from pysignalduino_amd.frontend import SignalParser
    cases = [c for c in golden("lines_golden.json.gz") if "\n" not in c["line"].strip("\n")]
    plain = SignalParser().parse_lines_json([c["line"] for c in cases])
    ok = [c for c, g in zip(cases, plain) if not isinstance(g, Exception)]
    bearing = [c for c in cases if c.get("e2e")]
    lost = [c for c, g in zip(cases, plain) if isinstance(g, Exception) and c.get("e2e")]
    assert len(lost) <= 0.05 * len(bearing), (len(lost), len(bearing))   # the cap test_lines.py allows
    noise = [c for c in ok if not c.get("e2e")]
    gen = next(c for c in golden("lines_general_golden.json.gz")
               if c.get("e2e") and "P10=" in c["line"] and "\n" not in c["line"].strip("\n") and len(c["line"]) < 2000)
    rng = np.random.default_rng(11)
    lines, keys, texts, times = [], [], [], []
    now = [1_000_000]

    def add(c, dt):
        now[0] += dt
        lines.append(c["line"].strip("\n"))
        keys.append(e2e_key(c.get("e2e", [])))
        texts.append(J.published(c.get("e2e", [])))
        times.append(now[0])
    tele = [c for c in ok if c.get("e2e")][:260]
    for j, c in enumerate(tele):
        for r in range(4):
            add(c, 300_000 if r else 10_000)
            if rng.integers(0, 3) == 0:
                add(noise[int(rng.integers(0, len(noise)))], 1_000)
            if j % 9 == 4 and r in (0, 2):
                add(gen, 1_000)              # a general-path line inside the timed run
        if j % 13 == 6:
            add(gen, 1_000)
            add(gen, 2_100_000)              # general-path lines repeating each other, then past the window
        add(c, 5_000_000)
    assert sum(k is not None for k in keys) > 1000
    return lines, keys, texts, times


def expect(keys, texts, times, w):
    m = restate(keys, times, w)
    return m, [None if x else t for x, t in zip(m, texts)]


def test_parse_lines_json_window(corpus):
    from pysignalduino_amd.frontend import SignalParser
    lines, keys, texts, times = corpus
    sp = SignalParser()
    m2, t2 = expect(keys, texts, times, W)
    m0, t0 = expect(keys, texts, times, None)
    assert sum(m0) > sum(m2) > 700      # the second bursts are published only with the window
    got = sp.parse_lines_json(lines, collapse_repeats=True, times=times, repeat_window=2.0)
    assert sp.last_repeat_mask.tolist() == m2
    assert got == t2
    assert sp.parse_lines_json(lines, collapse_repeats=True) == t0     # no window: both bursts give one text
    assert sp.last_repeat_mask.tolist() == m0
    assert sp.parse_lines_json(lines, collapse_repeats=True, times=times, repeat_window=None) == t0


def test_parse_lines_objects_window(corpus):
    from pysignalduino_amd.frontend import SignalParser
    lines, keys, texts, times = corpus
    sp = SignalParser()
    plain = sp.parse_lines(lines)
    got = sp.parse_lines(lines, collapse_repeats=True, times=times, repeat_window=2.0)
    m2, _ = expect(keys, texts, times, W)
    assert sp.last_repeat_mask.tolist() == m2
    for m, g, p in zip(m2, got, plain):
        assert g == [] if m else [(d.protocol_id, d.payload) for d in g] == [(d.protocol_id, d.payload) for d in p]


@pytest.mark.parametrize("output", ["json", "wire"])
def test_stream_window(corpus, output):
    from pysignalduino_amd.frontend import SignalParser
    lines, keys, texts, times = corpus
    sp = SignalParser()
    n = len(lines)

    def run(feed, window):
        kw = {} if window is None else {"repeat_window": window}
        ls = sp.stream(chunk_lines=CH, chunk_bytes=1 << 18, output=output, lag=2, collapse_repeats=True, **kw)
        feed(ls, window is not None)
        mask, got = [], []
        for r in ls.drain():
            assert r.repeat.dtype == np.uint8 and len(r.repeat) == r.n
            mask += r.repeat.tolist()
            if output == "json":
                got += r.texts()
        return mask, got

    def by_lines(ls, timed):
        for a in range(0, n, CH):
            ls.submit(lines[a: a + CH], **({"times": times[a: a + CH]} if timed else {}))

    # bytes: read buffers that end in the middle of a line; a line has the time of the buffer holding its
    # newline, so the expected times are built from the buffers here, not from ``times``
    raw = [(ln + "\n").encode("latin-1") for ln in lines]
    ends = np.cumsum([len(x) for x in raw])
    blob = b"".join(raw)
    cuts = sorted({0, len(blob)} | {int(e) - 3 for e in ends[37::41]} | {int(e) for e in ends[500::97]})
    buf_time = {}
    btimes = []
    for a, b in zip(cuts, cuts[1:]):
        last = int(np.searchsorted(ends, b, side="right")) - 1          # the last line that ends inside [.., b)
        buf_time[(a, b)] = times[last] if last >= 0 else times[0]
    for i, e in enumerate(ends):
        j = int(np.searchsorted(cuts, int(e), side="left"))             # the buffer (cuts[j-1], cuts[j]] holding the newline
        btimes.append(buf_time[(cuts[j - 1], cuts[j])])
    assert all(y >= x for x, y in zip(btimes, btimes[1:])) and btimes != times

    def by_bytes(ls, timed):
        for a, b in zip(cuts, cuts[1:]):
            ls.submit_bytes(blob[a:b], **({"time": buf_time[(a, b)]} if timed else {}))
        ls.close_bytes()

    for feed, tt in ((by_lines, times), (by_bytes, btimes)):
        m2, t2 = expect(keys, texts, tt, W)
        mask, got = run(feed, 2.0)
        assert mask == m2
        if output == "json":
            assert got == t2
    m0, t0 = expect(keys, texts, times, None)
    mask, got = run(by_lines, None)
    assert mask == m0
    if output == "json":
        assert got == t0
