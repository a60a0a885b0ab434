"""Repeat suppression per receiver: sdx_mark_repeats_by_source and the ``sources`` /
``repeat_sources`` arguments of the front end and the stream.

Every line carries a source id; each source's subsequence of the stream is decided as a stream of its own.
The expected masks come from ``restate`` below, a serial restatement of that recurrence with one [K, T]
per source.  Its inputs are never taken from the code under test: the keys, ids and times the test planted
into hand-built launch outputs, or -- end to end -- the reference-recorded (kind, protocol_id, payload) of
the goldens and ids / times the test chose."""
import numpy as np
import pytest

from oracle import json_oracle as J

pytestmark = pytest.mark.gpu

W = 2_000_000


def restate(keys, srcs, times, w, carry=None):
    """keys[i]: the line's key or None, srcs[i]: its source id, times[i]: its time (ignored for w = None),
    w: the window (None: no window) -> the mask.  carry: dict source -> [K, T], updated in place."""
    carry = {} if carry is None else carry
    mask = []
    for k, s, t in zip(keys, srcs, times):
        K, T = carry.get(s, (None, None))
        rep = k is not None and K is not None and k == K and (w is None or t - T <= w)
        mask.append(int(rep))
        if k is not None:
            carry[s] = [k, T if rep else t]
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

    def mark_src(self, state, srcs, S, times=None, w=None, table=False):
        from pysignalduino_amd import runtime
        t = self.eng.torch
        rep, scratch = self.eng.alloc_repeat_sources(self.n, S)
        rep.fill_(9)   # every entry must be written
        sdev = t.from_numpy(np.asarray(srcs, np.int32).copy()).to(self.eng.dev)
        tdev = None if w is None else t.from_numpy(np.asarray(times, np.int64).copy()).to(self.eng.dev)
        self.eng.mark_repeats_by_source(self.ins, self.n, sdev, S, tdev, w, rep, scratch, state)
        mask = rep[: self.n].cpu().numpy().tolist()
        if table:
            tab = self.eng.repeat_sources_table(scratch, S).cpu().numpy().view(runtime.REPEAT_SOURCE_ENTRY)
            return mask, tab
        return mask

    def mark_timed(self, state, times, w):
        t = self.eng.torch
        rep, scratch = self.eng.alloc_repeat_timed(self.n)
        tdev = t.from_numpy(np.asarray(times, np.int64).copy()).to(self.eng.dev)
        self.eng.mark_repeats_timed(self.ins, self.n, tdev, w, rep, scratch, state)
        return rep[: self.n].cpu().numpy().tolist()

    def mark(self, state):
        rep, scratch = self.eng.alloc_repeat(self.n)
        self.eng.mark_repeats(self.ins, self.n, rep, scratch, state)
        return rep[: self.n].cpu().numpy().tolist()


def keys_of(items):
    return [None if it is None else (it[0], it[1], bytes(it[2])) for it in items]


_states = {}


def fresh_state(eng, S):
    """A zeroed state of S slots (one buffer per S, zeroed again: 4096 slots are 268 MB)."""
    if S not in _states:
        _states[S] = eng.alloc_repeat_state(sources=S)
    else:
        _states[S].zero_()
    return _states[S]


def check_chunks(eng, chunks, S, w):
    """chunks: [(items, srcs, times), ...] of one stream through sdx_mark_repeats_by_source with one carried
    state == restate over all lines; after every chunk the compact table holds every source's (K, T) and
    its last result-bearing line."""
    state = fresh_state(eng, S)
    carry = {}
    got, exp = [], []
    for items, srcs, times in chunks:
        assert len(items) == len(srcs) == len(times)
        if not items:
            continue
        m, tab = Planted(eng, items).mark_src(state, srcs, S, times, w, table=True)
        got += m
        keys = keys_of(items)
        exp += restate(keys, srcs, times, w, carry)
        assert len(tab) == S
        for s in set(srcs) | set(carry):
            last = max((i for i, (k, x) in enumerate(zip(keys, srcs)) if x == s and k is not None), default=-1)
            assert int(tab[s]["last"]) == last, (s, tab[s], last)
            if s in carry:
                K, T = carry[s]
                assert (int(tab[s]["valid"]), int(tab[s]["kind"]), int(tab[s]["proto"]), int(tab[s]["len"])) == \
                    (1, K[0], K[1], len(K[2])), (s, tab[s], K)
                if w is not None:
                    assert int(tab[s]["t"]) == T, (s, tab[s], T)
            else:
                assert int(tab[s]["valid"]) == 0
    assert got == exp, (S, w, [(i, g, e) for i, (g, e) in enumerate(zip(got, exp)) if g != e][:10])
    return got


A, B, C = (0, 1, b"aaaaaaaa"), (0, 1, b"bbbbbbbb"), (1, 1, b"aaaaaaaa")


def test_one_run_per_receiver(eng):
    # two sticks hear the same telegram: one publication per stick
    assert check_chunks(eng, [([A, A, A, A], [0, 1, 0, 1], [0, 0, 0, 0])], 2, None) == [0, 0, 1, 1]
    # another stick's telegram does not break a run
    assert check_chunks(eng, [([A, B, A], [0, 1, 0], [0, 0, 0])], 2, None) == [0, 0, 1]
    assert check_chunks(eng, [([A, B, A], [0, 1, 0], [0, 1, 2])], 2, W) == [0, 0, 1]
    # a late line of source 1 does not re-anchor source 0: its third A is 2.5 s behind ITS last published line
    items, srcs = [A, A, A, A, A], [0, 0, 1, 0, 1]
    times = [0, 1_500_000, 2_400_000, 2_500_000, 2_600_000]
    assert check_chunks(eng, [(items, srcs, times)], 2, W) == [0, 1, 0, 0, 1]
    # ... and an early one of source 1 does not let source 0's window run out
    assert check_chunks(eng, [([A, A, A], [0, 1, 0], [10 * W, 0, 10 * W + 5])], 2, W) == [0, 0, 1]


def _random_items(rng, n, none=0.3, stay=0.6):
    pool = [A, B, C]
    items = []
    for _ in range(n):
        if rng.random() < none:
            items.append(None)
        elif items and rng.random() < stay:
            items.append(next((x for x in reversed(items) if x is not None), A))
        else:
            items.append(pool[int(rng.integers(0, 3))])
    return items


def test_one_source_is_the_one_stream_entry(eng):
    rng = np.random.default_rng(2)
    items = _random_items(rng, 700, none=0.4)
    times = np.cumsum(rng.choice([0, W // 4, W // 2, W, W + 1], len(items))).tolist()
    p = Planted(eng, items)
    zeros = [0] * len(items)
    plain = p.mark(eng.alloc_repeat_state())
    assert sum(plain) > 100
    assert p.mark_src(fresh_state(eng, 1).clone(), zeros, 1) == plain
    st_t = eng.alloc_repeat_state(timed=True)
    st_s = fresh_state(eng, 1).clone()
    assert st_s.numel() == st_t.numel()
    for a, b in ((0, 300), (300, 700)):       # two chunks: the carried slot as well
        q = Planted(eng, items[a:b])
        timed = q.mark_timed(st_t, times[a:b], W)
        assert q.mark_src(st_s, zeros[a:b], 1, times[a:b], W) == timed
        assert st_s.cpu().numpy().tobytes() == st_t.cpu().numpy().tobytes()   # slot 0 is the timed state
    assert 0 < sum(timed) < 400


@pytest.mark.parametrize("n", [65, 257])     # one lane past a wave, one line past a tile
def test_three_modes_through_repeat_pass(eng, n):
    """repeats.RepeatPass drives each entry through alloc / enqueue.  Plain, timed with a window wider than
    all the times, and by source with S = 1 and that window are one definition: the same masks -- restate's
    -- over two chunks (the second starts from the carried state), and the same K in the three states."""
    from pysignalduino_amd import runtime
    from pysignalduino_amd.repeats import RepeatPass
    rng = np.random.default_rng(n)
    wide = 1 << 40
    passes = [RepeatPass(eng), RepeatPass(eng, window_us=wide), RepeatPass(eng, window_us=wide, n_sources=1)]
    carry, now = {}, 0
    for chunk in range(2):
        items = _random_items(rng, n)
        items[-1] = items[-1] or A                     # the next chunk's first lines depend on this chunk's state
        times = (now + np.cumsum(rng.integers(0, 1000, n))).astype(np.int64)
        now = int(times[-1])
        zeros = np.zeros(n, np.int32)
        p = Planted(eng, items)
        masks = []
        for rp in passes:
            b = rp.alloc(n, pinned=False)
            b.mask.fill_(9)                            # every entry must be written
            rp.enqueue(b, p.ins, n, times=times, sources=zeros)
            masks.append(b.mask[:n].cpu().numpy().tolist())
        exp = restate(keys_of(items), [0] * n, times.tolist(), None, carry)
        assert masks[0] == exp and masks[1] == exp and masks[2] == exp, chunk
        assert 0 < sum(exp) < n
    plain, timed, slot0 = (rp.state.cpu().numpy() for rp in passes)
    assert len(slot0) == len(timed)                    # S = 1: the one slot is a timed state
    hdr = runtime.REPEAT_SLOT_HDR
    K = plain[:16].view(np.uint32).tolist()
    ln = K[3]
    assert K[0] == 1 and (K[1], K[2], bytes(plain[16: 16 + ln])) == carry[0][0]
    for st in (timed, slot0):
        assert st[:16].view(np.uint32).tolist() == K and st[hdr: hdr + ln].tobytes() == plain[16: 16 + ln].tobytes()
    assert timed[16:24].view(np.int64)[0] == slot0[16:24].view(np.int64)[0]


def _id_patterns(n, S):
    rr = [i % S for i in range(n)]
    per = -(-n // S)
    blocks = [i // per for i in range(n)]
    single = [0] * n
    single[n // 2] = S - 1
    ends = [0 if i % 2 == 0 else S - 1 for i in range(n)]
    mid = [(S // 2) if i % 3 == 1 else (0 if i % 3 == 0 else S - 1) for i in range(n)]
    return [rr, blocks, single, ends, mid]


@pytest.mark.parametrize("S", [1, 2, 3, 255, 256, 257, 4096])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 513])
def test_scan_and_sort_boundaries(eng, n, S):
    rng = np.random.default_rng(1000 * S + n)
    items = _random_items(rng, n)
    times = np.cumsum(rng.choice([0, W // 4, W // 2, W, W + 1], n)).tolist()
    for srcs in _id_patterns(n, S):
        check_chunks(eng, [(items, srcs, times)], S, W)
        check_chunks(eng, [(items, srcs, times)], S, None)
    # stability: the last source's lines alternate two keys (none of them a repeat) across every wave and
    # tile boundary, between lines of source 0; two of its lines swapped by the sort would stand beside an
    # equal key, and the mask would flip
    other = S - 1
    srcs = [other if i % 2 else 0 for i in range(n)]
    alt = [((A, B)[(i // 2) % 2] if i % 2 else A) for i in range(n)]
    if S == 1:
        alt = [(A, B)[i % 2] for i in range(n)]
    got = check_chunks(eng, [(alt, srcs, [0] * n)], S, None)
    if S > 1:
        assert got == [int(i % 2 == 0 and i > 0) for i in range(n)]
    else:
        assert got == [0] * n


def test_carried_state_over_three_chunks(eng):
    S = 5
    c1 = ([A, A, B, A, C], [0, 1, 2, 0, 3], [10, 20, 30, 40, 50])
    # source 1 is absent from the middle chunk, source 2 is there only with lines without results, source 0
    # goes on, source 4 never appears
    c2 = ([None, A, None, None, A], [2, 0, 2, 3, 0], [60, 70, 80, 90, W + 41])
    c3 = ([A, B, C, A, B], [1, 2, 3, 0, 2], [W + 20, W + 30, W + 51, W + 60, W + 31])
    assert check_chunks(eng, [c1, c2, c3], S, W) == [0, 0, 0, 1, 0, 0, 1, 0, 0, 0, 1, 1, 0, 1, 0]
    assert check_chunks(eng, [c1, c2, c3], S, None) == [0, 0, 0, 1, 0, 0, 1, 0, 0, 1, 1, 1, 1, 1, 1]
    # a slot never touched stays all zero, payload room included; a touched one holds its payload
    from pysignalduino_amd import runtime
    st = _states[S].cpu().numpy()      # the state of the run just above
    slot = len(st) // S
    assert not st[4 * slot: 5 * slot].any()
    assert st[3 * slot + runtime.REPEAT_SLOT_HDR: 3 * slot + runtime.REPEAT_SLOT_HDR + 8].tobytes() == C[2]


def test_long_payloads_and_many_chunks(eng):
    # payloads longer than a wave's stride, equal up to the last byte; the slot's copy is exact
    long_a, long_b = (0, 3, b"x" * 700 + b"1"), (0, 3, b"x" * 700 + b"2")
    chunks = [([long_a, long_b], [0, 1], [0, 0]), ([long_a, long_a, long_b], [0, 1, 1], [1, 1, 2]),
              ([long_b, long_a], [1, 0], [3, 3])]
    assert check_chunks(eng, chunks, 2, None) == [0, 0, 1, 0, 0, 1, 1]


WINDOW_CASES = [([A, A], [0, W]), ([A, A], [0, W + 1]), ([A, A, A], [0, 1_500_000, 2_500_000]),
                ([A, A, A, A], [5, 5, 5, 5]), ([A, A, A, A], [5, 6, 7, 8]),
                ([A, B, A, A, A], [0, 1_000_000, 1_200_000, 3_000_000, 3_300_000]),
                ([A, A, A], [-(1 << 62), -(1 << 62) + W, 1 << 62])]
WINDOW_MASKS = {W: [[0, 1], [0, 0], [0, 1, 0], [0, 1, 1, 1], [0, 1, 1, 1],
                    [0, 0, 0, 1, 0], [0, 1, 0]],
                0: [[0, 0], [0, 0], [0, 0, 0], [0, 1, 1, 1], [0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0]]}


@pytest.mark.parametrize("w", [W, 0])
def test_window_edges_per_source(eng, w):
    for (items, times), want in zip(WINDOW_CASES, WINDOW_MASKS[w]):
        # the case on source 0 and on source 2, a second source's A lines between its lines: first with the
        # same times, then an hour EARLIER (times decrease across the sources, not within one)
        for mine, shift in ((0, 0), (2, 0), (0, -3_600_000_000), (2, -3_600_000_000)):
            it2, src2, t2 = [], [], []
            for x, t in zip(items, times):
                it2 += [x, A]
                src2 += [mine, 1]
                t2 += [t, t + shift]
            got = check_chunks(eng, [(it2, src2, t2)], 3, w)
            assert got[0::2] == want, (items, times, mine, shift)
            # the other source is the same case shifted, unless a B stands in its place
            if B not in items:
                assert got[1::2] == want
            # cut into two chunks at every place
            for cut in range(1, len(it2) if mine == 0 else 1):
                check_chunks(eng, [(it2[:cut], src2[:cut], t2[:cut]), (it2[cut:], src2[cut:], t2[cut:])], 3, w)


def test_long_orbits_per_source(eng):
    # two sources with 1,500 lines of one key each, gaps W / 3: orbits that cross tiles, dealt in blocks of 7
    n = 3000
    srcs = [(i // 7) % 2 for i in range(n)]
    times = [i * (W // 6) for i in range(n)]
    got = check_chunks(eng, [([A] * n, srcs, times)], 2, W)
    assert 400 < got.count(0) < 520
    # equal times in long stretches: an orbit that jumps over whole tiles
    times = [(i // 600) * W for i in range(n)]
    check_chunks(eng, [([A if i % 11 != 5 else None for i in range(n)], srcs, times)], 2, W)


@pytest.mark.parametrize("seed", range(20))
def test_random(eng, seed):
    rng = np.random.default_rng(300 + seed)
    n = int(rng.integers(1, 701))
    S = int(rng.choice([1, 4, 300]))
    w = [0, W, None][seed % 3]
    items = _random_items(rng, n)
    srcs = rng.integers(0, S, n).tolist()
    if seed % 2:       # bursts: a source keeps the line for a while
        for i in range(1, n):
            if rng.random() < 0.7:
                srcs[i] = srcs[i - 1]
    # times: non-decreasing within a source, each source on a clock of its own
    ww = w or W
    clock = {s: int(rng.integers(-10 * ww, 10 * ww)) for s in set(srcs)}
    times = []
    for s in srcs:
        clock[s] += int(rng.choice([0, ww // 4, ww // 2, ww, ww + 1, 3 * ww]))
        times.append(clock[s])
    cut = int(rng.integers(0, n + 1))
    check_chunks(eng, [(items[:cut], srcs[:cut], times[:cut]), (items[cut:], srcs[cut:], times[cut:])], S, w)


def test_refuses_bad_arguments(eng):
    p = Planted(eng, [A, A])
    t = eng.torch
    S = 3
    rep, scratch = eng.alloc_repeat_sources(2, S)
    _, scratch_max = eng.alloc_repeat_sources(2, 4096)
    rep.fill_(9)
    st = eng.alloc_repeat_state(sources=S)
    times = t.zeros(2, dtype=t.int64, device=eng.dev)
    ids = t.zeros(2, dtype=t.int32, device=eng.dev)
    with pytest.raises(RuntimeError, match="libsdx error -1: .*null buffer"):     # SDX_EINVAL
        eng.mark_repeats_by_source(p.ins, 2, None, S, times, W, rep, scratch, st)
    for bad in (0, 4097):
        with pytest.raises(RuntimeError, match="n_sources"):
            eng.mark_repeats_by_source(p.ins, 2, ids, bad, times, W, rep, scratch_max, st)
        with pytest.raises(ValueError):
            eng.alloc_repeat_state(sources=bad)
        with pytest.raises(ValueError):
            eng.alloc_repeat_sources(2, bad)
    with pytest.raises(RuntimeError, match="window_us"):
        eng.mark_repeats_by_source(p.ins, 2, ids, S, times, -1, rep, scratch, st)
    pad = t.zeros(st.numel() + 16, dtype=t.uint8, device=eng.dev)
    with pytest.raises(RuntimeError, match="aligned"):
        eng.mark_repeats_by_source(p.ins, 2, ids, S, times, W, rep, scratch, pad[8:])
    t.cuda.synchronize()
    assert rep[:2].cpu().numpy().tolist() == [9, 9]      # nothing was launched
    assert not st.cpu().numpy().any()
    # without times the window is not read
    eng.mark_repeats_by_source(p.ins, 2, ids, S, None, -1, rep, scratch, st)
    assert rep[:2].cpu().numpy().tolist() == [0, 1]
    # the Python layer refuses ids outside [0, S), before anything is launched
    from pysignalduino_amd.frontend import SignalParser
    from pysignalduino_amd.repeats import check_sources
    for bad in ([0, 3], [-1, 0], [0.5, 1.0], [0], [[0, 1]]):
        with pytest.raises(ValueError):
            check_sources(bad, 2, 3)
    for bad in ([-1, 0], [0, 4096], [0.0, 1.0]):      # one call: S = the largest id + 1, at most 4096
        with pytest.raises(ValueError):
            SignalParser().parse_lines_json(["MS;x", "MS;y"], collapse_repeats=True, sources=bad, times=[0, 0],
                                            repeat_window=2.0)
    with pytest.raises(ValueError):
        SignalParser().parse_lines_json(["MS;x", "MS;y"], sources=[0, 1])       # sources need collapse_repeats


# ---- end to end: goldens in bursts, dealt to three receivers -----------------------------------------
CH = 97   # the stream's chunk: smaller than most bursts' distance, so runs and windows cross chunks
NS = 3


@pytest.fixture(scope="module")
def corpus(golden):
    """Golden lines the current front end answers without ContractError, as three receivers deliver them:
    every telegram arrives four times within the window (0.3 s apart, noise lines between some) and once
    more 5 s later, general-path lines (resolved on the host) stand inside some bursts; neighbouring
    receivers hear the same telegrams, each on a clock of its own, and their lines are merged one by one, so
    that bursts of different sources interleave line by line -> (lines, keys, texts, times, sources)."""
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
    rng = np.random.default_rng(12)
    tele = [c for c in ok if c.get("e2e")][:130]
    per = []
    for sid in range(NS):
        rows = []
        now = [1_000_000 - 400_000_000 * sid]      # source 1 and 2 run behind: times decrease across sources

        def add(c, dt):
            now[0] += dt
            rows.append((c["line"].strip("\n"), e2e_key(c.get("e2e", [])), J.published(c.get("e2e", [])), now[0]))
        # sources 0 and 1 hear the same telegrams in the same order, source 2 every other one
        mine = tele if sid < 2 else tele[::2]
        for j, c in enumerate(mine):
            for r in range(4):
                add(c, 300_000 if r else 10_000)
                if rng.integers(0, 3) == 0:
                    add(noise[int(rng.integers(0, len(noise)))], 1_000)
                if j % 9 == 4 and r in (0, 2):
                    add(gen, 1_000)              # a general-path line inside the run
            if j % 13 == 6:
                add(gen, 1_000)
                add(gen, 2_100_000)              # general-path lines repeating each other, then past the window
            add(c, 5_000_000)
        per.append(rows)
    lines, keys, texts, times, sources = [], [], [], [], []
    for i in range(max(len(p) for p in per)):
        for sid in range(NS):
            if i < len(per[sid]):
                ln, k, tx, tm = per[sid][i]
                lines.append(ln), keys.append(k), texts.append(tx), times.append(tm), sources.append(sid)
    assert sum(k is not None for k in keys) > 1000
    assert any(b < a for a, b in zip(times, times[1:]))
    return lines, keys, texts, times, sources


def expect(keys, texts, times, sources, w):
    m = restate(keys, sources, times, w)
    return m, [None if x else t for x, t in zip(m, texts)]


def test_parse_lines_json_sources(corpus):
    from pysignalduino_amd.frontend import SignalParser
    lines, keys, texts, times, sources = corpus
    sp = SignalParser()
    m2, t2 = expect(keys, texts, times, sources, W)
    m0, t0 = expect(keys, texts, times, sources, None)
    one = restate(keys, [0] * len(keys), times, None)
    assert sum(m0) > sum(m2) > 700 and m0 != one     # one run per receiver is not one run per stream
    got = sp.parse_lines_json(lines, collapse_repeats=True, sources=sources, times=times, repeat_window=2.0)
    assert sp.last_repeat_mask.tolist() == m2
    assert got == t2
    assert sp.parse_lines_json(lines, collapse_repeats=True, sources=sources) == t0
    assert sp.last_repeat_mask.tolist() == m0
    with pytest.raises(ValueError):      # the merged times decrease: without ids they are refused
        sp.parse_lines_json(lines, collapse_repeats=True, times=times, repeat_window=2.0)
    bad = list(times)
    j = max(i for i, s in enumerate(sources) if s == 1)
    bad[j] = times[j] - 10_000_000       # a time that decreases within source 1
    with pytest.raises(ValueError):
        sp.parse_lines_json(lines, collapse_repeats=True, sources=sources, times=bad, repeat_window=2.0)


def test_parse_lines_objects_sources(corpus):
    from pysignalduino_amd.frontend import SignalParser
    lines, keys, texts, times, sources = corpus
    sp = SignalParser()
    plain = sp.parse_lines(lines)
    for w, kw in ((W, {"times": times, "repeat_window": 2.0}), (None, {})):
        got = sp.parse_lines(lines, collapse_repeats=True, sources=sources, **kw)
        m, _ = expect(keys, texts, times, sources, w)
        assert sp.last_repeat_mask.tolist() == m
        for x, g, p in zip(m, got, plain):
            assert g == [] if x else [(d.protocol_id, d.payload) for d in g] == [(d.protocol_id, d.payload) for d in p]
    with pytest.raises(ValueError):
        sp.parse_lines(lines, sources=sources)


@pytest.mark.parametrize("output", ["json", "wire"])
def test_stream_sources(corpus, output):
    from pysignalduino_amd.frontend import SignalParser
    lines, keys, texts, times, sources = corpus
    sp = SignalParser()
    n = len(lines)

    def run(feed, window):
        """-> per source: its lines' mask and texts in the order the stream returned them"""
        kw = {} if window is None else {"repeat_window": window}
        ls = sp.stream(chunk_lines=CH, chunk_bytes=1 << 18, output=output, lag=2, collapse_repeats=True,
                       repeat_sources=NS, **kw)
        feed(ls, window is not None)
        mask, got = {s: [] for s in range(NS)}, {s: [] for s in range(NS)}
        for r in ls.drain():
            assert r.repeat.dtype == np.uint8 and len(r.repeat) == r.n
            assert r.source.dtype == np.int32 and len(r.source) == r.n
            tx = r.texts() if output == "json" else [None] * r.n
            for s, m, x in zip(r.source.tolist(), r.repeat.tolist(), tx):
                mask[s].append(m)
                got[s].append(x)
        return mask, got

    def split(seq):
        return {s: [x for x, y in zip(seq, sources) if y == s] for s in range(NS)}

    def by_lines(ls, timed):
        for a in range(0, n, CH):
            ls.submit(lines[a: a + CH], sources=sources[a: a + CH], **({"times": times[a: a + CH]} if timed else {}))

    # bytes: every source's own byte stream in read buffers that end in the middle of a line, the sources'
    # buffers handed over alternately; a line has the time of the buffer holding its newline
    feeds, btimes = [], {}
    for s in range(NS):
        sl, st = split(lines)[s], split(times)[s]
        raw = [(ln + "\n").encode("latin-1") for ln in sl]
        ends = np.cumsum([len(x) for x in raw])
        blob = b"".join(raw)
        cuts = sorted({0, len(blob)} | {int(e) - 3 - s for e in ends[17 + s::23]} | {int(e) for e in ends[200::97]})
        bt = {}
        for a, b in zip(cuts, cuts[1:]):
            last = int(np.searchsorted(ends, b, side="right")) - 1          # the last line that ends inside [.., b)
            bt[(a, b)] = st[last] if last >= 0 else st[0]
            feeds.append((a, s, blob[a:b], bt[(a, b)]))
        btimes[s] = [bt[(cuts[j - 1], cuts[j])] for j in (int(np.searchsorted(cuts, int(e), side="left")) for e in ends)]
        assert all(y >= x for x, y in zip(btimes[s], btimes[s][1:])) and btimes[s] != st
    order = sorted(range(len(feeds)), key=lambda i: (feeds[i][0] // 4096, feeds[i][1], feeds[i][0]))

    def by_bytes(ls, timed):
        for i in order:
            _, s, buf, tm = feeds[i]
            ls.submit_bytes(buf, source=s, **({"time": tm} if timed else {}))
        ls.close_bytes()

    skeys, stexts, stimes = split(keys), split(texts), split(times)
    for feed, tt in ((by_lines, stimes), (by_bytes, btimes)):
        for window, w in ((2.0, W), (None, None)):
            mask, got = run(feed, window)
            for s in range(NS):
                m, t = expect(skeys[s], stexts[s], tt[s], [s] * len(skeys[s]), w)
                assert mask[s] == m, (feed.__name__, window, s)
                if output == "json":
                    assert got[s] == t, (feed.__name__, window, s)
    # ids are part of the stream's contract in both directions
    ls = sp.stream(chunk_lines=CH, output=output, collapse_repeats=True, repeat_sources=NS)
    with pytest.raises(ValueError):
        ls.submit(lines[:5])
    with pytest.raises(ValueError):
        ls.submit(lines[:5], sources=[0, 1, 2, 3, 0])
    with pytest.raises(ValueError):
        ls.submit_bytes(b"MS;x\n")
    ls = sp.stream(chunk_lines=CH, output=output, collapse_repeats=True)
    with pytest.raises(ValueError):
        ls.submit(lines[:5], sources=[0] * 5)
    with pytest.raises(ValueError):
        ls.submit_bytes(b"MS;x\n", source=0)
