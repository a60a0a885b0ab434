"""sdx_dispatch_records through the C ABI on planted launch outputs.

Expected values come from ``Chunk.expect``, the definition restated in Python over the records and heap bytes the
test itself planted and over rules the test itself packed (class indices, not protocol ids): per line the cap over
runs of one proto, then the equal-message drop against the last record that passed the cap; the kept records in
list order, compacted in line order; every other status keeps its descriptor's bytes.  Everything is compared byte
for byte: descriptors, whole record buffers (9s where nothing may be written, 0xA5 behind every declared capacity),
the four cursor words, and the heap (0xA5 behind its last payload byte), which the pass must leave alone."""
import ctypes

import numpy as np
import pytest

from test_routes import eng  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

OK, RAISED, OVF_TILE, OVF_OUT, ABSENT = 0, 1, 2, 3, 0xFF
EINVAL = -1
COUNTS = (129, 66, 12, 19)      # this bank's class counts (test_profiles_host.py pins them)


def mk_rules(keep=((), (), (), ()), cap=4, drop=1):
    """keep[kind]: class indices exempt from the equal-drop; cap: one value or one per kind -> SdxDispatchRules."""
    from pysignalduino_amd import runtime
    r = runtime.SdxDispatchRules()
    for kd in range(4):
        for c in keep[kd]:
            r.keep_equal[kd][c >> 6] |= 1 << (c & 63)
        r.max_repeat[kd] = cap if isinstance(cap, int) else cap[kd]
    r.drop_equal, r.res = drop, 0
    return r


def decide(recs, heap, keep, cap, drop, n_class):
    """The definition over sdx_result rows -> the kept rows' positions."""
    out, run, prev, last = [], 0, None, None
    for j, r in enumerate(recs):
        proto = int(r["proto"])
        run = run + 1 if proto == prev else 1
        prev = proto
        if cap > 0 and run > cap:
            continue
        off, ln = int(r["payload_off"]), int(r["payload_len"])
        key = (proto, heap[off: off + ln].tobytes())
        eq = last is not None and key == last
        last = key
        if not (drop and eq and not (proto < n_class and proto in keep)):
            out.append(j)
    return out


class Chunk:
    """Planted launch outputs of the kinds given.  lines[i]: a list of slots (kind, records[, status]); a record is
    (proto, payload[, flags]) with flags "share" (the record's payload_off is the previous record's: one payload, two
    records) and / or an int (its bit_length).  Payloads stand in the heap back to back, without a separator: a
    compare that ran past a payload's end would read the next payload's bytes.  ``shuffle``: the lines' record ranges
    stand in a random order in the record array, as a launch's units reserve them.  The cursor's words 1 to 3 carry
    values the pass must copy."""

    CUR = (0, 4321, 2, 55)
    HEAP_GUARD = 64

    def __init__(self, eng, lines, kinds=None, shuffle=1):
        from pysignalduino_amd import runtime
        t = eng.torch
        self.eng, self.n, self.lines = eng, len(lines), lines
        n = self.n
        self.kinds = sorted({s[0] for ln in lines for s in ln} | {0}) if kinds is None else list(kinds)
        self.dev = lambda a: t.from_numpy(np.frombuffer(a.tobytes() if hasattr(a, "tobytes") else bytes(a),  # noqa: E731
                                                        np.uint8).copy()).to(eng.dev)
        self.meta = t.zeros(32 * max(n, 1), dtype=t.uint8, device=eng.dev)
        self.pat_val = t.full((10 * max(n, 1),), 377.5, dtype=t.float64, device=eng.dev)
        self.cp_slot = t.zeros(max(n, 1), dtype=t.int8, device=eng.dev)
        order = np.random.default_rng(shuffle).permutation(n) if shuffle else np.arange(n)
        self.outs, self.ins, self.desc, self.rec, self.heap = [], [], [], [], []
        for kd in self.kinds:
            desc = np.zeros(max(n, 1), runtime.DESC_DT)
            slot_of = {i: s for i, ln in enumerate(lines) for s in ln if s[0] == kd}
            recs, heap = [], bytearray()
            for i in order.tolist():
                s = slot_of.get(i)
                if s is None:
                    continue
                st = s[2] if len(s) > 2 else OK
                desc[i] = (len(recs), len(s[1]), st, 2 if st == RAISED else 0)
                for r in s[1]:
                    proto, payload, flags = r[0], r[1], r[2:]
                    bl = next((f for f in flags if isinstance(f, int)), 8 * len(payload))
                    if "share" in flags:
                        assert recs and recs[-1][1] == len(payload)
                        recs.append((recs[-1][0], len(payload), proto, bl, i))
                    else:
                        recs.append((len(heap), len(payload), proto, bl, i))
                        heap += payload
            rec = np.array(recs, runtime.RES_DT) if recs else np.zeros(1, runtime.RES_DT)
            cur = np.array(self.CUR, np.uint32)
            cur[0] = len(recs)
            hnp = np.frombuffer(bytes(heap) + b"\xA5" * self.HEAP_GUARD, np.uint8)     # nothing behind the last payload byte but the guard
            out = {"desc": self.dev(desc), "rec": self.dev(rec), "heap": self.dev(hnp), "rec_cap": len(rec), "heap_cap": len(heap),
                   "cursor": t.from_numpy(cur.view(np.int32).copy()).to(eng.dev), "n": n}
            self.outs.append(out)
            self.desc.append(desc[:n].copy())
            self.rec.append(rec)
            self.heap.append(hnp)
            self.ins.append(self.json_in(kd, out))

    def json_in(self, kd, out, first_only=True):
        return self.eng.json_in(kd, out, {"meta": self.meta, "pat_val": self.pat_val, "cp_slot": self.cp_slot}, self.n, first_only)

    def expect(self, rules, caps=None):
        """-> per kind (descriptors, [(begin, kept records)], cursor) by the definition; caps[i]: the declared capacity
        (default: nothing overflows)."""
        res = []
        for x, kd in enumerate(self.kinds):
            keep = {64 * w + b for w in range(4) for b in range(64) if (rules.keep_equal[kd][w] >> b) & 1}
            cap = None if caps is None else caps[x]
            d_in, r_in = self.desc[x], self.rec[x]
            desc = d_in.copy()
            stored, begin, ovf = [], 0, 0
            for i in np.nonzero(d_in["status"] == OK)[0].tolist():
                b0, nr = int(d_in[i]["rec_begin"]), int(d_in[i]["n_rec"])
                rows = r_in[b0: b0 + nr]
                kept = [rows[j] for j in decide(rows, self.heap[x], keep, int(rules.max_repeat[kd]), int(rules.drop_equal), COUNTS[kd])]
                if cap is not None and kept and begin + len(kept) > cap:
                    desc[i] = (begin, 0, OVF_OUT, 0)
                    ovf = 1
                else:
                    desc[i] = (begin, len(kept), OK, 0)
                    stored.append((begin, kept))
                begin += len(kept)
            cur = np.array(self.CUR, np.uint32)
            cur[0] = begin
            cur[2] |= ovf
            res.append((desc, stored, cur))
        return res

    def run(self, rules, caps=None, guard=4, call=None):
        """The pass over the chunk (``call``: another pass with dispatch_records' arguments).  Outputs are pre-filled
        with 9s; the record arrays own ``guard`` records of 0xA5 behind the declared capacity.  -> per kind
        (descriptors, the whole record buffer as bytes, cursor), the outs."""
        from pysignalduino_amd import runtime
        eng, n, t = self.eng, self.n, self.eng.torch
        caps = [o["rec_cap"] for o in self.outs] if caps is None else list(caps)
        bufs = eng.alloc_dispatch(n, self.outs)
        for o, c in zip(bufs["outs"], caps):
            o["rec"] = t.full(((c + guard) * 16,), 9, dtype=t.uint8, device=eng.dev)
            o["rec"][c * 16:] = 0xA5
            o["rec_cap"] = c
            o["desc"].fill_(9)
            o["cursor"].view(t.uint8).fill_(9)
        bufs["scratch"].fill_(0xEE)
        outs = (call or eng.dispatch_records)(rules, self.ins, n, bufs, rec_caps=caps)
        t.cuda.synchronize()
        got = [(o["desc"][: 8 * n].cpu().numpy().view(runtime.DESC_DT), o["rec"].cpu().numpy().tobytes(),
                o["cursor"].cpu().numpy().view(np.uint32)) for o in outs]
        return got, outs, caps, bufs

    def check(self, rules, caps=None, guard=4):
        got, outs, caps_, bufs = self.run(rules, caps, guard)
        exp = self.expect(rules, caps)
        for x, ((gd, gr, gc), (ed, stored, ec)) in enumerate(zip(got, exp)):
            assert gc.tolist() == ec.tolist(), (self.kinds[x], gc, ec)
            bad = np.nonzero(gd != ed)[0]
            assert not len(bad), (self.kinds[x], bad[:5], gd[bad[:5]], ed[bad[:5]])
            want = bytearray(b"\x09" * (16 * caps_[x]) + b"\xA5" * (16 * guard))
            for begin, kept in stored:
                for j, r in enumerate(kept):
                    want[16 * (begin + j): 16 * (begin + j + 1)] = r.tobytes()
            assert gr == bytes(want), (self.kinds[x], next(i for i in range(len(gr)) if gr[i] != want[i]) // 16)
            assert outs[x]["heap"] is self.outs[x]["heap"]                                 # the payloads stay in the launch's heap
            assert (self.outs[x]["heap"].cpu().numpy() == self.heap[x]).all()              # ... which nobody wrote
            assert (self.outs[x]["rec"].cpu().numpy().tobytes() == self.rec[x].tobytes())
        return got, exp, outs, bufs

    def kept_counts(self, exp, x=0):
        return exp[x][0]["n_rec"].tolist()


def runs_recs(rng, k, protos, vocab=(b"", b"7", b"70", b"71", b"A0F3"), p_same=0.6):
    """k records in runs: the proto stays with probability p_same, payloads out of a small vocabulary -- many equal
    neighbours, many runs longer than the cap."""
    out, p = [], None
    for _ in range(k):
        if p is None or rng.random() > p_same:
            p = int(protos[int(rng.integers(0, len(protos)))])
        out.append((p, vocab[int(rng.integers(0, len(vocab)))]))
    return out


def mixed_lines(n, seed, kinds=(0, 1, 2, 3), max_rec=7, bad_every=11):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        if i % 7 == 5:
            out.append([])
            continue
        kd = kinds[(i // 3) % len(kinds)]
        st = (RAISED, OVF_OUT, ABSENT, OVF_TILE)[(i // bad_every) % 4] if bad_every and i % bad_every == 4 else OK
        out.append([(kd, runs_recs(rng, int(rng.integers(0, max_rec + 1)), np.arange(0, COUNTS[kd], 5)), st)])
    return out


KEEP = ((0, 5, 60, 125), (0, 65), (5,), (15,))        # some of mixed_lines' protos per kind


@pytest.fixture(scope="module")
def default_rules():
    return mk_rules(KEEP, cap=4, drop=1)


# ---- line counts ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_line_counts(eng, default_rules, n):
    c = Chunk(eng, mixed_lines(n, seed=n), kinds=(0, 1, 2, 3))
    got, exp, _, _ = c.check(default_rules)
    if n >= 255:
        tot_in = sum(int(d["n_rec"][d["status"] == OK].sum()) for d in c.desc)
        tot_out = sum(int(e[2][0]) for e in exp)
        assert 0 < tot_out < tot_in
        assert all(any(d["status"] == s for e in exp for d in e[0]) for s in (RAISED, OVF_OUT, ABSENT, OVF_TILE))


def test_65537_lines_need_a_second_trip_of_the_block_scan(eng, default_rules):
    n = 65537                                            # 257 blocks of 256 lines: more block totals than one trip scans
    rng = np.random.default_rng(5)
    k = rng.integers(0, 4, n)
    pay = (b"", b"1")
    lines = [[(0, [(7, pay[(i + j) % 3 == 0]) for j in range(k[i])])] for i in range(n)]
    lines[n - 1] = [(0, [(0, b"x"), (0, b"x"), (1, b"x"), (2, b"y"), (2, b"y")])]     # the last block's only line
    c = Chunk(eng, lines, kinds=(0,))
    got, exp, _, _ = c.check(default_rules)
    assert exp[0][0][n - 1]["n_rec"] == 4 and int(exp[0][0][n - 1]["rec_begin"]) == int(exp[0][2][0]) - 4 > 30000
    assert int(exp[0][2][0]) < int(k.sum())


# ---- list lengths -----------------------------------------------------------------------------------------
def test_list_lengths_and_long_lines_at_block_edges(eng):
    rng = np.random.default_rng(7)
    protos = np.arange(0, 129, 8)
    lens = [200, 0, 1, 2, 5, 64, 65] + [1] * 248 + [200, 3] + [2] * 254 + [200]     # 200 first, at line 255, last
    assert len(lens) == 512 and lens[255] == 200 and lens[0] == lens[-1] == 200
    lines = [[(0, runs_recs(rng, k, protos, p_same=0.8))] for k in lens]
    for rules in (mk_rules(KEEP), mk_rules(KEEP, cap=0), mk_rules(KEEP, cap=1, drop=0), mk_rules(cap=0, drop=0)):
        c = Chunk(eng, lines, kinds=(0,))
        got, exp, _, _ = c.check(rules)
        nr = c.kept_counts(exp)
        if rules.max_repeat[0] == 0 and not rules.drop_equal:
            assert nr == lens                                                        # no rule: the input in line order
        else:
            assert 0 < nr[0] < 200 and 0 < nr[255] < 200 and 0 < nr[511] < 200 and nr[2] == 1
    # long lines on both sides of the block boundary
    lens = [1] * 255 + [200, 200] + [1] * 10
    Chunk(eng, [[(0, runs_recs(rng, k, protos, p_same=0.8))] for k in lens], kinds=(0,)).check(mk_rules(KEEP))


# ---- the cap ---------------------------------------------------------------------------------------------------
def test_runs_around_the_cap(eng):
    def line(*runs):     # (proto, length) runs of distinct payloads: the cap alone decides
        return [(0, [(p, b"%d" % j) for p, k in runs for j in range(k)])]
    lines = [line((3, 3)), line((3, 4)), line((3, 5)), line((3, 9)), line((3, 5), (4, 5), (3, 5)), line((3, 1), (4, 1), (3, 1)),
             line((3, 4), (4, 4)), line((128, 6), (129, 6), (65535, 6))]
    c = Chunk(eng, lines)
    _, exp, _, _ = c.check(mk_rules(cap=4, drop=0))
    assert c.kept_counts(exp) == [3, 4, 4, 4, 12, 3, 8, 12]
    _, exp, _, _ = c.check(mk_rules(cap=1, drop=0))
    assert c.kept_counts(exp) == [1, 1, 1, 1, 3, 3, 2, 3]
    _, exp, _, _ = c.check(mk_rules(cap=0, drop=0))
    assert c.kept_counts(exp) == [3, 4, 5, 9, 15, 3, 8, 18]
    _, exp, _, _ = c.check(mk_rules(cap=(2, 4, 4, 4), drop=1))
    assert c.kept_counts(exp) == [2, 2, 2, 2, 6, 3, 4, 6]
    # A A A A A: the cap counts the equal ones too, so one A is left -- and a capped record does not become ``last``
    eq = [[(0, [(3, b"A")] * 5)], [(0, [(3, b"A")] * 4 + [(3, b"B"), (4, b"B"), (3, b"A")])], [(0, [(3, b"A")] * 5 + [(3, b"B")])]]
    c = Chunk(eng, eq)
    _, exp, _, _ = c.check(mk_rules(cap=4))
    assert c.kept_counts(exp) == [1, 3, 1]
    _, exp, _, _ = c.check(mk_rules(cap=0))
    assert c.kept_counts(exp) == [1, 4, 2]
    _, exp, _, _ = c.check(mk_rules(cap=4, drop=0))
    assert c.kept_counts(exp) == [4, 6, 4]


# ---- the equal-message rule ------------------------------------------------------------------------------------
def test_payload_comparisons(eng):
    long_a = bytes(range(48, 48 + 75)) * 3
    lines = [
        [(0, [(3, b"Xabcdefg"), (3, b"Yabcdefg")])],                       # only the first byte differs
        [(0, [(3, b"abcdefgX"), (3, b"abcdefgY")])],                       # only the last byte differs
        [(0, [(3, b"abcdefgX"), (3, b"abcdefgX")])],                       # equal
        [(0, [(3, long_a + b"1"), (3, long_a + b"2"), (3, long_a + b"2")])],
        [(0, [(3, b""), (3, b""), (3, b"a"), (3, b"a")])],                 # lengths 0 and 1
        [(0, [(3, b"abc"), (3, b"abc", "share"), (3, b"abc")])],           # two records of one payload_off, then a copy
        [(0, [(3, b"abc"), (4, b"abc", "share"), (4, b"abc"), (3, b"abc")])],   # an equal payload under another proto
        [(0, [(3, b"abc", 24), (3, b"abc", 23), (3, b"abc", 0)])],         # bit_length is not part of the key
        [(0, [(3, b"abc"), (3, b"abcd"), (3, b"abc"), (3, b"ab")])],       # a prefix is not equal: the length first
        [(1, [(9, b"AB"), (9, b"AB"), (9, b"AB")])],
        [(0, [(3, b"b"), (3, b""), (3, b""), (3, b"a")])],
        [(0, [(3, b"ab"), (3, b"ab")])],                                   # the chunk's last payload: nothing behind it but the guard
    ]
    c = Chunk(eng, lines, shuffle=0)
    assert c.heap[0][: -Chunk.HEAP_GUARD].tobytes().endswith(b"abab")
    _, exp, _, _ = c.check(mk_rules())
    assert c.kept_counts(exp, 0)[:9] + c.kept_counts(exp, 0)[10:] == [2, 2, 1, 2, 2, 1, 3, 1, 4, 3, 1] and c.kept_counts(exp, 1)[9] == 1
    assert [int(r["bit_length"]) for r in exp[0][1][7][1]] == [24]
    _, exp, _, _ = c.check(mk_rules(drop=0))
    assert c.kept_counts(exp, 0)[:9] == [2, 2, 2, 3, 4, 3, 4, 3, 4]
    for shuffle in (1, 2):
        Chunk(eng, lines, shuffle=shuffle).check(mk_rules())


def test_keep_equal_word_edges_and_protos_beyond_the_class_count(eng):
    every = [0, 62, 63, 64, 65, 127, 128, 129, 130, 191, 192, 255, 256, 256 + 63, 320, 65535]
    lines = [[(0, [(p, b"same")] * 3)] for p in every]
    lines += [[(1, [(p, b"")] * 2)] for p in (0, 63, 64, 65, 66, 127, 255, 256 + 65)]       # 66 = MS's class count
    lines += [[(2, [(p, b"k")] * 2)] for p in (0, 11, 12, 63, 64 + 11, 255)]
    lines += [[(3, [(p, b"k")] * 2)] for p in (0, 18, 19, 63, 255, 256 + 18)]
    c = Chunk(eng, lines)
    on = mk_rules(((63, 64, 128), (0, 63, 64, 65), (11,), (18,)))
    _, exp, _, _ = c.check(on)
    want = {0: {63, 64, 128}, 1: {0, 63, 64, 65}, 2: {11}, 3: {18}}
    for x, kd in enumerate(c.kinds):
        for i, ln in enumerate(lines):
            if ln[0][0] == kd:
                p, k = ln[0][1][0][0], len(ln[0][1])
                # a proto at or above the class count (129 = MU's, 255, 256 + a set bit, 65535) is in no mask
                assert exp[x][0][i]["n_rec"] == (k if p in want[kd] else 1), (kd, p)
    off = mk_rules((sorted(set(range(129)) - {63, 64, 128}), range(1, 63), range(11), range(18)))
    _, exp, _, _ = c.check(off)
    assert [int(exp[0][0][i]["n_rec"]) for i in range(len(every))] == [3, 3, 1, 1, 3, 3, 1] + [1] * 9
    _, exp, _, _ = c.check(mk_rules([range(n) for n in COUNTS]))                            # every legal bit
    assert [int(exp[0][0][i]["n_rec"]) for i in range(len(every))] == [3] * 7 + [1] * 9
    _, exp, _, _ = c.check(mk_rules([range(n) for n in COUNTS], drop=0))
    assert [int(exp[0][0][i]["n_rec"]) for i in range(len(every))] == [3] * 16


# ---- status, kinds --------------------------------------------------------------------------------------------------
def test_other_statuses_are_copied_byte_for_byte(eng, default_rules):
    good = [(1, b"a"), (1, b"a"), (2, b"b")]
    lines = [[(0, good)], [(0, good, RAISED)], [], [(1, good, OVF_OUT)], [(2, good, ABSENT)], [(3, [])], [(3, good)],
             [(1, [], OK)], [(0, good, OVF_TILE)], [(0, [], RAISED)]]
    c = Chunk(eng, lines, shuffle=0)
    got, exp, _, _ = c.check(default_rules)
    k = c.kinds.index
    assert tuple(got[k(0)][0][1]) == tuple(c.desc[k(0)][1]) and got[k(0)][0][1]["raise_kind"] == 2 and got[k(0)][0][1]["n_rec"] == 3
    assert tuple(got[k(1)][0][3]) == tuple(c.desc[k(1)][3]) and got[k(1)][0][3]["status"] == OVF_OUT
    assert tuple(got[k(2)][0][4]) == tuple(c.desc[k(2)][4]) and got[k(2)][0][4]["status"] == ABSENT
    assert tuple(got[k(0)][0][8]) == tuple(c.desc[k(0)][8]) and got[k(0)][0][8]["status"] == OVF_TILE
    assert [int(g[2][0]) for g in got] == [2, 0, 0, 2]


def test_one_to_four_kinds_in_any_order(eng, default_rules):
    lines = mixed_lines(300, seed=12)
    for kinds in ((3, 1, 0, 2), (2,), (1, 3), (0, 3, 2)):
        c = Chunk(eng, [[s for s in ln if s[0] in kinds] for ln in lines], kinds=kinds)
        got, exp, _, _ = c.check(default_rules)
        assert all(int(e[2][0]) > 0 for e in exp)
    # one cap per kind
    c = Chunk(eng, lines, kinds=(0, 1, 2, 3))
    _, a, _, _ = c.check(mk_rules(KEEP, cap=(1, 0, 2, 4)))
    _, b, _, _ = c.check(mk_rules(KEEP, cap=(0, 1, 4, 2)))
    assert int(a[0][2][0]) < int(b[0][2][0]) and int(a[1][2][0]) > int(b[1][2][0])     # cap 1 < no cap, per kind


def test_the_pass_is_idempotent(eng, default_rules):
    c = Chunk(eng, mixed_lines(400, seed=3), kinds=(0, 1, 2, 3))
    got, exp, outs, bufs = c.check(default_rules)
    ins2 = [c.json_in(kd, o) for kd, o in zip(c.kinds, outs)]
    bufs2 = eng.alloc_dispatch(c.n, outs)
    outs2 = eng.dispatch_records(default_rules, ins2, c.n, bufs2)
    eng.torch.cuda.synchronize()
    for x, (o1, o2) in enumerate(zip(outs, outs2)):
        total = int(exp[x][2][0])
        assert o2["cursor"].cpu().numpy().view(np.uint32).tolist() == exp[x][2].tolist()
        assert o2["desc"][: 8 * c.n].cpu().numpy().tobytes() == o1["desc"][: 8 * c.n].cpu().numpy().tobytes()
        assert o2["rec"][: 16 * total].cpu().numpy().tobytes() == o1["rec"][: 16 * total].cpu().numpy().tobytes()


# ---- capacity ---------------------------------------------------------------------------------------------------
def test_capacity_contract(eng, default_rules):
    c = Chunk(eng, mixed_lines(600, seed=21, max_rec=8), kinds=(0, 1, 2, 3))
    demand = [int(e[2][0]) for e in c.expect(default_rules)]
    assert min(demand) > 40
    for caps in (demand, [d - 1 for d in demand], [d // 2 for d in demand], [0] * 4, [demand[0], 0, demand[2] - 1, demand[3] // 2]):
        got, exp, _, _ = c.check(default_rules, caps=caps)
        for x in range(4):
            d, cur = got[x][0], got[x][2]
            assert cur[0] == demand[x] and (cur[2] & 1) == (caps[x] < demand[x])     # word 0 still carries the demand
            n_ovf = int(((d["status"] == OVF_OUT) & (c.desc[x]["status"] == OK)).sum())
            assert (n_ovf > 0) == (caps[x] < demand[x])
            if caps[x] == demand[x] - 1:
                assert n_ovf == 1                                                    # the last line that keeps something
            fit = d[(d["status"] == OK) & (d["n_rec"] > 0)]
            assert all(int(f["rec_begin"]) + int(f["n_rec"]) <= caps[x] for f in fit)


# ---- one skeleton, two policies -------------------------------------------------------------------------------------
@pytest.mark.parametrize("short", [0, 1])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_no_rule_equals_the_profile_pass_with_every_class_enabled(eng, n, short):
    """sdx_dispatch_records with no rule on and sdx_filter_records with every class enabled both keep every record
    of every OK line, through the same count -> scan -> write (csrc/sdx_compact.h): descriptors, whole record
    buffers (so the records up to cursor[0], and the 9s and guards behind them) and the four cursor words are the
    same bytes.  ``short``: every kind's capacity is one record short of its demand, so both passes meet a list
    that does not fit."""
    from pysignalduino_amd import runtime
    from test_profiles import ALL, pack_table
    lines = mixed_lines(n, seed=40 + n) if n > 1 else [[(0, [(5, b"70"), (5, b"70"), (10, b"A0F3")])]]
    c = Chunk(eng, lines, kinds=(0, 1, 2, 3))
    demand = [int(d["n_rec"][d["status"] == OK].sum()) for d in c.desc]
    assert demand[0] > 0
    caps = [max(d - 1, 0) for d in demand] if short else None
    got, _, _, _ = c.check(mk_rules(cap=0, drop=0), caps=caps)
    table = runtime.DeviceProfileTable(eng, None, blob=pack_table([ALL], [0]))
    same, _, _, _ = c.run(None, caps, call=lambda _, ins, n_, bufs, rec_caps: eng.filter_records(table, ins, n_, bufs,
                                                                                                rec_caps=rec_caps))
    for x, ((dd, dr, dc), (fd, fr, fc)) in enumerate(zip(got, same)):
        assert dc.tolist() == fc.tolist() and dc[0] == demand[x], (x, dc, fc)
        assert dd.tobytes() == fd.tobytes() and dr == fr, x
        assert bool((dd["status"][c.desc[x]["status"] == OK] == OVF_OUT).any()) == bool(short and demand[x])


# ---- SDX_EINVAL ---------------------------------------------------------------------------------------------------
def test_einval_cases_launch_nothing(eng, default_rules):
    from pysignalduino_amd import runtime
    t = eng.torch
    lib = eng.lib
    c = Chunk(eng, mixed_lines(64, seed=2), kinds=(0, 1))
    bufs = eng.alloc_dispatch(64, c.outs)
    outs = bufs["outs"]
    for o in outs:
        o["desc"].fill_(9), o["cursor"].view(t.uint8).fill_(9), o["rec"].fill_(9)

    def call(bank=eng.handle, rules=default_rules, ins=c.ins, k=2, n=64, desc="d", rec="r", cap="c", cur="u",
             scratch=bufs["scratch"].data_ptr()):
        arr = (runtime.SdxJsonIn * max(len(ins), 1))(*ins) if ins is not None else None
        mk = lambda key: (ctypes.c_void_p * 2)(*[o[key].data_ptr() for o in outs])     # noqa: E731
        darr = mk("desc") if desc == "d" else desc
        rarr = mk("rec") if rec == "r" else rec
        uarr = mk("cursor") if cur == "u" else cur
        carr = (ctypes.c_uint32 * 2)(*[o["rec_cap"] for o in outs]) if cap == "c" else cap
        return lib.sdx_dispatch_records(bank, None if rules is None else ctypes.byref(rules), arr, k, n, darr, rarr, carr, uarr,
                                        scratch, eng.stream_ptr())

    def rules_with(**kw):
        r = mk_rules(KEEP)
        for key, v in kw.items():
            if key == "bit":
                r.keep_equal[v[0]][v[1] >> 6] |= 1 << (v[1] & 63)
            elif key == "cap":
                r.max_repeat[v[0]] = v[1]
            else:
                setattr(r, key, v)
        return r

    def without(field):
        x = runtime.SdxJsonIn()
        ctypes.memmove(ctypes.byref(x), ctypes.byref(c.ins[1]), ctypes.sizeof(runtime.SdxJsonIn))
        setattr(x, field, None)
        return x

    ptrs = lambda *v: (ctypes.c_void_p * 2)(*v)       # noqa: E731
    d0, d1 = (o["desc"].data_ptr() for o in outs)
    r0, r1 = (o["rec"].data_ptr() for o in outs)
    u0, u1 = (o["cursor"].data_ptr() for o in outs)
    cases = {
        "null bank": dict(bank=None), "null rules": dict(rules=None), "null kinds": dict(ins=None),
        "k = 0": dict(k=0), "k = 5": dict(k=5), "n < 0": dict(n=-1),
        "a kind twice": dict(ins=[c.ins[0], c.ins[0]]), "a bad kind": dict(ins=[c.ins[0], eng.json_in(4, c.outs[1], {"meta": c.meta}, 64)]),
        "another n": dict(ins=[c.ins[0], eng.json_in(1, c.outs[1], {"meta": c.meta}, 63)]),
        "a null rec_dev": dict(ins=[c.ins[0], without("rec_dev")]), "a null cursor_dev": dict(ins=[c.ins[0], without("cursor_dev")]),
        "a null desc_dev": dict(ins=[c.ins[0], without("desc_dev")]), "a null heap_dev": dict(ins=[c.ins[0], without("heap_dev")]),
        "null desc_out": dict(desc=None), "null rec_out": dict(rec=None), "null rec_cap": dict(cap=None), "null cursor_out": dict(cur=None),
        "a null desc entry": dict(desc=ptrs(d0, None)), "a null rec entry": dict(rec=ptrs(None, r1)),
        "a null cursor entry": dict(cur=ptrs(u0, None)), "null scratch": dict(scratch=None),
        "misaligned scratch": dict(scratch=bufs["scratch"].data_ptr() + 8),
        "misaligned desc": dict(desc=ptrs(d0 + 2, d1)), "misaligned rec": dict(rec=ptrs(r0, r1 + 8)),
        "misaligned cursor": dict(cur=ptrs(u0, u1 + 1)),
        # the validator: a bit at the class count of every kind (also of a kind the call does not name), the masks' last
        # bit (proto 255), a negative cap, the reserved word
        "MU bit 129": dict(rules=rules_with(bit=(0, 129))), "MS bit 66": dict(rules=rules_with(bit=(1, 66))),
        "MC bit 12": dict(rules=rules_with(bit=(2, 12))), "MN bit 19": dict(rules=rules_with(bit=(3, 19))),
        "MU bit 255": dict(rules=rules_with(bit=(0, 255))), "a negative cap": dict(rules=rules_with(cap=(1, -1))),
        "a negative cap of MN": dict(rules=rules_with(cap=(3, -2 ** 31))), "res": dict(rules=rules_with(res=1)),
    }
    for name, kw in cases.items():
        assert call(**kw) == EINVAL, name
        assert b"sdx_dispatch_records" in lib.sdx_last_error(), name
    t.cuda.synchronize()
    for o in outs:                                                   # nothing was launched
        assert set(o["desc"].cpu().numpy().tolist()) == {9} and set(o["cursor"].view(t.uint8).cpu().numpy().tolist()) == {9}
        assert set(o["rec"].cpu().numpy().tolist()) == {9}
    assert call(rules=rules_with(bit=(0, 128), drop_equal=-5)) == 0      # the last legal bit; any non-zero drop_equal is "on"
    t.cuda.synchronize()
    assert outs[0]["cursor"].cpu().numpy().view(np.uint32)[1] == Chunk.CUR[1]
    # the Python layer's own checks
    with pytest.raises(ValueError):
        eng.dispatch_records(default_rules, c.ins[:1], 64, bufs)
    with pytest.raises(ValueError):
        eng.dispatch_records(None, c.ins, 64, bufs)
    with pytest.raises(ValueError):
        eng.dispatch_records(default_rules, c.ins, 64, bufs, rec_caps=[10 ** 6, 1])


# ---- downstream consumers --------------------------------------------------------------------------------------
def planted_reduced(c, rules):
    """The chunk planted already reduced by the restatement: the same heaps and payload offsets, the kept records dense
    in line order, the cursors' record counts."""
    from pysignalduino_amd import runtime
    t, eng = c.eng.torch, c.eng
    outs = []
    for x, (desc, stored, cur) in enumerate(c.expect(rules)):
        rec = np.zeros(max(int(cur[0]), 1), runtime.RES_DT)
        for begin, kept in stored:
            for j, r in enumerate(kept):
                rec[begin + j] = r
        o = dict(c.outs[x])
        o.update(desc=c.dev(desc), rec=c.dev(rec), cursor=t.from_numpy(cur.view(np.int32).copy()).to(eng.dev), rec_cap=len(rec))
        outs.append(o)
    return outs


def texts(jo, items):
    off = jo["off"][:items].cpu().numpy().astype(np.int64)
    ln = jo["len"][:items].cpu().numpy().astype(np.int64)
    buf = jo["json"].cpu().numpy().tobytes()
    assert int(jo["cursor"][1].item()) == 0
    return [buf[o: o + k] if k else None for o, k in zip(off.tolist(), ln.tolist())]


def test_downstream_consumers_on_the_reduced_outputs(eng, default_rules):
    t = eng.torch
    n = 420
    rng = np.random.default_rng(33)
    pre = [b"P7#", b"P61#", b"W33#", b"u40#", b"s", b"i"]
    lines = []
    for i in range(n):
        if i % 9 == 7:
            lines.append([])
            continue
        kd = (i // 5) % 4
        vocab = [pre[int(rng.integers(0, len(pre)))] + b"%02X" % int(rng.integers(0, 2)) for _ in range(3)]
        base = runs_recs(rng, int(rng.integers(1, 9)), np.arange(0, COUNTS[kd], 3), vocab=vocab)
        if i % 4 == 1 and lines and lines[-1] and lines[-1][0][0] == kd:
            base = list(lines[-1][0][1])                  # a repeat of the previous line's list
        lines.append([(kd, base, RAISED if i % 31 == 30 else OK)])
    c = Chunk(eng, lines, kinds=(0, 1, 2, 3))
    got, exp, d_outs, bufs = c.check(default_rules)
    p_outs = planted_reduced(c, default_rules)
    assert sum(int((e[0]["n_rec"] != d["n_rec"]).sum()) for e, d in zip(exp, c.desc)) > 100

    def consumers(outs, items):
        r = {"json0": []}
        lo = {"meta": c.meta, "pat_val": c.pat_val, "cp_slot": c.cp_slot}
        for x, kd in enumerate(c.kinds):                  # sdx_serialize_json, one text per record
            jo = eng.alloc_json(max(outs[x]["rec_cap"], 1), 1 << 20)
            jo["len"].zero_()
            eng.launch_json(kd, outs[x], lo, n, jo, first_only=0)
            t.cuda.synchronize()
            r["json0"].append(texts(jo, items[x]))
        jo = eng.alloc_json(n, 1 << 20)                   # ... and one per line, sparse: the kinds share the outputs
        jo["len"].zero_()
        for x, kd in enumerate(c.kinds):
            eng.launch_json(kd, outs[x], lo, n, jo, first_only=2)
        t.cuda.synchronize()
        r["json2"] = texts(jo, n)
        rep, scratch = eng.alloc_repeat(n)
        state = eng.alloc_repeat_state()
        eng.mark_repeats([c.json_in(kd, o) for kd, o in zip(c.kinds, outs)], n, rep, scratch, state)
        t.cuda.synchronize()
        r["repeat"] = (rep[:n].cpu().numpy().tobytes(), state.cpu().numpy().tobytes())
        return r

    kept_n = [int(e[2][0]) for e in exp]
    a, b = consumers(d_outs, kept_n), consumers(p_outs, kept_n)
    assert a["json0"] == b["json0"] and a["json2"] == b["json2"] and a["repeat"] == b["repeat"]
    assert all(x is not None for k in a["json0"] for x in k) and sum(len(k) for k in a["json0"]) == sum(kept_n)
    # r_0 is always kept: the launch's own outputs give the same first_only = 2 texts and the same repeat mask and state
    raw = consumers(c.outs, [int(cu[0]) for cu in (o["cursor"].cpu().numpy().view(np.uint32) for o in c.outs)])
    assert raw["json2"] == a["json2"] and raw["repeat"] == a["repeat"]
    assert sum(x is not None for x in a["json2"]) > 150 and 0 < sum(a["repeat"][0]) < n
    assert sum(len(k) for k in raw["json0"]) > sum(kept_n)
