"""sdx_filter_records through the C ABI on planted launch outputs.

Expected values come from ``Chunk.expect``, the definition restated in Python over the records the test itself
planted and over masks the test itself packed: every line keeps the records whose class its source's profile
enables, in list order, compacted in line order; every other status keeps its descriptor's bytes."""
import ctypes
import struct

import numpy as np
import pytest

from test_routes import eng  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

OK, RAISED, OVF_OUT, ABSENT = 0, 1, 3, 0xFF
EINVAL = -1
COUNTS = (129, 66, 12, 19)      # this bank's class counts (test_profiles_host.py pins them)
MAGIC = 0x46505853


def pack_table(masks, of_source, counts=COUNTS):
    """masks[p][kind]: an iterable of enabled class indices -> the blob (csrc/sdx_profile_layout.h)."""
    m = np.zeros((len(masks), 4, 4), "<u8")
    for p, per_kind in enumerate(masks):
        for kd, cls in enumerate(per_kind):
            for c in cls:
                m[p, kd, c >> 6] |= np.uint64(1) << np.uint64(c & 63)
    body = m.tobytes() + bytes(of_source)
    total = (48 + len(body) + 15) & ~15
    return (struct.pack("<12I", MAGIC, 1, total, len(masks), len(of_source), *counts, 0, 0, 0) + body).ljust(total, b"\0")


class Table:
    """A profile table by its masks: the device handle and the restated lookup."""

    def __init__(self, eng, masks, of_source, counts=COUNTS):
        from pysignalduino_amd import runtime
        self.masks = [[frozenset(k) for k in p] for p in masks]
        self.of_source = list(of_source)
        self.dev = runtime.DeviceProfileTable(eng, None, blob=pack_table(masks, of_source, counts))

    def enabled(self, source, kind, proto):
        if not 0 <= source < len(self.of_source):
            return False
        return proto < COUNTS[kind] and proto in self.masks[self.of_source[source]][kind]


ALL = [range(c) for c in COUNTS]
NONE = [(), (), (), ()]


class Chunk:
    """Planted launch outputs of the kinds given.  lines[i]: a list of slots (kind, records[, status]); a record is
    (proto, payload).  ``shuffle``: the lines' record ranges stand in a random order in the launch's record array, as
    a launch's units reserve them.  The cursor's words 1 to 3 carry values the pass must copy."""

    CUR = (0, 1234, 2, 77)

    def __init__(self, eng, lines, kinds=None, shuffle=1, sources=None):
        from pysignalduino_amd import runtime
        t = eng.torch
        self.eng, self.n, self.lines = eng, len(lines), lines
        n = self.n
        self.kinds = sorted({s[0] for ln in lines for s in ln} | {0}) if kinds is None else list(kinds)
        self.sources = None if sources is None else np.asarray(sources, np.int32)
        self.d_src = None if sources is None else t.from_numpy(self.sources.copy()).to(eng.dev)
        self.dev = lambda a: t.from_numpy(np.frombuffer(a.tobytes() if hasattr(a, "tobytes") else bytes(a),  # noqa: E731
                                                        np.uint8).copy()).to(eng.dev)
        self.meta = t.zeros(32 * max(n, 1), dtype=t.uint8, device=eng.dev)
        self.pat_val = t.full((10 * max(n, 1),), 377.5, dtype=t.float64, device=eng.dev)
        self.cp_slot = t.zeros(max(n, 1), dtype=t.int8, device=eng.dev)
        order = np.random.default_rng(shuffle).permutation(n) if shuffle else np.arange(n)
        self.outs, self.ins, self.desc, self.rec, self.slots = [], [], [], [], []
        for kd in self.kinds:
            desc = np.zeros(max(n, 1), runtime.DESC_DT)
            slot_of = {}
            for i, ln in enumerate(lines):
                for s in ln:
                    if s[0] == kd:
                        slot_of[i] = s
            recs, heap = [], bytearray(b"\xA5")
            for i in order.tolist():
                s = slot_of.get(i)
                if s is None:
                    continue
                st = s[2] if len(s) > 2 else OK
                desc[i] = (len(recs), len(s[1]), st, 2 if st == RAISED else 0)
                for proto, payload in s[1]:
                    recs.append((len(heap), len(payload), proto, 8 * len(payload), i))
                    heap += payload + b"A0F"
            rec = np.array(recs, runtime.RES_DT) if recs else np.zeros(1, runtime.RES_DT)
            cur = np.array(self.CUR, np.uint32)
            cur[0] = len(recs)
            out = {"desc": self.dev(desc), "rec": self.dev(rec), "heap": self.dev(heap), "rec_cap": len(rec), "heap_cap": len(heap),
                   "cursor": t.from_numpy(cur.view(np.int32).copy()).to(eng.dev), "n": n}
            self.outs.append(out)
            self.desc.append(desc[:n].copy())
            self.rec.append(rec)
            self.slots.append(slot_of)
            self.ins.append(self.json_in(kd, out))

    def json_in(self, kd, out, first_only=True):
        return self.eng.json_in(kd, out, {"meta": self.meta, "pat_val": self.pat_val, "cp_slot": self.cp_slot}, self.n, first_only)

    def expect(self, table, caps=None):
        """-> per kind (descriptors, the kept records in line order, cursor) by the definition; caps[i]: the declared
        capacity (default: nothing overflows)."""
        from pysignalduino_amd import runtime
        res = []
        for x, kd in enumerate(self.kinds):
            cap = None if caps is None else caps[x]
            d_in, r_in = self.desc[x], self.rec[x]
            desc = d_in.copy()
            kept_all, stored, begin, ovf = [], [], 0, 0
            for i in range(self.n):
                if d_in[i]["status"] != OK:
                    continue
                src = 0 if self.sources is None else int(self.sources[i])
                b0 = int(d_in[i]["rec_begin"])
                kept = [r_in[j] for j in range(b0, b0 + int(d_in[i]["n_rec"])) if table.enabled(src, kd, int(r_in[j]["proto"]))]
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

    def run(self, table, caps=None, guard=4):
        """The pass over the chunk.  Outputs are pre-filled with 9s; the record arrays own ``guard`` records of 0xA5
        behind the declared capacity.  -> per kind (descriptors, the whole record buffer as bytes, cursor), the outs."""
        from pysignalduino_amd import runtime
        eng, n, t = self.eng, self.n, self.eng.torch
        caps = [o["rec_cap"] for o in self.outs] if caps is None else list(caps)
        bufs = eng.alloc_profiles(n, self.outs)
        for o, c in zip(bufs["outs"], caps):
            o["rec"] = t.full(((c + guard) * 16,), 9, dtype=t.uint8, device=eng.dev)
            o["rec"][c * 16:] = 0xA5
            o["rec_cap"] = c
            o["desc"].fill_(9)
            o["cursor"].view(t.uint8).fill_(9)
        bufs["scratch"].fill_(0xEE)
        outs = eng.filter_records(table.dev, self.ins, n, bufs, source=self.d_src)
        t.cuda.synchronize()
        got = [(o["desc"][: 8 * n].cpu().numpy().view(runtime.DESC_DT), o["rec"].cpu().numpy().tobytes(),
                o["cursor"].cpu().numpy().view(np.uint32)) for o in outs]
        return got, outs, caps, bufs

    def check(self, table, caps=None, guard=4):
        """The pass == the definition, byte for byte: descriptors, every record buffer (the kept records in their place,
        9s everywhere else below the capacity, 0xA5 behind it) and all four cursor words."""
        got, outs, caps_, bufs = self.run(table, caps, guard)
        exp = self.expect(table, caps)
        for x, ((gd, gr, gc), (ed, stored, ec)) in enumerate(zip(got, exp)):
            assert gc.tolist() == ec.tolist(), (self.kinds[x], gc, ec)
            bad = np.nonzero(gd != ed)[0]
            assert not len(bad), (self.kinds[x], bad[:5], gd[bad[:5]], ed[bad[:5]])
            want = bytearray(b"\x09" * (16 * caps_[x]) + b"\xA5" * (16 * guard))
            for begin, kept in stored:
                for j, r in enumerate(kept):
                    want[16 * (begin + j): 16 * (begin + j + 1)] = r.tobytes()
            assert gr == bytes(want), (self.kinds[x], next(i for i in range(len(gr)) if gr[i] != want[i]) // 16)
        return got, exp, outs, bufs


def recs(rng, k, protos, plen=6):
    return [(int(protos[int(rng.integers(0, len(protos)))]), bytes(rng.integers(48, 58, int(rng.integers(0, plen + 1)), dtype=np.uint8)))
            for _ in range(k)]


def mixed_lines(n, seed, kinds=(0, 1, 2, 3), max_rec=5, bad_every=11):
    """n lines over the kinds with 0 to max_rec records of valid classes; some raised / overflowed / absent, some empty."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        if i % 7 == 5:
            out.append([])
            continue
        kd = kinds[(i // 3) % len(kinds)]
        st = (RAISED, OVF_OUT, ABSENT)[(i // bad_every) % 3] if bad_every and i % bad_every == 4 else OK
        out.append([(kd, recs(rng, int(rng.integers(0, max_rec + 1)), np.arange(COUNTS[kd])), st)])
    return out


def half_masks(seed):
    rng = np.random.default_rng(seed)
    return [sorted(rng.choice(c, c // 2, replace=False).tolist()) for c in COUNTS]


@pytest.fixture(scope="module")
def four(eng):
    """Four profiles over four sources: everything, a random half, another half, nothing."""
    return Table(eng, [ALL, half_masks(1), half_masks(2), NONE], [0, 1, 2, 3])


# ---- line counts ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_line_counts(eng, four, n):
    lines = mixed_lines(n, seed=n)
    rng = np.random.default_rng(n)
    c = Chunk(eng, lines, kinds=(0, 1, 2, 3), sources=rng.integers(0, 4, n))
    got, exp, _, _ = c.check(four)
    if n >= 255:
        tot_in = sum(len(r) for r in c.rec)
        tot_out = sum(int(e[2][0]) for e in exp)
        assert 0 < tot_out < tot_in
        assert all(any(d["status"] == s for e in exp for d in e[0]) for s in (RAISED, OVF_OUT, ABSENT))


def test_65537_lines_need_a_second_trip_of_the_block_scan(eng, four):
    n = 65537                                            # 257 blocks of 256 lines: more block totals than one trip scans
    rng = np.random.default_rng(5)
    k = rng.integers(0, 3, n)
    protos = rng.integers(0, COUNTS[0], (n, 2))
    lines = [[(0, [(int(protos[i, j]), b"") for j in range(k[i])])] for i in range(n)]
    lines[n - 1] = [(0, [(0, b"x"), (1, b"y")])]         # the last block's only line keeps something under profile 0
    src = rng.integers(0, 4, n)
    src[n - 1] = 0
    c = Chunk(eng, lines, kinds=(0,), sources=src)
    got, exp, _, _ = c.check(four)
    assert exp[0][0][n - 1]["n_rec"] == 2 and int(exp[0][0][n - 1]["rec_begin"]) == int(exp[0][2][0]) - 2 > 30000


# ---- list lengths -----------------------------------------------------------------------------------------
def test_list_lengths_and_long_lines_at_block_edges(eng, four):
    rng = np.random.default_rng(7)
    mu = np.arange(COUNTS[0])
    lens = [200, 0, 1, 2, 63, 64, 65] + [1] * 248 + [200, 3] + [2] * 254 + [200]     # 200 first, at lines 255 | 256, last
    assert len(lens) == 512 and lens[255] == 200 and lens[0] == lens[-1] == 200
    lines = [[(0, recs(rng, k, mu, plen=2))] for k in lens]
    for src in (None, np.arange(len(lens)) % 3 + (np.arange(len(lens)) == 511)):     # lines 0 and 255: source 0, 511: 2
        c = Chunk(eng, lines, kinds=(0,), sources=src)
        got, exp, _, _ = c.check(four)
        nr = exp[0][0]["n_rec"]
        assert (nr[0] == 200) == (src is None or src[0] == 0)
        if src is not None:
            assert nr[255] == 200 and 0 < nr[511] < 200 and 0 < nr[256 + 2] <= 2
    # a long line straddling the boundary: lines 255 and 256 both long, under a half-enabled profile
    lens = [1] * 255 + [200, 200] + [1] * 10
    c = Chunk(eng, [[(0, recs(rng, k, mu, plen=2))] for k in lens], kinds=(0,), sources=[1] * len(lens))
    c.check(four)


# ---- mask word edges, sources and profiles -------------------------------------------------------------------
def test_mask_word_edges_and_protos_beyond_the_class_count(eng):
    edges = [0, 63, 64, 127, 128]
    t_on = Table(eng, [[edges, [0, 63, 64, 65], [0, 11], [0, 18]]], [0])
    t_off = Table(eng, [[sorted(set(range(129)) - set(edges)), range(1, 63), range(1, 11), range(1, 18)]], [0])
    every = [0, 1, 62, 63, 64, 65, 126, 127, 128, 129, 130, 191, 192, 255, 256, 256 + 63, 320, 512 + 128, 65535]
    lines = [[(0, [(p, b"%d" % p) for p in every])],
             [(1, [(p, b"") for p in (0, 63, 64, 65, 66, 67, 127, 128, 255, 256, 65535)])],
             [(2, [(p, b"") for p in (0, 10, 11, 12, 13, 63, 64, 255, 256 + 11)])],
             [(3, [(p, b"") for p in (0, 17, 18, 19, 20, 63, 64, 255)])],
             [(0, [(129, b"a")])], [(0, [(255, b"a")])], [(0, [(128, b"a")])]]
    c = Chunk(eng, lines)
    got, exp, _, _ = c.check(t_on)
    assert [int(r["proto"]) for r in exp[0][1][0][1]] == edges                   # 129 (= the class count) .. 65535 dropped
    assert exp[0][0]["n_rec"].tolist()[4:] == [0, 0, 1] and [e[2][0] for e in exp] == [6, 4, 2, 2]
    got, exp, _, _ = c.check(t_off)
    assert [int(r["proto"]) for r in exp[0][1][0][1]] == [1, 62, 65, 126]
    allt = Table(eng, [ALL], [0])
    got, exp, _, _ = c.check(allt)
    assert [int(r["proto"]) for r in exp[0][1][0][1]] == [p for p in every if p < 129]


def test_profile_63_source_4095_and_ids_outside_the_table(eng):
    masks = [NONE] * 64
    masks[0] = [[1], [1], [1], [1]]
    masks[63] = [[2, 128], [2, 65], [2, 11], [2, 18]]
    of_source = [0] * 4096
    of_source[4095] = 63
    of_source[1] = 62                                    # keeps nothing
    tab = Table(eng, masks, of_source)
    small = Table(eng, [[[1, 2]] * 4, NONE], [0, 1, 0])  # three sources: ids 3 and beyond keep nothing
    rng = np.random.default_rng(3)
    lines, src = [], []
    for i in range(300):
        kd = i % 4
        lines.append([(kd, [(1, b"a"), (2, b"b"), (COUNTS[kd] - 1, b"c"), (3, b"d")])])
        src.append([0, 4095, 1, 4096, -1, 2, 3, 2 ** 31 - 1, -2 ** 31][i % 9])
    c = Chunk(eng, lines, sources=src)
    got, exp, _, _ = c.check(tab)
    for x, kd in enumerate(c.kinds):
        for i in range(kd, 300, 4):
            want = {0: 1, 2: 1, 3: 1, 4095: 2}.get(src[i], 0)          # sources 2 and 3 are on profile 0 too
            assert exp[x][0][i]["n_rec"] == want, (i, src[i])
    got, exp, _, _ = c.check(small)
    assert {int(exp[0][0][i]["n_rec"]) for i in range(0, 300, 4) if src[i] in (0, 2)} == {2}
    assert not any(exp[0][0][i]["n_rec"] for i in range(0, 300, 4) if src[i] not in (0, 2))
    # source_dev = NULL: every line is source 0
    c0 = Chunk(eng, lines, sources=None)
    got, exp, _, _ = c0.check(tab)
    assert [int(e[2][0]) for e in exp] == [75, 75, 75, 75]


# ---- all on, all off, status, kinds ----------------------------------------------------------------------------
def test_all_enabled_is_the_input_in_line_order_and_nothing_enabled_is_empty(eng):
    lines = mixed_lines(700, seed=9)
    c = Chunk(eng, lines, kinds=(0, 1, 2, 3))
    got, exp, _, _ = c.check(Table(eng, [ALL], [0]))
    for x in range(4):
        d_in, (d_out, rec_b, cur) = c.desc[x], got[x]
        ok = d_in["status"] == OK
        assert (d_out["n_rec"] == d_in["n_rec"]).all() and cur[0] == d_in["n_rec"][ok].sum() > 0
        assert (d_out[~ok] == d_in[~ok]).all() and (~ok).sum() > 3
        out = np.frombuffer(rec_b, c.rec[x].dtype)
        by_line = np.concatenate([c.rec[x][int(d["rec_begin"]): int(d["rec_begin"]) + int(d["n_rec"])] for d in d_in[ok]])
        assert (out[: cur[0]] == by_line).all()                        # the input re-ordered by line
        assert (np.diff(out[: cur[0]]["msg"].astype(np.int64)) >= 0).all()
        assert not (np.diff(c.rec[x]["msg"].astype(np.int64)) >= 0).all()   # which the planted launch was not
    got, exp, _, _ = c.check(Table(eng, [NONE], [0]))
    for x in range(4):
        d_in, (d_out, rec_b, cur) = c.desc[x], got[x]
        ok = d_in["status"] == OK
        assert cur[0] == 0 and not d_out["n_rec"][ok].any() and (d_out["status"][ok] == OK).all()
        assert (d_out[~ok] == d_in[~ok]).all()
        assert set(rec_b[: 16 * c.outs[x]["rec_cap"]]) == {9}         # nothing stored


def test_other_statuses_are_copied_byte_for_byte(eng, four):
    good = [(1, b"a"), (2, b"b")]
    lines = [[(0, good)], [(0, good, RAISED)], [], [(1, good, OVF_OUT)], [(2, good, ABSENT)], [(3, [])], [(3, good)],
             [(1, [], OK)], [(0, good, 2)], [(0, [], RAISED)]]
    c = Chunk(eng, lines, shuffle=0)
    got, exp, _, _ = c.check(four)
    k = c.kinds.index
    assert tuple(got[k(0)][0][1]) == tuple(c.desc[k(0)][1]) and got[k(0)][0][1]["raise_kind"] == 2 and got[k(0)][0][1]["n_rec"] == 2
    assert tuple(got[k(1)][0][3]) == tuple(c.desc[k(1)][3]) and got[k(1)][0][3]["status"] == OVF_OUT
    assert tuple(got[k(2)][0][4]) == tuple(c.desc[k(2)][4]) and got[k(2)][0][4]["status"] == ABSENT
    assert tuple(got[k(0)][0][8]) == tuple(c.desc[k(0)][8])                       # SDX_ST_OVF_TILE
    assert [int(g[2][0]) for g in got] == [2, 0, 0, 2]


def test_four_kinds_in_one_call_in_any_order(eng, four):
    lines = mixed_lines(300, seed=12)
    rng = np.random.default_rng(12)
    src = rng.integers(0, 4, 300)
    for kinds in ((3, 1, 0, 2), (2,), (1, 3)):
        c = Chunk(eng, [[s for s in ln if s[0] in kinds] for ln in lines], kinds=kinds, sources=src)
        got, exp, _, _ = c.check(four)
        assert all(int(e[2][0]) > 0 for e in exp) and [e[2][0] for e in exp] == [g[2][0] for g in got]


# ---- capacity ---------------------------------------------------------------------------------------------------
def test_capacity_contract(eng, four):
    lines = mixed_lines(600, seed=21, max_rec=6)
    rng = np.random.default_rng(21)
    c = Chunk(eng, lines, kinds=(0, 1, 2, 3), sources=rng.integers(0, 3, 600))
    demand = [int(e[2][0]) for e in c.expect(four)]
    assert min(demand) > 40
    for caps in (demand, [d - 1 for d in demand], [d // 2 for d in demand], [0] * 4, [demand[0], 0, demand[2] - 1, demand[3] // 2]):
        got, exp, _, _ = c.check(four, caps=caps)
        for x in range(4):
            d, cur = got[x][0], got[x][2]
            assert cur[0] == demand[x] and (cur[2] & 1) == (caps[x] < demand[x])     # word 0 still carries the demand
            n_ovf = int(((d["status"] == OVF_OUT) & (c.desc[x]["status"] == OK)).sum())
            assert (n_ovf > 0) == (caps[x] < demand[x])
            if caps[x] == demand[x] - 1:
                assert n_ovf == 1                                                    # the last line that keeps something
            fit = d[(d["status"] == OK) & (d["n_rec"] > 0)]
            assert all(int(f["rec_begin"]) + int(f["n_rec"]) <= caps[x] for f in fit)


# ---- SDX_EINVAL ---------------------------------------------------------------------------------------------------
def test_einval_cases_launch_nothing(eng, four):
    from pysignalduino_amd import runtime
    t = eng.torch
    lib = eng.lib
    c = Chunk(eng, mixed_lines(64, seed=2), kinds=(0, 1))
    bufs = eng.alloc_profiles(64, c.outs)
    outs = bufs["outs"]
    for o in outs:
        o["desc"].fill_(9), o["cursor"].view(t.uint8).fill_(9), o["rec"].fill_(9)
    src = t.zeros(80, dtype=t.int32, device=eng.dev)

    def call(bank=eng.handle, table=four.dev.handle, ins=c.ins, k=2, n=64, source=src.data_ptr(), desc="d", rec="r", cap="c",
             cur="u", scratch=bufs["scratch"].data_ptr()):
        arr = (runtime.SdxJsonIn * max(len(ins), 1))(*ins) if ins is not None else None
        mk = lambda key: (ctypes.c_void_p * 2)(*[o[key].data_ptr() for o in outs])     # noqa: E731
        darr = mk("desc") if desc == "d" else desc
        rarr = mk("rec") if rec == "r" else rec
        uarr = mk("cursor") if cur == "u" else cur
        carr = (ctypes.c_uint32 * 2)(*[o["rec_cap"] for o in outs]) if cap == "c" else cap
        return lib.sdx_filter_records(bank, table, arr, k, n, source, darr, rarr, carr, uarr, scratch, eng.stream_ptr())

    ptrs = lambda *v: (ctypes.c_void_p * 2)(*v)       # noqa: E731
    d0, d1 = (o["desc"].data_ptr() for o in outs)
    r0, r1 = (o["rec"].data_ptr() for o in outs)
    u0, u1 = (o["cursor"].data_ptr() for o in outs)
    twice = [c.ins[0], c.ins[0]]
    bad_kind = [c.ins[0], eng.json_in(4, c.outs[1], {"meta": c.meta}, 64)]
    other_n = [c.ins[0], eng.json_in(1, c.outs[1], {"meta": c.meta}, 63)]
    no_rec = runtime.SdxJsonIn()
    ctypes.memmove(ctypes.byref(no_rec), ctypes.byref(c.ins[1]), ctypes.sizeof(runtime.SdxJsonIn))
    no_rec.rec_dev = None
    no_cur = runtime.SdxJsonIn()
    ctypes.memmove(ctypes.byref(no_cur), ctypes.byref(c.ins[1]), ctypes.sizeof(runtime.SdxJsonIn))
    no_cur.cursor_dev = None
    other_bank = runtime.DeviceProfileTable(eng, None, blob=pack_table([[range(5)] * 4], [0], counts=(130, 66, 12, 19)))
    cases = {
        "null bank": dict(bank=None), "null table": dict(table=None), "null kinds": dict(ins=None),
        "k = 0": dict(k=0), "k = 5": dict(k=5), "n < 0": dict(n=-1),
        "a kind twice": dict(ins=twice), "a bad kind": dict(ins=bad_kind), "another n": dict(ins=other_n),
        "a null rec_dev": dict(ins=[c.ins[0], no_rec]), "a null cursor_dev": dict(ins=[c.ins[0], no_cur]),
        "null desc_out": dict(desc=None), "null rec_out": dict(rec=None), "null rec_cap": dict(cap=None), "null cursor_out": dict(cur=None),
        "a null desc entry": dict(desc=ptrs(d0, None)), "a null rec entry": dict(rec=ptrs(None, r1)),
        "a null cursor entry": dict(cur=ptrs(u0, None)), "null scratch": dict(scratch=None),
        "misaligned source": dict(source=src.data_ptr() + 2), "misaligned scratch": dict(scratch=bufs["scratch"].data_ptr() + 8),
        "misaligned desc": dict(desc=ptrs(d0 + 2, d1)), "misaligned rec": dict(rec=ptrs(r0, r1 + 8)),
        "misaligned cursor": dict(cur=ptrs(u0, u1 + 1)),
        "a table of another bank": dict(table=other_bank.handle),
    }
    for name, kw in cases.items():
        assert call(**kw) == EINVAL, name
        assert b"sdx_filter_records" in lib.sdx_last_error(), name
    t.cuda.synchronize()
    for o in outs:                                                   # nothing was launched
        assert set(o["desc"].cpu().numpy().tolist()) == {9} and set(o["cursor"].view(t.uint8).cpu().numpy().tolist()) == {9}
    assert call() == 0
    t.cuda.synchronize()
    assert outs[0]["cursor"].cpu().numpy().view(np.uint32)[1] == Chunk.CUR[1]
    # a blob the validator refuses uploads nothing
    with pytest.raises(RuntimeError, match="of_source"):
        runtime.DeviceProfileTable(eng, None, blob=pack_table([ALL], [1]))
    # the Python layer's own checks
    with pytest.raises(ValueError):
        eng.filter_records(four.dev, c.ins[:1], 64, bufs)
    with pytest.raises(ValueError):
        eng.filter_records(four.dev, c.ins, 64, bufs, source=src[:10])


# ---- downstream consumers --------------------------------------------------------------------------------------
def planted_filtered(c, table):
    """The chunk planted already filtered by the restatement: the same heaps and payload offsets, the kept records
    dense in line order, the cursors' record counts."""
    from pysignalduino_amd import runtime
    t, eng = c.eng.torch, c.eng
    outs = []
    for x, (desc, stored, cur) in enumerate(c.expect(table)):
        rec = np.zeros(max(int(cur[0]), 1), runtime.RES_DT)
        for begin, kept in stored:
            for j, r in enumerate(kept):
                rec[begin + j] = r
        o = dict(c.outs[x])
        o.update(desc=c.dev(desc), rec=c.dev(rec), cursor=t.from_numpy(cur.view(np.int32).copy()).to(eng.dev), rec_cap=len(rec))
        outs.append(o)
    return outs


def texts(eng, jo, items):
    off = jo["off"][:items].cpu().numpy().astype(np.int64)
    ln = jo["len"][:items].cpu().numpy().astype(np.int64)
    buf = jo["json"].cpu().numpy().tobytes()
    assert int(jo["cursor"][1].item()) == 0
    return [buf[o: o + k] if k else None for o, k in zip(off.tolist(), ln.tolist())]


def test_downstream_consumers_on_the_filtered_outputs(eng, four):
    from pysignalduino_amd.routes import DEFAULT_ROUTES, RouteTable
    t = eng.torch
    n = 420
    rng = np.random.default_rng(33)
    pre = [b"P7#", b"P61#", b"W33#", b"u40#", b"s", b"i", b"TX", b"P1#"]
    lines = []
    for i in range(n):
        if i % 9 == 7:
            lines.append([])
            continue
        kd = (i // 5) % 4
        k = int(rng.integers(1, 6))
        base = [(int(rng.integers(0, COUNTS[kd])), pre[int(rng.integers(0, len(pre)))] + b"%04X" % int(rng.integers(0, 3)))
                for _ in range(k)]
        if i % 4 == 1 and lines and lines[-1] and lines[-1][0][0] == kd:
            base = list(lines[-1][0][1])                  # a repeat of the previous line's list
        lines.append([(kd, base, RAISED if i % 31 == 30 else OK)])
    src = rng.integers(0, 4, n)
    for i in range(1, n):
        if i % 4 == 1:
            src[i] = src[i - 1]                           # the repeats come from the receiver that sent the line before
    c = Chunk(eng, lines, kinds=(0, 1, 2, 3), sources=src)
    got, exp, f_outs, bufs = c.check(four)
    p_outs = planted_filtered(c, four)
    changed = sum(int((e[0]["n_rec"] != d["n_rec"]).sum()) for e, d in zip(exp, c.desc))
    first = sum(1 for x, e in enumerate(exp) for _, kept in e[1]                    # a list kept with a new first message
                if kept and kept[0].tobytes() != c.rec[x][int(c.desc[x][int(kept[0]["msg"])]["rec_begin"])].tobytes())
    assert changed > 100 and first > 20

    results = []
    for outs in (f_outs, p_outs):
        r = {}
        lo = {"meta": c.meta, "pat_val": c.pat_val, "cp_slot": c.cp_slot}
        r["json0"] = []
        for x, kd in enumerate(c.kinds):                  # sdx_serialize_json, one text per record
            jo = eng.alloc_json(outs[x]["rec_cap"], 1 << 20)
            jo["len"].zero_()
            eng.launch_json(kd, outs[x], lo, n, jo, first_only=0)
            t.cuda.synchronize()
            r["json0"].append(texts(eng, jo, int(exp[x][2][0])))
        jo = eng.alloc_json(n, 1 << 20)                   # ... and one per line, sparse: the kinds share the outputs
        jo["len"].zero_()
        for x, kd in enumerate(c.kinds):
            eng.launch_json(kd, outs[x], lo, n, jo, first_only=2)
        t.cuda.synchronize()
        r["json2"] = texts(eng, jo, n)
        ins = [c.json_in(kd, o) for kd, o in zip(c.kinds, outs)]
        b = eng.alloc_routes(n, mask=True, skip=False, pick=True, views=4)
        eng.route_records(eng.route_table(RouteTable(DEFAULT_ROUTES)), ins, n, b["route"], b["pick"], b["views"], mask=b["mask"])
        rep, scratch = eng.alloc_repeat_sources(n, 4)
        state = eng.alloc_repeat_state(sources=4)
        eng.mark_repeats_by_source(ins, n, c.d_src, 4, None, None, rep, scratch, state)
        t.cuda.synchronize()
        r["route"] = [b[k][:n].cpu().numpy().tobytes() for k in ("route", "pick", "mask")] + [v[: 8 * n].cpu().numpy().tobytes() for v in b["views"]]
        r["repeat"] = (rep[:n].cpu().numpy().tobytes(), state.cpu().numpy().tobytes())
        results.append(r)
    a, b = results
    assert a["json0"] == b["json0"] and a["json2"] == b["json2"] and a["route"] == b["route"] and a["repeat"] == b["repeat"]
    assert sum(x is not None for x in a["json2"]) > 150 and sum(len(k) for k in a["json0"]) == sum(int(e[2][0]) for e in exp)
    assert all(x is not None for k in a["json0"] for x in k)
    assert 0 < sum(a["repeat"][0]) < n
