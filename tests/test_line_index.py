"""sdx_index_records + sdx_serialize_json_lines through the C ABI on planted launch outputs.

Expected values: ``first`` is a numpy restatement (cumsum of the per-line counts the test planted: the n_rec of an OK
descriptor, 0 for every other status and for a skipped line).  The texts are those ``sdx_serialize_json`` with
first_only = 0 -- the serialiser the suite already holds against the reference -- builds for every record of every
kind, placed by the HOST at first[line] + (the record's place in its line's list); a few hand cases are also compared
with oracle/json_oracle.message_to_json.  0xA5 stands behind first[n], behind off / len[rec_max] and behind json_cap:
nothing may be stored there."""
import ctypes

import numpy as np
import pytest

from oracle import json_oracle as J

from test_routes import eng  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

OK, RAISED, OVF_TILE, OVF_OUT, ABSENT = 0, 1, 2, 3, 0xFF
BAD = (RAISED, OVF_OUT, OVF_TILE, ABSENT)
EINVAL = -1
COUNTS = (129, 66, 12, 19)      # this bank's class counts (test_profiles_host.py pins them)
SIZES = (0, 1, 2, 5, 64, 65, 200)
GUARD = 8                       # entries of 0xA5 behind first / off / len
A5_32 = 0xA5A5A5A5


class Plant:
    """Planted launch outputs.  lines[i]: None (the line belongs to no kind) or (kind, records, status); a line's
    records stand together in its kind's array whatever its status -- a line that is not OK keeps stale records, with
    a descriptor that still names them.  ``stale``: records that no descriptor names, "front" of the first line's,
    "between" the lines' and "behind" the last one's; their msg is a line of the chunk, as a launch writes it."""

    def __init__(self, eng, lines, kinds, stale=("front", "between", "behind")):
        from pysignalduino_amd import runtime
        t = eng.torch
        self.eng, self.n, self.lines, self.kinds = eng, len(lines), lines, list(kinds)
        n = self.n
        up = lambda a: t.from_numpy(np.frombuffer(a.tobytes(), np.uint8).copy()).to(eng.dev)   # noqa: E731
        self.lo = {"meta": t.zeros(32 * max(n, 1), dtype=t.uint8, device=eng.dev),
                   "pat_val": t.full((10 * max(n, 1),), 377.5, dtype=t.float64, device=eng.dev),
                   "cp_slot": t.zeros(max(n, 1), dtype=t.int8, device=eng.dev)}
        self.outs, self.desc, self.rec = [], [], []
        for kd in self.kinds:
            desc = np.zeros(max(n, 1), runtime.DESC_DT)
            recs, heap = [], bytearray()

            def add(i, j):
                payload = b"%X" % (977 * i + 31 * j + kd)
                recs.append((len(heap), len(payload), (i + 3 * j) % COUNTS[kd], 8 + j, i))
                heap.extend(payload)
            mine = [i for i, ln in enumerate(lines) if ln is not None and ln[0] == kd]
            if "front" in stale and mine:
                for j in range(3):
                    add(mine[0], 100 + j)
            for x, i in enumerate(mine):
                _, cnt, st = lines[i]
                desc[i] = (len(recs), cnt, st, 2 if st == RAISED else 0)
                for j in range(cnt):
                    add(i, j)
                if "between" in stale and x % 3 == 0:
                    add(i, 300)
                    add(mine[(x + 1) % len(mine)], 301)
            if "behind" in stale and mine:
                for j in range(5):
                    add(mine[-1], 400 + j)
            rec = np.array(recs, runtime.RES_DT) if recs else np.zeros(1, runtime.RES_DT)
            cur = np.array([len(recs), len(heap), 0, 0], np.uint32)
            hnp = np.frombuffer(bytes(heap) + b"\xA5" * 64, np.uint8)
            self.outs.append({"desc": up(desc), "rec": up(rec), "heap": up(hnp), "rec_cap": max(len(recs), 1),
                              "heap_cap": len(heap), "cursor": t.from_numpy(cur.view(np.int32).copy()).to(eng.dev), "n": n})
            self.desc.append(desc)
            self.rec.append(rec)
        self._ref = None

    def ins(self):
        return [self.eng.json_in(kd, o, self.lo, self.n, 0) for kd, o in zip(self.kinds, self.outs)]

    def counts(self, skip=None):
        c = np.zeros(self.n, np.int64)
        for i, ln in enumerate(self.lines):
            if ln is not None and ln[0] in self.kinds and ln[2] == OK and not (skip is not None and skip[i]):
                c[i] = ln[1]
        return c

    def ref_texts(self):
        """Per kind, the text of every record of its array: sdx_serialize_json, first_only = 0 (computed once)."""
        if self._ref is None:
            eng, t = self.eng, self.eng.torch
            self._ref = []
            for kd, o, rec in zip(self.kinds, self.outs, self.rec):
                jo = eng.alloc_json(o["rec_cap"], 400 * o["rec_cap"] + 4096)
                jo["len"].zero_()
                eng.launch_json(kd, o, self.lo, self.n, jo, first_only=0)
                t.cuda.synchronize()
                cur = jo["cursor"].cpu().numpy()
                assert not cur[1]
                blob = jo["json"][: int(cur[0])].cpu().numpy().tobytes()
                off, ln = jo["off"].cpu().numpy().tolist(), jo["len"].cpu().numpy().tolist()
                self._ref.append([blob[a: a + b] for a, b in zip(off, ln)])
        return self._ref

    def expect(self, skip=None):
        """-> (first, the chunk's texts by chunk record index) by the definition, placed on the host."""
        c = self.counts(skip)
        first = np.concatenate([[0], np.cumsum(c)])
        ref = self.ref_texts()
        texts = [None] * int(first[-1])
        for x, kd in enumerate(self.kinds):
            d = self.desc[x]
            for i in np.nonzero(c)[0].tolist():
                if self.lines[i][0] == kd:
                    b = int(d[i]["rec_begin"])
                    for j in range(int(c[i])):
                        texts[int(first[i]) + j] = ref[x][b + j]
        assert all(x for x in texts)
        return first, texts

    def run(self, skip=None, rec_max=None, json_cap=None, index_only=False):
        """The two entries over the chunk, every output inside 0xA5 -> first (with its guard), off, len (with
        theirs), the text buffer with 64 guard bytes, the cursor."""
        eng, t, n = self.eng, self.eng.torch, self.n
        total = int(self.counts(skip).sum())
        rec_max = total if rec_max is None else rec_max
        json_cap = 400 * max(total, 1) if json_cap is None else json_cap
        a5 = lambda k: t.full((k,), 0xA5, dtype=t.uint8, device=eng.dev)   # noqa: E731
        idx = {"first": a5(4 * (n + 1 + GUARD)).view(t.int32), "off": a5(4 * (rec_max + GUARD)).view(t.int32),
               "len": a5(4 * (rec_max + GUARD)).view(t.int32), "json": a5(json_cap + 64),
               "cursor": t.zeros(2, dtype=t.int32, device=eng.dev), "cap": json_cap, "rec_max": rec_max, "n": n,
               "scratch": t.full((int(eng.lib.sdx_index_scratch_bytes(n)),), 0xEE, dtype=t.uint8, device=eng.dev)}
        d_skip = None if skip is None else t.from_numpy(np.asarray(skip, np.uint8)).to(eng.dev)
        eng.index_records(self.ins(), n, idx, skip=d_skip)
        if not index_only:
            for kd, o in zip(self.kinds, self.outs):
                eng.launch_json_lines(kd, o, self.lo, n, idx)
        t.cuda.synchronize()
        u32 = lambda x: x.cpu().numpy().view(np.uint32)   # noqa: E731
        return u32(idx["first"]), u32(idx["off"]), u32(idx["len"]), idx["json"].cpu().numpy(), u32(idx["cursor"])

    def check(self, skip=None, rec_max=None, json_cap=None):
        first, texts = self.expect(skip)
        n, total = self.n, len(texts)
        g_first, off, ln, blob, cur = self.run(skip, rec_max, json_cap)
        rec_max = total if rec_max is None else rec_max
        cap = len(blob) - 64
        assert g_first[: n + 1].tolist() == first.tolist()
        assert (g_first[n + 1:] == A5_32).all()                       # nothing behind first[n]
        stored = min(total, rec_max)
        demand = sum(len(x) for x in texts[:stored])
        assert int(cur[0]) == demand                                  # every placed record reserved its bytes
        assert int(cur[1]) == (1 if total > rec_max or demand > cap else 0)
        assert (off[stored:] == A5_32).all() and (ln[stored:] == A5_32).all()   # nothing at or beyond min(total, rec_max)
        assert (blob[cap:] == 0xA5).all()                             # no byte at or beyond json_cap
        raw = blob.tobytes()
        lost = 0
        spans = []
        for c in range(stored):
            k, o = int(ln[c]), int(off[c])
            if k == 0 and demand > cap:     # text overflow: a wave that did not fit stores length 0
                lost += 1
                continue
            assert k == len(texts[c]) and o + k <= cap and raw[o: o + k] == texts[c], (c, k, o, texts[c][:40])
            spans.append((o, k))
        spans.sort()
        assert all(a + k <= b for (a, k), (b, _) in zip(spans, spans[1:]))     # every text in a range of its own
        if demand <= cap:
            assert lost == 0
        else:
            assert lost > 0
        return first, texts


def mixed(n, seed=0, kinds=(0, 1, 2, 3), sizes=SIZES, bad_every=11):
    """Every line in exactly one kind (or, every 7th, in none), the counts cycling through ``sizes``, a status that
    is not OK every ``bad_every`` lines."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        if i % 7 == 5:
            out.append(None)
            continue
        st = BAD[(i // bad_every) % 4] if bad_every and i % bad_every == 4 else OK
        out.append((kinds[int(rng.integers(0, len(kinds)))], sizes[(i + seed) % len(sizes)], st))
    return out


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_sizes_around_one_block(eng, n):   # noqa: F811
    p = Plant(eng, mixed(n, seed=n), (2, 0, 3, 1))
    first, texts = p.check()
    if n >= 255:
        assert len(texts) > 5000 and first[-1] == len(texts)
    alt = (np.arange(n) % 2).astype(np.uint8)
    for skip in (np.zeros(n, np.uint8), np.ones(n, np.uint8), alt):
        f, tx = p.check(skip=skip)
        assert len(tx) == int(p.counts(skip).sum())
    assert p.check(skip=np.ones(n, np.uint8))[1] == []


def test_257_blocks_and_the_long_line_at_block_edges(eng):   # noqa: F811
    """65,537 lines = 257 blocks: the block-total scan's second round.  A 200-record line first, last, and on both
    sides of a block boundary; everything else short, so the chunk stays small."""
    n = 65537
    lines = mixed(n, seed=3, kinds=(0, 1, 3), sizes=(0, 1, 2, 1, 0), bad_every=13)
    for i in (0, 255, 256, 65535, n - 1):
        lines[i] = (1, 200, OK)
    lines[511], lines[512] = (0, 65, OK), (3, 64, OK)
    p = Plant(eng, lines, (3, 0, 1), stale=("front", "behind"))
    first, texts = p.check()
    assert first[1] == 200 and first[257] - first[255] == 400 and first[n] - first[n - 1] == 200
    assert len(texts) > 30000
    a = p.run(index_only=True)[0]
    b = p.run(index_only=True)[0]
    assert a.tobytes() == b.tobytes()                                 # the same bytes every run
    alt = (np.arange(n) % 2).astype(np.uint8)
    g = p.run(skip=alt, index_only=True)[0]
    assert g[: n + 1].tolist() == np.concatenate([[0], np.cumsum(p.counts(alt))]).tolist()


@pytest.mark.parametrize("kinds", [(0,), (3,), (1, 0), (2, 3), (3, 1, 0), (0, 1, 2, 3), (3, 2, 1, 0), (1, 3, 0, 2)])
def test_one_to_four_kinds_in_any_order(eng, kinds):   # noqa: F811
    p = Plant(eng, mixed(300, seed=len(kinds), kinds=kinds, sizes=(0, 1, 2, 5, 1, 65, 3)), kinds)
    p.check()
    p.check(skip=(np.arange(300) % 3 == 0).astype(np.uint8))


def test_only_ok_descriptors_count(eng):   # noqa: F811
    """Every status but OK gives count 0 although the descriptor names records; stale records in front of, between
    and behind the lines' ranges get no text."""
    lines = [(0, 5, st) for st in (OK, RAISED, OK, OVF_OUT, OVF_TILE, OK, ABSENT)] + [None, (0, 0, OK), (0, 2, OK)]
    p = Plant(eng, lines, (0,))
    first, texts = p.check()
    assert np.diff(first).tolist() == [5, 0, 5, 0, 0, 5, 0, 0, 0, 2]
    assert sum(len(r) for r in p.rec) > len(texts) + 10               # the array holds far more records than get a text


def test_hand_cases_against_the_json_oracle(eng):   # noqa: F811
    """MC and MS lines whose texts are written down from the bank's ids: the reference's own publication."""
    bk = eng.bank
    lines = [(2, 2, OK), (1, 3, OK), None, (2, 1, OK)]
    p = Plant(eng, lines, (1, 2), stale=())
    first, texts = p.check()
    assert first.tolist() == [0, 2, 5, 5, 6]
    exp = []
    for i, ln in enumerate(lines):
        for j in range(ln[1] if ln else 0):
            kd = ln[0]
            proto, payload = (i + 3 * j) % COUNTS[kd], "%X" % (977 * i + 31 * j + kd)
            if kd == 2:
                pid = str(bk.mc_pids[proto])
                exp.append(J.message_to_json(pid, payload, {"protocol_id": pid, "rssi": None, "freq_afc": None}))
            else:   # MS: the raw R string (planted empty) and abs(P[CP]) = 377.5
                exp.append(J.message_to_json(str(bk.ms_pids[proto]), payload, {"bit_length": 8 + j, "rssi": "", "clock": 377.5}))
    assert [x.decode("ascii") for x in texts] == exp


def test_capacities(eng):   # noqa: F811
    p = Plant(eng, mixed(300, seed=5, sizes=(0, 1, 2, 5, 3, 65, 1)), (0, 1, 2, 3))
    first, texts = p.expect()
    total, demand = len(texts), sum(len(x) for x in texts)
    assert total > 2000
    for rec_max in (total, total - 1, total // 2, 0):
        p.check(rec_max=rec_max)
    p.check(json_cap=demand)
    p.check(json_cap=demand - 1)
    p.check(rec_max=total // 2, json_cap=demand // 4)                 # both at once


def test_einval_launches_nothing(eng):   # noqa: F811
    from pysignalduino_amd import runtime
    t, lib = eng.torch, eng.lib
    n = 40
    p = Plant(eng, mixed(n, seed=9), (0, 1, 2, 3))
    first = t.full((4 * (n + 2),), 0xA5, dtype=t.uint8, device=eng.dev)
    scratch = t.zeros(64, dtype=t.uint8, device=eng.dev)
    fp, sp = first.data_ptr(), scratch.data_ptr()

    def call(ins, k=None, n_=n, f=fp, s=sp):
        arr = (runtime.SdxJsonIn * max(len(ins), 1))(*ins) if ins is not None else None
        return lib.sdx_index_records(arr, len(ins) if k is None else k, n_, None, f, s, None)

    def changed(i, **kw):
        ins = p.ins()
        for f, v in kw.items():
            setattr(ins[i], f, v)
        return ins
    good = p.ins()
    assert call(None, k=1) == EINVAL
    assert call(good, k=0) == EINVAL and call(good[:1] * 5, k=5) == EINVAL
    assert call(good, n_=-1) == EINVAL
    assert call(changed(1, kind=7)) == EINVAL and call(changed(1, kind=-1)) == EINVAL
    assert call(changed(2, kind=0)) == EINVAL                          # a kind given twice
    for f in ("desc_dev", "rec_dev", "heap_dev"):
        assert call(changed(3, **{f: None})) == EINVAL, f              # what sdx_mark_repeats refuses
    assert call(changed(0, n=n - 1)) == EINVAL
    assert call(good, f=None) == EINVAL
    assert call(good, s=None) == EINVAL                                # a null scratch with n > 0
    assert call(good, f=fp + 2) == EINVAL and call(good, s=sp + 1) == EINVAL
    assert b"sdx_index_records" in lib.sdx_last_error()
    t.cuda.synchronize()
    assert (first.cpu().numpy() == 0xA5).all()                         # nothing was launched
    # n = 0 needs no scratch and writes first[0] = 0 alone
    ins0 = p.ins()
    for x in ins0:
        x.n = 0
    assert call(ins0, n_=0, s=None) == 0
    t.cuda.synchronize()
    got = first.cpu().numpy()
    assert got[:4].tolist() == [0, 0, 0, 0] and (got[4:] == 0xA5).all()
    # the serialiser's own refusals
    idx = eng.alloc_line_index(n, 64)
    ji = eng.json_in(0, p.outs[0], p.lo, n, 0)
    jo = runtime.SdxJsonOut(idx["json"].data_ptr(), idx["off"].data_ptr(), idx["len"].data_ptr(), idx["cursor"].data_ptr(),
                            idx["cap"], 0)
    ser = lambda ji_, f: lib.sdx_serialize_json_lines(eng.handle, ctypes.byref(ji_), ctypes.byref(jo), f, 64, None)   # noqa: E731
    assert ser(ji, None) == EINVAL and ser(ji, idx["first"].data_ptr() + 1) == EINVAL
    for fo in (1, 2):
        ji1 = eng.json_in(0, p.outs[0], p.lo, n, 0)
        ji1.first_only = fo
        assert ser(ji1, idx["first"].data_ptr()) == EINVAL
    assert lib.sdx_serialize_json_lines(None, ctypes.byref(ji), ctypes.byref(jo), idx["first"].data_ptr(), 64, None) == EINVAL
    with pytest.raises(ValueError):
        eng.index_records(p.ins() * 2, n, idx)
    with pytest.raises(ValueError):
        eng.index_records(p.ins(), n + 1, idx)
