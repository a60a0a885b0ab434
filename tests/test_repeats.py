"""Repeat suppression on the device: sdx_mark_repeats, sdx_serialize_json_skip and the
``collapse_repeats`` argument of the front end and the stream.

The expected masks come from ``restate`` below, a serial restatement of the definition.  Its inputs are
never taken from the code under test: the reference-recorded (kind, protocol_id, payload) of the goldens
("e2e" of tests/golden/lines_golden.json.gz, lines_general_golden.json.gz), or -- for the kernel-level
cases -- the keys the test itself planted into hand-built launch outputs."""
import numpy as np
import pytest

from oracle import json_oracle as J

pytestmark = pytest.mark.gpu


def restate(keys):
    """keys[i]: the line's key, None for a line without results -> the repeat mask."""
    mask, prev = [], None
    for k in keys:
        if k is None:
            mask.append(0)
            continue
        mask.append(int(k == prev))
        prev = k
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
    items[i]: None, or (kind, proto, payload[, later results[, status]]); every payload is followed by a
    byte that differs from line to line, so a compare that ran past a payload's end would see it."""

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
                later = it[3] if len(it) > 3 else []
                desc[i] = (len(recs), 1 + len(later), it[4] if len(it) > 4 else runtime.ST_OK, 0)
                for proto, payload in [(it[1], it[2])] + list(later):
                    recs.append((len(heap), len(payload), proto, 0, i))
                    heap += payload + bytes([(7 * i + 1) & 0xFF])
            rec = np.array(recs, runtime.RES_DT) if recs else np.zeros(1, runtime.RES_DT)
            dev = lambda a: t.from_numpy(np.frombuffer(a.tobytes() if hasattr(a, "tobytes") else bytes(a),  # noqa: E731
                                                       np.uint8).copy()).to(eng.dev)
            out = {"desc": dev(desc), "rec": dev(rec), "heap": dev(heap), "rec_cap": len(rec),
                   "cursor": t.zeros(4, dtype=t.int32, device=eng.dev)}
            self.keep.append(out)
            self.ins.append(eng.json_in(kd, out, {"meta": dummy}, n))

    def mark(self, state):
        rep, scratch = self.eng.alloc_repeat(self.n)
        rep.fill_(9)   # every entry must be written
        self.eng.mark_repeats(self.ins, self.n, rep, scratch, state)
        return rep[: self.n].cpu().numpy().tolist()


def planted_keys(items):
    from pysignalduino_amd import runtime
    return [None if it is None or (len(it) > 4 and it[4] != runtime.ST_OK) else (it[0], it[1], bytes(it[2]))
            for it in items]


def check_chunks(eng, chunks):
    """The chunks of one stream through sdx_mark_repeats with one carried state == restate over all lines."""
    state = eng.alloc_repeat_state()
    got = []
    for items in chunks:
        got += Planted(eng, items).mark(state) if items else []
    exp = restate(planted_keys([it for items in chunks for it in items]))
    assert got == exp, [(i, g, e) for i, (g, e) in enumerate(zip(got, exp)) if g != e][:10]


def test_payload_compare_edges(eng):
    from pysignalduino_amd import runtime
    A = bytes(range(65, 65 + 17))
    items = []
    for ln in (7, 8, 9, 15, 16, 17):     # either side of any 8- or 16-byte compare step
        p = A[:ln]
        items += [(0, 3, p), (0, 3, p),                           # equal: a repeat
                  (0, 3, p[:-1] + b"!"),                          # differs only in the last byte
                  (0, 3, p[:-1]), (0, 3, p),                      # differ only in length (prefix, both ways)
                  (0, 4, p), (0, 4, p)]                           # another protocol, the same bytes
    items += [(0, 5, b"same", [(6, b"x")]), (0, 5, b"same", [(7, b"yy")]), (0, 5, b"same")]   # later results differ: repeats
    items += [(2, 1, b"PAYLOAD"), (1, 1, b"PAYLOAD"), (1, 1, b"PAYLOAD"), (2, 1, b"PAYLOAD")]  # MC / MS, same proto and bytes
    items += [(3, 0, b""), (3, 0, b""), (0, 0, b"")]                                            # empty payloads
    items += [(0, 9, b"r"), (0, 9, b"r", [], runtime.ST_RAISED), None, (0, 9, b"r")]            # a raised line is no result
    big = bytes((i * 31 + 7) & 0xFF for i in range(65535))
    items += [(1, 2, big), (1, 2, big), (1, 2, big[:-1] + b"\x00"), (1, 2, big)]              # the contract's longest payload
    check_chunks(eng, [items])
    # the same across a chunk boundary at every position: the carried state compares the same way
    for cut in (1, 2, 5, len(items) - 3, len(items) - 1):
        check_chunks(eng, [items[:cut], items[cut:]])


def test_scan_boundaries(eng):
    T = eng.repeat_tile()
    a, b = (0, 1, b"aaaaaaaa"), (0, 1, b"bbbbbbbb")

    def runs(n, bounds):   # line i belongs to run number (bounds passed), the runs alternate a / b
        return [(a, b)[sum(i >= x for x in bounds) % 2] for i in range(n)]
    cases = [[a], [a] * T, [a] * (T + 1), [None], [None] * (T + 1),
             runs(2 * T + 70, [63]), runs(2 * T + 70, [64]), runs(2 * T + 70, [65]),
             runs(2 * T + 70, [T - 1]), runs(2 * T + 70, [T]), runs(2 * T + 70, [T + 1]), runs(2 * T + 70, [2 * T]),
             runs(2 * T + 70, [63, 64, 65, T - 1, T, T + 1, 2 * T]),
             runs(3 * T + 5, [T - 2, 2 * T + 2]),                     # a run that spans three tiles
             [a] * (T - 3) + [None] * (T + 6) + [a] * T,              # a tile without results inside a run
             [a] * 5 + [None] * (3 * T) + [b] + [None] * T + [b]]
    rng = np.random.default_rng(5)
    for n in (1000, 4 * T + 1):   # sparse results, random short runs
        pick = rng.integers(0, 6, n)
        cases.append([None if p > 2 else (0, int(p), b"k" * (int(p) + 1)) for p in pick])
    for items in cases:
        check_chunks(eng, [items])
    # chunks of one stream: a run across a boundary, across a chunk without results, a chunk's last line as head
    check_chunks(eng, [[a] * 3 + [None] * 2, [a, a, b], [None] * (T + 1), [b, b, a], [a], [], [a, None], [None, a, b]])


def test_a_new_state_has_no_previous_key(eng):
    a = (0, 1, b"aaaa")
    st = eng.alloc_repeat_state()
    assert Planted(eng, [a, a]).mark(st) == [0, 1]
    assert Planted(eng, [a]).mark(st) == [1]
    assert Planted(eng, [a]).mark(eng.alloc_repeat_state()) == [0]


def test_mark_repeats_refuses_bad_arguments(eng):
    p = Planted(eng, [(0, 1, b"x"), (1, 1, b"x")])
    rep, scratch = eng.alloc_repeat(2)
    st = eng.alloc_repeat_state()
    with pytest.raises(RuntimeError, match="given twice"):
        eng.mark_repeats([p.ins[0], p.ins[0]], 2, rep, scratch, st)
    with pytest.raises(RuntimeError, match="chunk's n"):
        eng.mark_repeats(p.ins, 1, rep, scratch, st)
    with pytest.raises(ValueError):
        eng.mark_repeats(p.ins, 2, rep, scratch[:16], st)


# ---- the serialiser's masked entry ------------------------------------------------------------------
def _json_runner(lines):
    """MU launch of ``lines`` -> run(skip, through the skip entry?) -> (json bytes used, off, len, per-line texts)."""
    import ctypes
    from pysignalduino_amd import runtime
    from pysignalduino_amd.frontend import LineBatch, SignalParser, pack_lines
    sp = SignalParser()
    eng = sp.protocols._ensure()
    data, offsets, bad = pack_lines(lines)
    n = len(lines)
    lb = LineBatch(eng, data, offsets)
    lb.launch()
    sels, cnt = lb.selections()
    out = eng.alloc_out(n, 8 * n + 1024, 200 * n + 65536, eng.pulses_work_bytes(n))
    eng.launch_pulses(runtime.KIND_MU, lb.pulse_batch(), out, sel=sels[runtime.SEL_MU_SHORT])
    lo = {"meta": lb.meta, "pat_val": lb.pat_val, "cp_slot": lb.cp_slot}

    def run(skip, use_skip_entry):
        keep = (lb, out)   # noqa: F841  (the launch's buffers live as long as the runner)
        jo = eng.alloc_json(n, 600 * n + 65536)
        for f in ("json", "off", "len"):
            jo[f].zero_()
        if use_skip_entry:
            ji = eng.json_in(runtime.KIND_MU, out, lo, n, True)
            o = runtime.SdxJsonOut(runtime._ptr(jo["json"]), runtime._ptr(jo["off"]), runtime._ptr(jo["len"]),
                                   runtime._ptr(jo["cursor"]), jo["cap"], 0)
            runtime._check(eng.lib, eng.lib.sdx_serialize_json_skip(eng.handle, ctypes.byref(ji), ctypes.byref(o),
                                                                   runtime._ptr(skip), eng.stream_ptr()))
        else:
            eng.launch_json(runtime.KIND_MU, out, lo, n, jo, first_only=True)
        used = int(jo["cursor"].cpu().numpy()[0])
        off, ln = jo["off"][:n].cpu().numpy(), jo["len"][:n].cpu().numpy()
        blob = jo["json"][:used].cpu().numpy().tobytes()
        return blob, off, ln, [blob[o: o + k] for o, k in zip(off.tolist(), ln.tolist())]
    return eng, run


def test_serialize_json_skip_null_and_zero_mask_are_serialize_json(golden):
    """skip_dev = NULL and an all-zero mask give sdx_serialize_json's output byte for byte, in json, off
    and len.  Compared on 64 lines: one wave, whose texts take the buffer in lane order (waves reserve
    their bytes with one atomic each, so the order of several waves in the buffer is free)."""
    mu = [c["line"] for c in golden("lines_golden.json.gz") if c.get("e2e") and c["e2e"][0][3][1] == "MU"][:64]
    assert len(mu) == 64
    eng, run = _json_runner(mu)
    t = eng.torch
    base = run(None, False)
    assert (base[2] > 0).sum() > 32
    for got in (run(None, True), run(t.zeros(64, dtype=t.uint8, device=eng.dev), True)):
        assert got[0] == base[0] and (got[1] == base[1]).all() and (got[2] == base[2]).all()


def test_serialize_json_skip_removes_text_and_space(golden):
    """Over all golden lines (several workgroups): every line's own text is sdx_serialize_json's unless
    its mask entry is set; a masked line has len 0 and its bytes are not reserved."""
    lines = [c["line"] for c in golden("lines_golden.json.gz")]
    n = len(lines)
    eng, run = _json_runner(lines)
    t = eng.torch
    base = run(None, False)
    rows = np.nonzero(base[2] > 0)[0]
    assert len(rows) > 100
    for got in (run(None, True), run(t.zeros(n, dtype=t.uint8, device=eng.dev), True)):
        assert len(got[0]) == len(base[0]) and (got[2] == base[2]).all() and got[3] == base[3]
    mask = np.zeros(n, np.uint8)
    mask[rows[::3]] = 1
    mask[0] = 1
    got = run(t.from_numpy(mask).to(eng.dev), True)
    assert len(got[0]) == len(base[0]) - int(base[2][mask != 0].sum())
    for i in range(n):
        assert got[3][i] == (b"" if mask[i] else base[3][i])


# ---- front end: goldens with repeats ----------------------------------------------------------------
@pytest.fixture(scope="module")
def corpus(golden):
    """Golden lines the current front end answers without ContractError, every result-bearing one 1 to 4
    times in a row with non-decoding golden lines inside the runs -> (lines, keys, texts)."""
    from pysignalduino_amd.frontend import SignalParser
    cases = [c for c in golden("lines_golden.json.gz") if "\n" not in c["line"].strip("\n")]
    plain = SignalParser().parse_lines_json([c["line"] for c in cases])
    ok = [c for c, g in zip(cases, plain) if not isinstance(g, Exception)]
    bearing = [c for c in cases if c.get("e2e")]
    lost = [c for c, g in zip(cases, plain) if isinstance(g, Exception) and c.get("e2e")]
    assert len(lost) <= 0.05 * len(bearing), (len(lost), len(bearing))   # the cap test_lines.py allows
    noise = [c for c in ok if not c.get("e2e")]
    rng = np.random.default_rng(11)
    lines, keys, texts = [], [], []

    def add(c):
        lines.append(c["line"].strip("\n"))
        keys.append(e2e_key(c.get("e2e", [])))
        texts.append(J.published(c.get("e2e", [])))
    for c in ok:
        if not c.get("e2e"):
            add(c)
            continue
        for r in range(int(rng.integers(1, 5))):
            add(c)
            if rng.integers(0, 3) == 0:
                add(noise[int(rng.integers(0, len(noise)))])
    assert sum(k is not None for k in keys) > 600 and sum(restate(keys)) > 300
    return lines, keys, texts


def expect_texts(keys, texts):
    return [None if m else t for m, t in zip(restate(keys), texts)]


def test_parse_lines_json_collapses_golden_repeats(corpus):
    from pysignalduino_amd.frontend import SignalParser
    lines, keys, texts = corpus
    sp = SignalParser()
    got = sp.parse_lines_json(lines, collapse_repeats=True)
    assert sp.last_repeat_mask.tolist() == restate(keys)
    assert got == expect_texts(keys, texts)
    # the byte entry, and the default stays what it was
    raw = "".join(ln + "\n" for ln in lines).encode("latin-1")
    assert sp.parse_bytes_json(raw, collapse_repeats=True) == got
    assert sp.parse_lines_json(lines) == texts


def test_parse_lines_objects_collapse(corpus):
    from pysignalduino_amd.frontend import SignalParser
    lines, keys, _ = corpus
    sp = SignalParser()
    plain = sp.parse_lines(lines)
    got = sp.parse_lines(lines, collapse_repeats=True)
    mask = restate(keys)
    assert sp.last_repeat_mask.tolist() == mask
    for m, g, p in zip(mask, got, plain):
        assert g == [] if m else [(d.protocol_id, d.payload) for d in g] == [(d.protocol_id, d.payload) for d in p]
    raw = "".join(ln + "\n" for ln in lines).encode("latin-1")
    assert [len(x) for x in sp.parse_bytes(raw, collapse_repeats=True)] == [len(x) for x in got]


def test_mn_lines_collapse(golden):
    """MN goldens (one rfmode): each decoding line three times -> only its first text."""
    from pysignalduino_amd.frontend import SignalParser
    from pysignalduino_amd.sd_protocols import SDProtocols
    cases = golden("mn_golden.json.gz")["lines"]
    rf = cases[0][2]
    sel = [c for c in cases if c[2] == rf][:300]
    lines, keys, texts = [], [], []
    for c in sel:
        out = c[3].get("out", [])
        for _ in range(3 if out else 1):
            lines.append(c[1])
            keys.append(("MN", out[0][0], out[0][1]) if out else None)
            texts.append(J.published(out))
    sp = SignalParser(SDProtocols(), rfmode=rf)
    plain = sp.parse_lines_json(lines)
    keep = [i for i, g in enumerate(plain) if not isinstance(g, Exception)]
    lines, keys, texts = ([x[i] for i in keep] for x in (lines, keys, texts))
    assert sum(restate(keys)) > 50
    assert sp.parse_lines_json(lines, collapse_repeats=True) == expect_texts(keys, texts)


# ---- stream -----------------------------------------------------------------------------------------
def stream_results(sp, output, feed, **kw):
    """-> (mask, texts or None) over all chunks; feed(ls) submits."""
    ls = sp.stream(chunk_lines=257, chunk_bytes=1 << 18, output=output, lag=2, collapse_repeats=True, **kw)
    feed(ls)
    mask, texts = [], []
    for r in ls.drain():
        assert r.repeat.dtype == np.uint8 and len(r.repeat) == r.n
        mask += r.repeat.tolist()
        if output == "json":
            t = r.texts()
            assert [i for i, _ in r.items()] == [i for i, x in enumerate(t) if x is not None]
            texts += t
    return mask, texts


@pytest.fixture(scope="module")
def stream_corpus(corpus):
    """In front of the golden corpus: a run across a chunk boundary, a run head that is a chunk's last
    line, a run across a chunk without results (chunks of 257 lines)."""
    lines, keys, texts = corpus
    rb = [i for i, k in enumerate(keys) if k is not None]
    ia = rb[0]
    ib = next(i for i in rb if keys[i] != keys[ia])
    inz = next(i for i, k in enumerate(keys) if k is None)
    order = [ia] * 3 + [inz] * 253 + [ib] + [ib] * 2 + [inz] * 255 + [inz] * 257 + [ib, ia] + [inz] * 255 + [ia] * 2
    pick = order + list(range(len(lines)))
    return [lines[i] for i in pick], [keys[i] for i in pick], [texts[i] for i in pick]


@pytest.mark.parametrize("output", ["json", "wire"])
def test_stream_collapses_across_chunks(stream_corpus, output):
    from pysignalduino_amd.frontend import SignalParser
    lines, keys, texts = stream_corpus
    sp = SignalParser()
    exp = restate(keys)
    assert exp[256] == 0 and exp[257] == 1 and exp[3 * 257] == 1    # the planted boundary cases

    def by_lines(ls):
        for a in range(0, len(lines), 257):
            ls.submit(lines[a: a + 257])

    raw = "".join(ln + "\n" for ln in lines).encode("latin-1")

    def by_bytes(ls):
        cuts = [0, 1, 777, 778, 40_001, 40_002, len(raw) // 2, len(raw)]
        for a, b in zip(cuts, cuts[1:]):
            ls.submit_bytes(raw[a:b])
        ls.close_bytes()
    for feed in (by_lines, by_bytes):
        mask, got = stream_results(sp, output, feed)
        assert mask == exp
        if output == "json":
            assert got == expect_texts(keys, texts)
    if output == "json":
        assert sp.parse_lines_json(lines, collapse_repeats=True) == expect_texts(keys, texts)
    # d2h accounting: the mask travels, the skipped texts do not
    ls_on = sp.stream(chunk_lines=257, chunk_bytes=1 << 18, output=output, lag=2, collapse_repeats=True)
    ls_off = sp.stream(chunk_lines=257, chunk_bytes=1 << 18, output=output, lag=2)
    for ls in (ls_on, ls_off):
        by_lines(ls)
        ls.drain()
    if output == "json":
        assert ls_on.d2h_bytes < ls_off.d2h_bytes
    else:
        assert ls_on.d2h_bytes > ls_off.d2h_bytes


@pytest.mark.parametrize("output", ["json", "wire"])
def test_stream_host_resolved_lines(corpus, golden, output):
    """An LS_GENERAL line (resolved by the batch API on the host) inside a run, between two runs, twice
    in a row, as a chunk's last line and as the next chunk's first."""
    from pysignalduino_amd.frontend import SignalParser
    lines, keys, texts = corpus
    gen = next(c for c in golden("lines_general_golden.json.gz")
               if c.get("e2e") and "P10=" in c["line"] and "\n" not in c["line"].strip("\n") and len(c["line"]) < 2000)
    G = (gen["line"].strip("\n"), e2e_key(gen["e2e"]), J.published(gen["e2e"]))
    rb = [i for i, k in enumerate(keys) if k is not None]
    ia = rb[0]
    ib = next(i for i in rb if keys[i] != keys[ia])
    inz = next(i for i, k in enumerate(keys) if k is None)
    A, Bq, N = ((lines[i], keys[i], texts[i]) for i in (ia, ib, inz))
    seq = [A, A, G, A, A,                 # inside a run: the device skipped the A after G, it must be published
           Bq, Bq, G, A, A,               # between two runs
           G, G, N, G, A, G, G]           # host rows repeating host rows, noise in between
    seq += [N] * (256 - len(seq)) + [G]   # G is the first chunk's last line ...
    seq += [G, G, A, A, N] + [N] * 251 + [A]      # ... and repeats into the next; A's run then spans two boundaries
    seq += [A, G] + [N] * 254 + [G]
    seq += [N] * 257                      # a chunk without results behind a host row
    seq += [G, A, A, Bq]
    ls_lines = [s[0] for s in seq]
    k = [s[1] for s in seq]
    tx = [s[2] for s in seq]
    sp = SignalParser()

    def feed(ls):
        for a in range(0, len(seq), 257):
            ls.submit(ls_lines[a: a + 257])
    mask, got = stream_results(sp, output, feed)
    assert mask == restate(k)
    if output == "json":
        assert got == expect_texts(k, tx)
        assert sp.parse_lines_json(ls_lines, collapse_repeats=True) == expect_texts(k, tx)
        assert sp.last_repeat_mask.tolist() == restate(k)
