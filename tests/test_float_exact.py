"""The exact float() on the device (csrc/sdx_strtod.h): sdx_parse_floats / SDProtocols.float_batch
against Python's float() bit for bit, and sdx_lines_exact as the second stage of the line front end
-- lines whose P# values leave sdx_parse_lines' one-operation float() decode like the reference's,
and what stays outside the contract keeps raising ContractError."""
import ctypes
import struct

import numpy as np
import pytest

import float_corpus as FC
from oracle import lines_oracle as LO
from oracle import sd_oracle as O


# ---------------------------------------------------------------------------------- CPU ------
def test_new_entries_reject_bad_arguments_without_a_gpu():
    """sdx_parse_floats / sdx_lines_exact validate before any HIP call (runs on the CPU)."""
    from pysignalduino_amd import build, runtime
    build.build()
    lib = runtime.load_library()
    assert lib.sdx_parse_floats(None, None, None, None) == -1
    assert b"sdx_parse_floats" in lib.sdx_last_error()
    assert lib.sdx_lines_exact(None, None, None, 0, None, None) == -1
    assert b"sdx_lines_exact" in lib.sdx_last_error()
    empty = runtime.SdxLines(None, None, 0)
    assert lib.sdx_parse_floats(ctypes.byref(empty), None, None, None) == 0          # n == 0
    one = runtime.SdxLines(None, None, 1)
    assert lib.sdx_parse_floats(ctypes.byref(one), None, None, None) == -1
    assert b"null" in lib.sdx_last_error()
    buf = (ctypes.c_uint8 * 64)()
    a = ctypes.addressof(buf)
    a += -a % 8
    odd = runtime.SdxLines(a + 1, a + 8, 1)                                          # never dereferenced
    assert lib.sdx_parse_floats(ctypes.byref(odd), a + 16, a + 24, None) == -1
    assert b"aligned" in lib.sdx_last_error()
    lo, go = runtime.SdxLinesOut(), runtime.SdxLinesGeneralOut()
    assert lib.sdx_lines_exact(ctypes.byref(empty), ctypes.byref(lo), None, 0, ctypes.byref(go), None) == 0
    assert lib.sdx_lines_exact(ctypes.byref(one), ctypes.byref(lo), None, 1, ctypes.byref(go), None) == -1
    assert b"null" in lib.sdx_last_error()
    assert lib.sdx_lines_exact(ctypes.byref(one), ctypes.byref(lo), None, -1, ctypes.byref(go), None) == -1


# ---------------------------------------------------------------------------------- GPU ------
@pytest.fixture(scope="module")
def proto():
    from pysignalduino_amd.sd_protocols import SDProtocols
    return SDProtocols()


@pytest.fixture(scope="module")
def expected():
    return [FC.expected(s) for s in FC.corpus()]


def _got(res):
    return [(0, 0) if isinstance(r, ValueError) else (1, FC.float_bits(r)) for r in res]


def _assert_equal(strings, got, exp):
    bad = [(s[:60], len(s), g, e) for s, g, e in zip(strings, got, exp) if g != e]
    assert len(got) == len(exp) and not bad, f"{len(bad)} of {len(exp)} differ from float(): {bad[:5]}"


@pytest.mark.gpu
def test_float_batch_whole_corpus_one_launch(proto, expected):
    c = list(FC.corpus())
    _assert_equal(c, _got(proto.float_batch(c)), expected)


@pytest.mark.gpu
def test_float_batch_reversed_and_bytes(proto, expected):
    """The corpus in reverse order (fallback and fast lanes meet differently within a wave), as bytes."""
    c = [s.encode("ascii") for s in reversed(FC.corpus())]
    _assert_equal(c, _got(proto.float_batch(c)), expected[::-1])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 65])
def test_float_batch_small_batches(proto, expected, n):
    """n = 1, and n = 65: a one-lane tail in a second workgroup.  Taken from the end of the midpoint
    group, so that the tail lane runs the digit-array fallback."""
    c = list(FC.corpus())
    k = c.index("9007199254740993.0") - 1 - n   # up to the last string of the midpoint group
    assert k >= 0 and len(c[k + n - 1]) > 300
    _assert_equal(c[k: k + n], _got(proto.float_batch(c[k: k + n])), expected[k: k + n])
    assert proto.float_batch([]) == []


@pytest.mark.gpu
def test_high_byte_is_class_2_and_contract_error(proto):
    from pysignalduino_amd import runtime
    from pysignalduino_amd.packing import ContractError
    cls, bits = runtime.UnitRunner.get(proto.device).parse_floats([b"1.5", b"1.5\xe9", b"\xa02", b"x"])
    assert cls.tolist() == [1, 2, 2, 0] and int(bits[0]) == FC.float_bits(1.5)
    with pytest.raises(ContractError):
        proto.float_batch(["1.5", "1.5\xe9"])
    with pytest.raises(ContractError):
        proto.float_batch([b"1.5\xe9"])
    with pytest.raises(ContractError):
        proto.float_batch([1.5])


# ---- the line front end ---------------------------------------------------------------------
def _flat_msgs(res):
    return [[d.protocol_id, d.payload, d.metadata, [d.raw.line, d.raw.message_type, d.raw.rssi, d.raw.freq_afc]]
            for d in res]


@pytest.mark.gpu
def test_lines_float_golden_end_to_end_without_exceptions(golden):
    """parse_lines on tests/golden/lines_float_golden.json.gz: no exception at all (with the full float()
    no line of the fixture is outside the contract), every line equals the reference's recorded result."""
    from pysignalduino_amd.frontend import SignalParser
    cases = golden("lines_float_golden.json.gz")
    got = SignalParser().parse_lines([c["line"] for c in cases])
    exc = [(i, str(g)) for i, g in enumerate(got) if isinstance(g, BaseException)]
    assert not exc, f"{len(exc)} exceptions; first: {exc[:3]}"
    bad = [(c["src"], c["line"][:80], c.get("e2e", [])[:2], _flat_msgs(g)[:2]) for c, g in zip(cases, got)
           if _flat_msgs(g) != c.get("e2e", [])]
    assert not bad, f"{len(bad)} mismatches; first: {bad[:2]}"
    unsup = [i for i, c in enumerate(cases) if LO.parse_line(c["line"].encode("latin-1"))["status"] == LO.UNSUPPORTED]
    assert len(unsup) == 100 and sum(bool(cases[i].get("e2e")) for i in unsup) == 17


@pytest.mark.gpu
def test_lines_float_golden_json(golden):
    from oracle import json_oracle as J
    from pysignalduino_amd.frontend import SignalParser
    cases = golden("lines_float_golden.json.gz")
    got = SignalParser().parse_lines_json([c["line"] for c in cases])
    exc = [(i, str(g)) for i, g in enumerate(got) if isinstance(g, BaseException)]
    assert not exc, f"{len(exc)} exceptions; first: {exc[:3]}"
    bad = [(i, c["line"][:80], g, J.published(c.get("e2e", []))) for i, (c, g) in enumerate(zip(cases, got))
           if g != J.published(c.get("e2e", []))]
    assert not bad, f"{len(bad)} mismatches; first: {bad[:2]}"


@pytest.mark.gpu
@pytest.mark.parametrize("output", ["json", "wire"])
def test_lines_float_golden_stream(golden, output):
    """SignalParser.stream on the fixture as one chunk, both output modes."""
    from oracle import json_oracle as J
    from pysignalduino_amd import runtime
    from pysignalduino_amd.frontend import SignalParser
    cases = golden("lines_float_golden.json.gz")
    lines = [c["line"].encode("latin-1") for c in cases]
    exp_all = [c.get("e2e", []) for c in cases]
    sp = SignalParser()
    ls = sp.stream(chunk_lines=len(lines), chunk_bytes=sum(map(len, lines)) + 4096, output=output, lag=2)
    ls.submit(lines)
    got = [r.detach() for r in ls.drain()]
    assert len(got) == 1 and got[0].n == len(lines)
    r = got[0]
    if output == "json":
        texts = r.texts()
        exc = [(i, str(g)) for i, g in enumerate(texts) if isinstance(g, BaseException)]
        assert not exc, f"{len(exc)} exceptions; first: {exc[:3]}"
        for i, (e, g) in enumerate(zip(exp_all, texts)):
            assert g == J.published(e), (i, lines[i][:80], g, e)
        return
    bk = sp.protocols._bank
    pid = {"MU": bk.mu_pids, "MS": bk.ms_pids, "MC": bk.mc_pids, "MN": bk.mn_pids}
    lk = {runtime.LINE_MU: "MU", runtime.LINE_MS: "MS", runtime.LINE_MC: "MC", runtime.LINE_MN: "MN"}
    dec = {nm: r.decode(j) for j, nm in enumerate(r.names)}
    nhost = 0
    for i, e in enumerate(exp_all):
        want = [(x[0], x[1]) for x in e]
        if i in r.host:
            g = r.host[i]
            assert not isinstance(g, BaseException), (i, lines[i][:80], g)
            got_i = [(m.protocol_id, m.payload) for m in g]
            nhost += 1
        else:
            nm = lk.get(int(r.kind[i]))
            if int(r.status[i]) != runtime.LS_OK or nm not in dec:
                got_i = []
            else:
                d, rc, h = dec[nm]
                got_i = [(str(pid[nm][int(x["proto"])]),
                          h[int(x["payload_off"]): int(x["payload_off"]) + int(x["payload_len"])].tobytes().decode("latin-1"))
                         for x in rc[int(d[i]["rec_begin"]): int(d[i]["rec_begin"]) + int(d[i]["n_rec"])]]
        assert got_i == want, (i, lines[i][:80], got_i, want)
    assert nhost >= 100


def _py_float(v: bytes):
    try:
        return float(v.decode("latin-1"))
    except ValueError:
        return None


def _expected_table(payload: bytes):
    """{str(int(k[1:])): float(v)} of the payload's pairs in dictionary order (message_unsynced.py:28-35):
    first position, last value, ValueError values skipped."""
    pats = {}
    for k, v in LO._kv(payload):
        if k[:1] == b"P" and k[1:].isdigit():
            f = _py_float(v)
            if f is not None:
                pats[str(int(k[1:]))] = f
    return pats


def _exact_stage(eng, lines):
    """sdx_parse_lines, then sdx_lines_exact on the SDX_LS_UNSUPPORTED rows: host copies of both."""
    import torch
    from pysignalduino_amd import runtime
    from pysignalduino_amd.frontend import LineBatch, pack_lines
    data, offsets, bad = pack_lines(lines)
    assert not bad
    lb = LineBatch(eng, data, offsets)
    lb.launch()
    n = len(lines)
    status0 = lb.status[:n].cpu().numpy().copy()
    rows = np.nonzero(status0 == runtime.LS_UNSUPPORTED)[0]
    m = len(rows)
    sel = torch.from_numpy(rows.astype(np.int32)).to(eng.dev)
    g = {k: torch.empty(sz, dtype=dt, device=eng.dev) for k, sz, dt in
         (("offsets", m, torch.int64), ("len", m, torch.int32), ("npat", m, torch.uint8),
          ("pat_ids", 256 * m, torch.uint8), ("pat_val", 16 * m, torch.float64), ("cp_slot", m, torch.int8),
          ("ms_ok", m, torch.uint8))}
    p = runtime._ptr
    go = runtime.SdxLinesGeneralOut(*(p(g[k]) for k in ("offsets", "len", "npat", "pat_ids", "pat_val", "cp_slot", "ms_ok")))
    runtime._check(eng.lib, eng.lib.sdx_lines_exact(ctypes.byref(lb.c_lines), ctypes.byref(lb.c_out), p(sel), m,
                                                    ctypes.byref(go), eng.stream_ptr()))
    h = {k: v.cpu().numpy() for k, v in g.items()}
    return dict(rows=rows, status0=status0, status=lb.status[:n].cpu().numpy(), h=h, slot=lb.slot.cpu().numpy(),
                doff=lb.doff[:n].cpu().numpy(), dlen=lb.dlen[:n].cpu().numpy(),
                meta=lb.meta[: 32 * n].cpu().numpy().reshape(n, 32))


@pytest.mark.gpu
def test_status_and_tables_after_the_second_stage(proto, golden):
    """sdx_parse_lines then sdx_lines_exact on lines_float_golden: all 100 unsupported rows become
    SDX_LS_GENERAL with the reference's pattern table (values bitwise), D in the slot, the MS gates."""
    from pysignalduino_amd import runtime
    cases = golden("lines_float_golden.json.gz")
    lines = [c["line"] for c in cases]
    r = _exact_stage(proto._ensure(), lines)
    rows, h = r["rows"], r["h"]
    assert len(rows) == 100
    assert (r["status"][rows] == runtime.LS_GENERAL).all(), r["status"][rows]
    others = np.setdiff1d(np.arange(len(lines)), rows)
    assert (r["status"][others] == r["status0"][others]).all()
    for j, i in enumerate(rows):
        o = LO.parse_line(lines[i].encode("latin-1"))
        payload = o["payload"]
        kv = dict(LO._kv(payload))
        exp = _expected_table(payload)
        npat = int(h["npat"][j])
        base = [256 * j + 16 * z for z in range(npat)]
        ids = [bytes(h["pat_ids"][b + 1: b + 1 + int(h["pat_ids"][b])]).decode() for b in base]
        # message_synced.py:21-57: the string gates, then str(int(CP)) among the pattern ids
        digits = lambda k, req: (k in kv and kv[k].isdigit()) if req else (k not in kv or kv[k].isdigit())  # noqa: E731
        gates = digits(b"D", True) and digits(b"CP", True) and digits(b"SP", True) and digits(b"R", False)
        if gates:   # patterns are converted past the gates only
            assert ids == list(exp), (i, lines[i][:80], ids, list(exp))
            assert h["pat_val"][16 * j: 16 * j + npat].tobytes() == np.array(list(exp.values()), np.float64).tobytes(), \
                (i, lines[i][:80])
        cp_ok = gates and str(int(kv[b"CP"])) in exp
        assert int(h["ms_ok"][j]) == int(cp_ok), (i, lines[i][:80])
        if cp_ok:
            assert int(h["cp_slot"][j]) == list(exp).index(str(int(kv[b"CP"])))
        d = kv[b"D"]
        assert int(h["len"][j]) == len(d) == int(r["dlen"][i]) and int(h["offsets"][j]) == int(r["doff"][i])
        s0 = int(r["doff"][i])
        assert bytes(r["slot"][s0: s0 + len(d)]) == d
        ml = int(r["meta"][i][15])
        assert (None if ml == 255 else bytes(r["meta"][i][:ml])) == kv.get(b"R")


SPELL = ("zeros", "shifted", "tiny", "plus", "digits")


def _respell(v: bytes, how: str, rng) -> bytes:
    """An integer P value in another spelling: equal-valued (zeros, shifted, tiny -- sdx_parse_lines' float()
    reduces these to the integer, so they show that the old answers stay) or different-valued with 20 or more
    significant digits (plus: the value + 1e-25; digits: a 19-digit fraction), which only the exact
    conversion takes.  The expectation is the oracle's either way."""
    s = v.decode()
    sign, dig = ("-", s[1:]) if s[0] == "-" else ("", s)
    if how == "zeros":
        return (s + "." + "0" * 19).encode()
    if how == "shifted":
        return (sign + dig + "0" * 19 + "e-19").encode()
    if how == "tiny":
        k = int(rng.integers(25, 330))
        return (sign + "0." + "0" * k + dig + f"e+{k + len(dig)}").encode()
    if how == "digits":
        return (s + ".1234567890123456789").encode()
    return (s + "." + "0" * 24 + "1").encode()


def _synthetic_ms_lines():
    from pysignalduino_amd import bank as B, synth
    rng = np.random.default_rng(771)
    base, _ = synth.line_corpus(B.Bank().protocols, 300, seed=77, mix=(0, 1, 0), compress_frac=0.0)
    out = []
    for n, ln in enumerate(base):
        head, _, tail = ln.partition(b"\x03")
        parts = head[1:].split(b";")
        pk = [k for k, q in enumerate(parts) if q[:1] == b"P" and q[1:2].isdigit()]
        for t, k in enumerate(rng.choice(pk, size=min(len(pk), 1 + n % 2), replace=False)):
            key, _, v = parts[k].partition(b"=")   # the first one always leaves the one-operation float()
            parts[k] = key + b"=" + _respell(v, SPELL[3 + n // 2 % 2] if t == 0 else SPELL[int(rng.integers(0, 5))], rng)
        if n % 5 == 0:   # the multi-digit route and the exact floats in one line
            parts.insert(len(parts) - 1, b"P10=" + _respell(b"-1446", SPELL[n // 5 % 5], rng))
        out.append(b"\x02" + b";".join(parts) + b"\x03" + tail)
    return out


@pytest.mark.gpu
def test_synthetic_ms_lines_against_the_oracle_demodulator():
    from pysignalduino_amd.frontend import SignalParser
    lines = _synthetic_ms_lines()
    recs = [LO.parse_line(ln) for ln in lines]
    assert all(r["status"] == LO.UNSUPPORTED for r in recs)   # every line needs the second stage
    got = SignalParser().parse_lines(lines)
    ob = O.OracleBank()
    nres = 0
    for i, (ln, g) in enumerate(zip(lines, got)):
        assert not isinstance(g, BaseException), (i, ln[:120], g)
        payload = LO.extract_payload(ln)
        msg = {k.decode("latin-1"): v.decode("latin-1") for k, v in LO._kv(payload)}
        msg["data"] = msg["D"]
        try:
            exp = [(r["protocol_id"], r["payload"], r["meta"]["bit_length"], r["meta"]["clock"])
                   for r in O.demod(ob, msg, "MS")]
        except Exception:   # the reference's parser catches a demodulator exception: no results
            exp = []
        assert [(d.protocol_id, d.payload, d.metadata["bit_length"], d.metadata["clock"]) for d in g] == exp, (i, ln[:120])
        nres += bool(exp)
    assert nres >= 100, f"only {nres} of {len(lines)} lines yield results: the generator is too weak"


@pytest.mark.gpu
def test_what_stays_refused():
    """Lines outside the contract for another reason than their P# floats still come back as
    ContractError -- each also carries a 20-digit P value where its type allows -- and their
    neighbours in the same batch decode."""
    from pysignalduino_amd.frontend import SignalParser
    from pysignalduino_amd.packing import ContractError
    ok = (b"\x02MS;P2=246;P3=-249.1234567890123456789;P4=-1446;P6=-11601;D=262324242424232323232423242424232323"
          b"2423232324232423232423242324242424242323242426232424;CP=2;SP=6;R=59;\x03\n")
    pv = b"P3=-249.1234567890123456789;"
    d = b"D=2623242424242323232324232424242323232423232324232423232423242324242424242323242426232424;CP=2;SP=6;"
    pats17 = b"".join(b"P%d=%d;" % (k, 100 + k) for k in range(17))
    refused = [
        b"\x02MS;P2=246;" + pv + b"P4=-1446;P6=-11601;" + d + b"R=1234567890123456;\x03\n",       # a 16-digit R
        b"\x02MS;P2=246;" + pv + b"P4=-1446;P6=-11601;" + d + b"R=59;X=\xe9;\x03\n",              # a byte >= 0x80
        b"\x02MS;" + pats17 + pv.replace(b"P3=", b"P2=") + d + b"R=59;\x03\n",                    # 17 patterns
        b"\x02MS;P2=246;" + pv + b"P4=-1446;P6=-11601;P1234567890123456=5;" + d + b"R=59;\x03\n",  # a 16-digit id
        b"\x02MC;LL=-2883;LH=2982;SL=-1401;SH=1509;D=AF7EFF2E;C=99999999999;L=32;R=14;\x03\n",     # C beyond int32
    ]
    lines = []
    for r in refused:
        lines += [ok, r]
    lines.append(ok)
    got = SignalParser().parse_lines(lines)
    for i, g in enumerate(got):
        if i % 2:
            assert isinstance(g, ContractError), (i, lines[i][:80], g)
            assert "outside the device contract of the front end" in str(g) and f"line {i} " in str(g)
        else:
            assert [(m.protocol_id, m.payload, m.metadata["clock"]) for m in g] == [("23", "u23#785C452BE6C", 246.0)], i
    js = SignalParser().parse_lines_json(lines)
    for i, g in enumerate(js):
        assert isinstance(g, ContractError) == bool(i % 2), (i, g)
        if i % 2:
            assert f"line {i} " in str(g)


def test_unpack_helper_is_bitwise():
    assert FC.float_bits(-0.0) == 1 << 63 and struct.pack("<Q", FC.float_bits(float("-nan")))[7] & 0x80
