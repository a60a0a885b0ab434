"""repr(float) on the device (csrc/sdx_dtoa.h): sdx_format_floats / SDProtocols.repr_batch against
Python's repr() and json.dumps() byte for byte, and the MS clock of the publish path: k_json prints
abs(P[CP]) of any double as the reference's json.dumps does ("P3=377.25", "P3=246e19", ...)."""
import ctypes
import json
import math

import numpy as np
import pytest

import repr_corpus as RC
from oracle import json_oracle as J
from oracle import lines_oracle as LO
from oracle import sd_oracle as O


# ---------------------------------------------------------------------------------- CPU ------
def test_format_floats_rejects_bad_arguments_without_a_gpu():
    """sdx_format_floats validates before any HIP call (runs on the CPU)."""
    from pysignalduino_amd import build, runtime
    build.build()
    lib = runtime.load_library()
    buf = (ctypes.c_uint8 * 128)()
    a = ctypes.addressof(buf)
    a += -a % 8
    assert lib.sdx_format_floats(None, 1, 0, a + 32, None) == -1
    assert b"sdx_format_floats" in lib.sdx_last_error() and b"null" in lib.sdx_last_error()
    assert lib.sdx_format_floats(a, 1, 1, None, None) == -1
    assert b"null" in lib.sdx_last_error()
    assert lib.sdx_format_floats(None, 1, 0, None, None) == -1
    assert lib.sdx_format_floats(a, -1, 0, a + 32, None) == -1                      # never dereferenced
    assert b"sdx_format_floats" in lib.sdx_last_error()
    assert lib.sdx_format_floats(a, 0, 0, a + 32, None) == 0                        # n == 0
    assert lib.sdx_format_floats(None, 0, 0, None, None) == 0
    assert lib.sdx_format_floats(a + 1, 1, 0, a + 32, None) == -1
    assert b"aligned" in lib.sdx_last_error()
    assert lib.sdx_format_floats(a, 1, 0, a + 36, None) == -1
    assert b"aligned" in lib.sdx_last_error()
    assert "sdx_format_floats" in runtime.EXPORTED and lib.sdx_abi_version() == 14


# ---------------------------------------------------------------------------------- GPU ------
@pytest.fixture(scope="module")
def proto():
    from pysignalduino_amd.sd_protocols import SDProtocols
    return SDProtocols()


def _assert_texts(values, got, json_form):
    bad = [(RC.bits_of(v), g, RC.expected(v, json_form)) for v, g in zip(values, got) if g != RC.expected(v, json_form)]
    assert len(got) == len(values) and not bad, f"{len(bad)} of {len(values)} differ from Python: {bad[:5]}"


@pytest.mark.gpu
@pytest.mark.parametrize("json_form", [False, True])
def test_repr_batch_whole_corpus_and_round_trip(proto, json_form):
    c = RC.corpus()
    got = proto.repr_batch(c, json_form=json_form)
    _assert_texts(c, got, json_form)
    # and back through the device's float(): the same bits (json's NaN / Infinity are not float() syntax)
    fin = [k for k, v in enumerate(c) if math.isfinite(v) or not json_form]
    back = proto.float_batch([got[k] for k in fin])
    for k, b in zip(fin, back):
        assert not isinstance(b, ValueError), (c[k], got[k])
        if math.isnan(c[k]):
            assert math.isnan(b)
        else:
            assert RC.bits_of(b) == RC.bits_of(c[k]), (c[k], got[k], b)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_repr_batch_small_batches(proto, n):
    """a lone lane, a wave less one, a full wave, a wave plus one; taken where 17-digit values and
    subnormals sit, then from the corpus's front (zeros, inf, nan)."""
    cl = RC.classes()
    for src in (cl["digits17"][7:] + cl["random_subnormal"], RC.corpus()):
        part = src[:n]
        for json_form in (False, True):
            _assert_texts(part, proto.repr_batch(part, json_form=json_form), json_form)


@pytest.mark.gpu
def test_repr_batch_takes_floats_only(proto):
    from pysignalduino_amd.packing import ContractError
    assert proto.repr_batch([np.float64(0.1), -0.0]) == ["0.1", "-0.0"]
    for bad in (["1.5"], [1], [None]):
        with pytest.raises(ContractError):
            proto.repr_batch(bad)
    texts = proto._ensure().format_floats(np.array([0x7FF8000000000001, 0xFFF0000000000000], np.uint64), True)
    assert texts == [b"NaN", b"-Infinity"]


# ---- the MS clock on the publish path ---------------------------------------------------------
FRACTION = (b".25", b".1", b".0625", b".123456789")    # appended to the CP pattern's value
EXPONENT = (b"e19", b"e-7", b".7e14")                  # appended to every P value


def _respell(ln: bytes, suffix: bytes, every: bool) -> bytes:
    head, _, tail = ln.partition(b"\x03")
    parts = head[1:].split(b";")
    cp = b"P" + dict(p.split(b"=", 1) for p in parts if b"=" in p)[b"CP"]
    for k, q in enumerate(parts):
        key, _, v = q.partition(b"=")
        if key[:1] == b"P" and key[1:].isdigit() and (every or key == cp):
            parts[k] = key + b"=" + v + suffix
    return b"\x02" + b";".join(parts) + b"\x03" + tail


def _oracle(ob, ln: bytes):
    """[(protocol_id, payload, metadata)] of the oracle demodulator for one MS line"""
    payload = LO.extract_payload(ln)
    msg = {k.decode("latin-1"): v.decode("latin-1") for k, v in LO._kv(payload)}
    msg["data"] = msg["D"]
    try:
        return [(r["protocol_id"], r["payload"], r["meta"]) for r in O.demod(ob, msg, "MS")]
    except Exception:   # the reference's parser catches a demodulator exception: no results
        return []


@pytest.fixture(scope="module")
def clock_lines():
    """the 300 seeded MS lines and their 7 respellings, interleaved line by line (8 x 300 lines); per
    line the suffix and the oracle's results"""
    from pysignalduino_amd import bank as B, synth
    base, _ = synth.line_corpus(B.Bank().protocols, 300, seed=77, mix=(0, 1, 0), compress_frac=0.0)
    ob = O.OracleBank()
    lines, sufs = [], []
    for ln in base:
        lines.append(ln)
        sufs.append(b"")
        for s in FRACTION:
            lines.append(_respell(ln, s, False))
            sufs.append(s)
        for s in EXPONENT:
            lines.append(_respell(ln, s, True))
            sufs.append(s)
    exp = [_oracle(ob, ln) for ln in lines]
    return lines, sufs, exp


@pytest.fixture(scope="module")
def clock_texts(clock_lines):
    from pysignalduino_amd.frontend import SignalParser
    return SignalParser().parse_lines_json(clock_lines[0])


@pytest.mark.gpu
def test_ms_clock_of_any_double_in_parse_lines_json(clock_lines, clock_texts):
    from pysignalduino_amd.frontend import SignalParser
    lines, sufs, exp = clock_lines
    assert len(lines) == 8 * 300
    # every line stays on the device's fixed-layout path: the texts below are k_json's
    assert all(LO.parse_line(ln)["status"] == 0 for ln in lines)
    got = clock_texts
    exc = [(i, str(g)) for i, g in enumerate(got) if isinstance(g, BaseException)]
    assert not exc, f"{len(exc)} exceptions; first: {exc[:3]}"
    bad = [(i, lines[i][:100], g, J.published(e)) for i, (g, e) in enumerate(zip(got, exp)) if g != J.published(e)]
    assert not bad, f"{len(bad)} of {len(lines)} texts differ from the oracle's; first: {bad[:2]}"
    objs = SignalParser().parse_lines(lines)
    for i, (o, g) in enumerate(zip(objs, got)):
        assert not isinstance(o, BaseException), (i, o)
        assert g == J.published(o), (i, lines[i][:100])
    per = {s: sum(1 for t, g in zip(sufs, got) if t == s and g is not None) for s in FRACTION + EXPONENT}
    assert all(per[s] >= 150 for s in FRACTION) and all(per[s] >= 50 for s in EXPONENT), per
    # the clocks really are the ones the new branch prints
    clocks = [json.loads(g)["metadata"]["clock"] for t, g in zip(sufs, got) if t and g is not None]
    assert all(2 * c != math.floor(2 * c) or c >= 1e15 for c in clocks)


@pytest.mark.gpu
def test_ms_clock_of_any_double_in_the_json_stream(clock_lines, clock_texts):
    """the same lines through SignalParser.stream(output="json") in chunks of 257 lines"""
    from pysignalduino_amd.frontend import SignalParser
    lines = clock_lines[0]
    ls = SignalParser().stream(chunk_lines=257, chunk_bytes=257 * 256, output="json", lag=2)
    got = []
    for a in range(0, len(lines), 257):
        ls.submit(lines[a: a + 257])
        got += [t for r in ls.poll() for t in r.detach().texts()]
    got += [t for r in ls.drain() for t in r.detach().texts()]
    assert len(got) == len(lines)
    bad = [(i, lines[i][:100], g, e) for i, (g, e) in enumerate(zip(got, clock_texts)) if g != e]
    assert not bad, f"{len(bad)} texts differ from parse_lines_json's; first: {bad[:2]}"


@pytest.mark.gpu
def test_ms_clock_per_record_form(proto, clock_lines):
    """launch_json(first_only=False) over one MS launch of the ".25" lines: one text per result record,
    each with the exact clock"""
    from pysignalduino_amd import runtime
    from pysignalduino_amd.frontend import LineBatch, pack_lines
    lines, sufs, exp = clock_lines
    pick = [i for i, s in enumerate(sufs) if s == b".25"]
    sub, sub_exp = [lines[i] for i in pick], [exp[i] for i in pick]
    n = len(sub)
    eng = proto._ensure()
    data, offsets, bad = pack_lines(sub)
    assert not bad
    lb = LineBatch(eng, data, offsets)
    lb.launch()
    sels, cnt = lb.selections()
    assert int(cnt[runtime.SEL_MS_SHORT]) + int(cnt[runtime.SEL_MS_LONG]) == n
    out = eng.alloc_out(n, 16 * n + 1024, 256 * n + 65536, eng.pulses_work_bytes(n))
    pb = lb.pulse_batch()
    for sel, long_v in ((sels[runtime.SEL_MS_SHORT], False), (sels[runtime.SEL_MS_LONG], True)):
        if sel.numel():
            eng.launch_pulses(runtime.KIND_MS, pb, out, sel=sel, long_variant=long_v)
    jo = eng.alloc_json(out["rec_cap"], 400 * out["rec_cap"])
    eng.launch_json(runtime.KIND_MS, out, {"meta": lb.meta, "pat_val": lb.pat_val, "cp_slot": lb.cp_slot}, n, jo,
                    first_only=False)
    desc, rec, heap = eng.fetch(out)
    cur = jo["cursor"].cpu().numpy()
    assert not cur[1] and not out["cursor"].cpu().numpy()[2]
    offs, lens = jo["off"].cpu().numpy(), jo["len"].cpu().numpy()
    blob = jo["json"][: int(cur[0])].cpu().numpy().tobytes()
    nrec = len(rec)
    assert nrec == sum(len(e) for e in sub_exp) and nrec >= 150
    seen = 0
    for i, e in enumerate(sub_exp):
        b, k = int(desc[i]["rec_begin"]), int(desc[i]["n_rec"])
        assert k == len(e), (i, sub[i][:100])
        for j, (pid, payload, meta) in enumerate(e):
            g = b + j
            assert int(rec[g]["msg"]) == i
            text = blob[int(offs[g]): int(offs[g]) + int(lens[g])].decode("ascii")
            assert text == J.message_to_json(pid, payload, meta), (i, j, text)
            assert meta["clock"] % 1 == 0.25
            seen += 1
    assert seen == nrec


# Hand-made MS lines (line 9 of the seeded corpus, protocol 3.1) for the longest clock texts:
# every P value times 2.2250738585072014e-308, which leaves the one-operation float() and takes the
# second stage (a 23-character clock, 1.1948646620183671e-305); every P value times 1e22, on the
# device's fixed-layout path (5.37e+24); and the longest the fixed-layout path can meet, a 16-digit
# clock with a negative exponent (5.370000000000001e-05, 21 characters).
_D9 = b"D=05170317031703170317031717170317170317031703031703;CP=0;SP=5;R=136;\x03\n"
HAND = [
    b"\x02MS;P1=3.658021423385839e-305;P3=-3.5868190599136086e-305;P5=-3.672929418237837e-304;"
    b"P7=-1.1169870769706151e-305;P0=1.1948646620183671e-305;" + _D9,
    b"\x02MS;P1=1644e22;P3=-1612e22;P5=-16507e22;P7=-502e22;P0=537e22;" + _D9,
    b"\x02MS;P1=1644e-7;P3=-1612e-7;P5=-16507e-7;P7=-502e-7;P0=5370000000000001e-20;" + _D9,
    b"\x02MS;P1=1644e-7;P3=-1612e-7;P5=-16507e-7;P7=-502e-7;P0=-5370000000000001e-20;" + _D9,   # abs() of a negative clock
]


@pytest.mark.gpu
def test_longest_clock_texts_in_a_batch_of_65(clock_lines):
    from pysignalduino_amd.frontend import SignalParser
    base = [ln for ln, s in zip(clock_lines[0], clock_lines[1]) if s == b""]
    lines = base[:30] + HAND[:2] + base[30:60] + HAND[2:] + base[60:61]
    assert len(lines) == 65
    ob = O.OracleBank()
    exp = [J.published(_oracle(ob, ln)) for ln in lines]
    got = SignalParser().parse_lines_json(lines)
    for i, (g, e) in enumerate(zip(got, exp)):
        assert g == e, (i, lines[i][:120], g, e)
    hand = [exp[30], exp[31], exp[62], exp[63]]
    assert any(t is not None for t in hand)
    want = {json.loads(t)["metadata"]["clock"] for t in hand if t is not None}
    assert 1.1948646620183671e-305 in want and 5.37e+24 in want and 5.370000000000001e-05 in want
    assert len(repr(1.1948646620183671e-305)) == 23
