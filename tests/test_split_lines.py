"""Byte-stream input: sdx_split_lines (csrc/sdx_split.hip) and SignalParser.parse_bytes / parse_bytes_json.

The reference splits a transport's bytes with StreamReader.readline() (signalduino/transport.py:113-123):
every '\\n' ends a line, the rest is a line only at EOF.  The CPU tests pin the exports and the argument
checks; the GPU tests compare the device's offsets with numpy's on buffers whose sizes and newline
positions sit on every boundary of the kernels (a lane's 16 bytes, a wave's 1024, a round's 4096, a
workgroup's 16384), and the byte entries with the line entries on the reference-recorded lines."""
import ctypes

import numpy as np
import pytest

from pysignalduino_amd import frontend, runtime

LANE, WAVE, ROUND, SPAN = 16, 1024, 4096, 16384     # csrc/sdx_split.hip: LANE_BYTES, 64 lanes, ROUND_BYTES, SPAN


def test_split_entries_are_exported():
    from pysignalduino_amd import build
    build.build()
    lib = runtime.load_library()
    for name in ("sdx_split_lines", "sdx_split_work_bytes", "sdx_host_count_byte"):
        assert name in runtime.EXPORTED and hasattr(lib, name), name
    assert lib.sdx_abi_version() == 14
    # one int32 per workgroup span, at least one
    assert [lib.sdx_split_work_bytes(n) for n in (0, 1, SPAN, SPAN + 1, 3 * SPAN + 5)] == [4, 4, 4, 8, 16]


def test_host_count_byte_matches_numpy():
    """The host's newline count (what submit_bytes sizes a chunk with): every length around the loop's
    64-byte step and its 255-step blocks, dense and sparse, at odd start addresses."""
    lib = runtime.load_library()
    rng = np.random.default_rng(4)
    blk = 255 * 64
    for n in [0, 1, 63, 64, 65, 127, 128, blk - 1, blk, blk + 1, blk + 64, 2 * blk + 63, 5 * blk + 17]:
        for dense in (False, True):
            a = np.full(n + 3, 10, np.uint8) if dense else rng.integers(0, 256, n + 3).astype(np.uint8)
            for start in (0, 3):
                got = lib.sdx_host_count_byte(a.ctypes.data + start, n, 10)
                assert got == int(np.count_nonzero(a[start: start + n] == 10)), (n, dense, start)


def test_split_rejects_bad_arguments_without_a_gpu():
    """Validation comes before any HIP call (as sdx_demod_step): null pointers, nbytes outside [0, 2^31)
    and a negative cap return SDX_EINVAL with a text; the pointers given are never dereferenced."""
    lib = runtime.load_library()
    p = ctypes.c_void_p(4096)     # aligned, never read

    def call(b=p, nbytes=64, o=p, cap=8, c=p, s=p):
        rc = lib.sdx_split_lines(b, nbytes, 0, o, cap, c, s, None)
        return rc, lib.sdx_last_error()

    for kw in ({"b": None}, {"o": None}, {"c": None}, {"s": None}, {"nbytes": -1}, {"nbytes": 2 ** 31}, {"cap": -1},
               {"b": ctypes.c_void_p(4097)}):
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith(b"sdx_split_lines") and len(msg) > 20, (kw, rc, msg)


def test_lines_of():
    assert frontend.lines_of(b"a\nb\n") == ([b"a", b"b"], b"")
    assert frontend.lines_of(b"a\n\nb") == ([b"a", b"", b"b"], b"")
    assert frontend.lines_of(b"a\n\nb", final=False) == ([b"a", b""], b"b")
    assert frontend.lines_of(b"") == ([], b"") and frontend.lines_of(b"\n") == ([b""], b"")


# ---- GPU -------------------------------------------------------------------------------------------------
def _expected(buf: np.ndarray, final: bool):
    """(offsets int64[n + 1], n, tail start) by numpy."""
    ends = np.flatnonzero(buf == 10).astype(np.int64) + 1
    nb = len(buf)
    last = int(ends[-1]) if len(ends) else 0
    if final and last < nb:
        ends, last = np.append(ends, nb), nb
    return np.concatenate([[0], ends]).astype(np.int64), len(ends), last


def _contents(nb: int, rng):
    """name -> buffer of nb bytes."""
    out = {"none": rng.integers(11, 256, nb).astype(np.uint8), "all": np.full(nb, 10, np.uint8)}
    edges = rng.integers(11, 128, nb).astype(np.uint8)
    for unit in (LANE, WAVE, ROUND, SPAN):      # the last byte of each unit and the first of the next
        edges[unit - 1::unit] = 10
        edges[unit::unit] = 10
    out["edges"] = edges
    rnd = rng.integers(0, 256, nb).astype(np.uint8)      # bytes >= 0x80 present, ~1 newline in 40
    rnd[rng.random(nb) < 0.025] = 10
    out["random"] = rnd
    if nb:
        a, b = rnd.copy(), rnd.copy()
        a[-1], b[-1] = 10, 0x8A     # no tail / a tail ending in a byte that differs from '\n' in bit 7 only
        out["random-notail"], out["random-tail"] = a, b
    return out


SIZES = [0, 1, LANE - 1, LANE, LANE + 1, WAVE - 1, WAVE, WAVE + 1, ROUND - 1, ROUND, ROUND + 1,
         SPAN - 1, SPAN, SPAN + 1, 3 * SPAN + 5]


@pytest.fixture(scope="module")
def parser():
    from pysignalduino_amd.sd_protocols import SDProtocols
    return frontend.SignalParser(SDProtocols(mc_mode="fixed"))


@pytest.mark.gpu
def test_gpu_split_lines_matches_numpy(parser):
    import torch
    eng = parser.protocols._ensure()
    d = eng.dev
    top = max(SIZES)
    bytes_dev = torch.empty(top + 16, dtype=torch.uint8, device=d)
    offsets_dev = torch.empty(top + 3, dtype=torch.int64, device=d)
    count = torch.empty(2, dtype=torch.int64, device=d)
    scratch = torch.empty(eng.split_work_ints(top), dtype=torch.int32, device=d)
    rng = np.random.default_rng(20)
    cases = capped = 0
    for nb in SIZES:
        for name, buf in _contents(nb, rng).items():
            host = np.concatenate([buf, np.full(16, 10, np.uint8)])     # the pad holds newlines: never counted
            bytes_dev[: nb + 16] = torch.from_numpy(host)
            for final in (False, True):
                exp_off, n, tail = _expected(buf, final)
                for cap in sorted({n + 1, n, n // 2, 0}):
                    offsets_dev.fill_(-7)
                    count.fill_(-7)
                    eng.split_lines(bytes_dev, nb, final, offsets_dev, cap, count, scratch)
                    got_cnt = count.cpu().numpy()
                    got = offsets_dev[: cap + 2].cpu().numpy()
                    tag = (nb, name, final, cap)
                    assert got_cnt.tolist() == [n, tail], (tag, got_cnt, n, tail)
                    k = min(n, cap)
                    assert np.array_equal(got[: k + 1], exp_off[: k + 1]), tag
                    assert (got[k + 1:] == -7).all(), (tag, got[k + 1:])    # nothing past offsets[min(n, cap)]
                    cases += 1
                    capped += cap < n
    assert cases > 300 and capped > 50, (cases, capped)


def _golden_bytes(golden, sep: bytes, limit=None) -> bytes:
    lines = [c["line"].encode("latin-1") for c in golden("lines_golden.json.gz")][:limit]
    return sep.join(lines) + sep


def _same(exp, got):
    assert len(exp) == len(got)
    for i, (e, g) in enumerate(zip(exp, got)):
        if isinstance(e, Exception):
            assert type(g) is type(e), (i, e, g)
        else:
            assert e == g, (i, e, g)


@pytest.mark.gpu
@pytest.mark.parametrize("sep", [b"\n", b"\r\n"])
def test_gpu_parse_bytes_json_equals_parse_lines_json(parser, golden, sep):
    """The same product path after the split, so every line's text (or None, or ContractError) is equal."""
    data = _golden_bytes(golden, sep)
    lines, tail = frontend.lines_of(data)
    assert len(lines) > 3000 and tail == b""
    exp = parser.parse_lines_json(lines)
    _same(exp, parser.parse_bytes_json(data))
    assert sum(isinstance(e, str) for e in exp) > 500
    # an unterminated tail: the last line at EOF, handed back otherwise
    cut = data[: -len(sep) - 5]
    _same(parser.parse_lines_json(frontend.lines_of(cut)[0]), parser.parse_bytes_json(cut))
    head, rest = frontend.lines_of(cut, final=False)
    got, got_tail = parser.parse_bytes_json(cut, final=False)
    assert got_tail == rest and len(rest) > 0
    _same(exp[: len(head)], got)
    assert parser.parse_bytes_json(b"") == [] and parser.parse_bytes_json(b"MU;", final=False) == ([], b"MU;")


@pytest.mark.gpu
def test_gpu_parse_bytes_equals_parse_lines(parser, golden):
    data = _golden_bytes(golden, b"\n", limit=400)
    lines, _ = frontend.lines_of(data)
    key = lambda r: r if isinstance(r, Exception) else [  # noqa: E731  (RawFrame.timestamp is the wall clock)
        (m.protocol_id, m.payload, m.metadata, m.raw.line, m.raw.rssi, m.raw.freq_afc, m.raw.message_type) for m in r]
    exp, got = parser.parse_lines(lines), parser.parse_bytes(data)
    _same([key(e) for e in exp], [key(g) for g in got])
    assert sum(bool(e) and not isinstance(e, Exception) for e in exp) > 50
