"""Id-pair presence from the staging registers (pulses_tile, NW <= 4: L.pairs built from each lane's
16 characters and the one after them) against the plain-C oracle.  The inputs are small hand-built
batches in which one 2-pulse key decides a message's result and sits on a lane, dword or 64-bit word
boundary, at the message's end, next to characters that are no ids, or would exist only if a
neighbouring message's characters were read.  Every case runs through sdx_demod_pulses (MU; MS under
SDX_MS_TILE=64 and =128) and sdx_demod_step, in batches of 1, 65 and 129 messages."""
import functools

import numpy as np
import pytest

from test_full_size import _compare_with_c_oracle

pytestmark = pytest.mark.gpu

ROUTES = ("pulses", "step")
TILES = (128, 64)
SIZES = (1, 65, 129)
FE, NONDIGIT = "٣", "x"     # isdigit() but no id (0xFE in the batch) / no digit at all

# (protocol, p, n, pad, m): a message of n pulses = [pad pulse] + head + filler units, the other unit
# once at (p, p + 1); m > 0: the head + m filler units repeated in front (MS frames are short).
# Chosen on the C oracle (_deciding asserts it): the message has a result, and another result list
# when the unit at p is a filler unit too.  p = 15 | 31 | 47: lane boundaries, 63 | 127 | 191: bitmap
# words, 126: inside the last lane of a 128-pulse row, n = p + 2: the pair is the message's last two
# characters (254: the last two of a full 256-pulse row).
MU_CASES = [("31", 15, 17, 1, 0), ("31", 15, 24, 1, 0), ("40", 15, 55, 1, 0), ("40", 31, 33, 1, 0), ("86", 31, 40, 1, 0),
            ("75", 31, 71, 1, 0), ("128", 47, 49, 1, 0), ("94", 47, 56, 1, 0), ("8", 47, 87, 1, 0), ("61", 63, 65, 1, 0),
            ("135", 63, 72, 1, 0), ("64", 63, 103, 1, 0), ("9", 127, 129, 1, 0), ("54", 127, 136, 1, 0),
            ("42", 127, 167, 1, 0), ("94", 191, 193, 1, 0), ("9", 191, 200, 1, 0), ("82", 191, 231, 1, 0),
            ("40", 254, 256, 0, 0), ("31", 254, 256, 0, 0)]
MS_SHORT_CASES = [("15", 15, 24, 1, 0), ("13", 15, 55, 1, 0), ("15", 31, 33, 1, 0), ("15", 31, 40, 1, 0), ("90", 31, 71, 1, 0),
                  ("118.1", 47, 49, 0, 0), ("25", 47, 56, 1, 0), ("33", 47, 87, 1, 0), ("20", 63, 65, 1, 0),
                  ("93", 63, 72, 1, 0), ("25", 63, 103, 1, 0), ("65", 126, 128, 0, 0)]
MS_LONG_CASES = [("65", 127, 129, 1, 0), ("88", 127, 136, 1, 0), ("87", 127, 167, 1, 0), ("68", 191, 193, 1, 20),
                 ("13", 191, 200, 1, 24), ("13.2", 191, 231, 1, 24), ("68", 254, 256, 0, 20), ("13", 254, 256, 0, 24)]
CASES = {"MU": ("MU", MU_CASES), "MS128": ("MS", MS_SHORT_CASES), "MS256": ("MS", MS_LONG_CASES)}


@functools.lru_cache(maxsize=None)
def _env():
    from oracle import c_oracle as CO
    from pysignalduino_amd import bank as B, runtime
    bk = B.Bank()
    return bk, runtime.Engine(bk, 0), CO.CBank()


def _oracle(kind, msgs):
    """Per message the C oracle's result list [(pid, payload, bit_length)] or the exception class."""
    from oracle import c_oracle as CO
    return CO.results(_env()[2], kind, CO.pack_pulses(msgs))


def _craft(kind, pid, p, n, pad, m):
    """(message, the same with a filler unit at p, the deciding key as id characters)."""
    pr = _env()[0].protocols[pid]
    head = [float(x) for x in (pr["sync"] if kind == "MS" else pr.get("start") or [])]
    fill, odd = [float(x) for x in pr["one"]], [float(x) for x in pr["zero"]]
    vals = []
    for v in head + fill + odd:
        if v not in vals:
            vals.append(v)
    ix = lambda seq: [vals.index(v) for v in seq]   # noqa: E731
    seq = ix(fill)[1:] if pad else []
    seq += ix(head)
    while m and len(seq) + 4 * m + len(head) <= p and (p - len(seq) - 2 * m - len(head)) % 2 == 0:
        seq += ix(fill) * m + ix(head)
    assert p >= len(seq) and (p - len(seq)) % 2 == 0, (pid, p)
    seq += ix(fill) * ((p - len(seq)) // 2)
    alt = seq + ix(fill)
    seq = seq + ix(odd)
    tail = ix(fill) * ((n - p) // 2)
    seq, alt = (seq + tail)[:n], (alt + tail)[:n]
    clock = float(pr["clockabs"])
    d = {kind: "", "R": "30"}
    for s, v in enumerate(vals):
        d["P%d" % s] = str(int(round(v * clock)))
    d["CP"] = str(min(range(len(vals)), key=lambda s: abs(abs(vals[s]) - 1.0)))
    if kind == "MS":
        d["SP"] = str(vals.index(max(head, key=abs)))
    key = "".join(map(str, ix(odd)))
    msg, flat = dict(d, data="".join(map(str, seq))), dict(d, data="".join(map(str, alt)))
    assert len(msg["data"]) == n and msg["data"][p:p + 2] == key and msg["data"].count(key) == 1 and key not in flat["data"]
    return msg, flat, key


@functools.lru_cache(maxsize=None)
def _deciding(group):
    """The crafted messages of a group, each checked on the CPU: the oracle returns a result for it,
    and another result list without the unit at p."""
    kind, cases = CASES[group]
    crafted = [_craft(kind, *c) for c in cases]
    with_key, without = _oracle(kind, [c[0] for c in crafted]), _oracle(kind, [c[1] for c in crafted])
    for c, a, b in zip(cases, with_key, without):
        assert isinstance(a, list) and len(a) > 0 and a != b, (group, c, a, b)
    return [c[0] for c in crafted]


def _batch(kind, msgs):
    from pysignalduino_amd import packing
    pk = packing.PulsePacker(kind)
    for m in msgs:
        pk.add(m)
    return pk.batch()


def _check(kind, route, msgs):
    """One launch of msgs in their order through the route; every message equals the C oracle's."""
    import torch
    from pysignalduino_amd import runtime
    bk, eng, _ = _env()
    batch = _batch(kind, msgs)
    n = batch.n
    bd = eng.to_device_pulses(batch)
    out = eng.alloc_out(n, 40 * n + 4096, 1024 * n + 65536, eng.pulses_work_bytes(n))
    if route == "pulses":
        eng.launch_pulses(runtime.KIND_MU if kind == "MU" else runtime.KIND_MS, bd, out, group=False)
    elif kind == "MU":
        eng.launch_step(mu=(bd, out, None, None))
    else:
        eng.launch_step(ms=(bd, out, None, None))
    torch.cuda.synchronize()
    return _compare_with_c_oracle(kind, bk, batch, *eng.fetch(out))


def _rotations(msgs, n):
    """Batches of n messages, the crafted ones in turn: over the rotations every one of them is the
    batch's last message (alone, the only one of a second tile, of a third), and for n = 129 stands
    in both halves of a 128-message tile."""
    return [[msgs[(s + i) % len(msgs)] for i in range(n)] for s in range(len(msgs))]


def _params():
    return [pytest.param(g, tm, id=f"{g}-tile{tm}") for g in CASES for tm in (TILES if g != "MU" else TILES[:1])]


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("group,tm", _params())
def test_deciding_pair_on_a_boundary(monkeypatch, group, tm, n, route):
    """A 2-pulse key that occurs once, across positions 15|16 ... 254|255 or as the last two
    characters: the message loses its result if that pair's bit is missed."""
    monkeypatch.setenv("SDX_MS_TILE", str(tm))
    kind = CASES[group][0]
    msgs = _deciding(group)
    if group == "MS128":
        assert all(len(m["data"]) <= 128 for m in msgs)     # so that tm = 128 runs the 128-message tile
    for b in _rotations(msgs, n):
        assert _check(kind, route, b) >= n


@functools.lru_cache(maxsize=None)
def _adjacent(group):
    """Messages that hold every key of their protocol but one, "ab": each ends with a and begins with b,
    so the pair exists only across a message boundary in the batch's data.  Checked on the CPU: with b
    appended the oracle's result list changes, so a pair bit taken from the neighbour would show.  The
    lengths step through all alignments."""
    kind, cases = CASES[group]
    out = []
    for i, c in enumerate(cases):
        pid, p, n, pad, m = c
        _, flat, key = _craft(kind, pid, p, n, pad, m)
        # 4 lengths per case, so that the next message's offset takes all of off & 3, and a whole number
        # of lanes: the character after the last lane's 16 is then the next message's first
        for extra in sorted({0, 1, 2, 3, -len(flat["data"]) % 16}):
            if len(flat["data"]) + extra > (128 if group == "MS128" else 256):
                continue
            filler = flat["data"][-2:] * 8
            data = key[1] + flat["data"][1:] + filler[:extra]
            data = data[:-1] + key[0]
            if key in data:
                continue
            a, b = _oracle(kind, [dict(flat, data=data), dict(flat, data=data + key[1])])
            if a != b and isinstance(b, list) and len(b) > 0:
                out.append((dict(flat, data=data), key))
    return out


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("group,tm", _params())
def test_no_pair_from_the_next_message(monkeypatch, group, tm, route):
    """Message m ends with id a, message m + 1 begins with id b, "ab" being the one key message m lacks:
    the character after a lane's 16 may lie in a loaded dword and still belong to the next message."""
    monkeypatch.setenv("SDX_MS_TILE", str(tm))
    kind = CASES[group][0]
    msgs, keys = [a[0] for a in _adjacent(group)], [a[1] for a in _adjacent(group)]
    assert len(msgs) >= 8, len(msgs)
    # neighbours in the list are mostly of one protocol: the boundary then spells the key the first one lacks
    assert sum(a["data"][-1] + b["data"][0] == k for a, b, k in zip(msgs, msgs[1:], keys)) >= len(msgs) // 2
    batch = _batch(kind, msgs)      # the list's order: the first rotation of n = 129 below
    assert len(msgs) <= SIZES[-1]
    ends = batch.offsets[1:-1]
    assert set((ends & 3).tolist()) == {0, 1, 2, 3}              # the boundary at every byte of a dword
    assert set((batch.offsets[:-1] & 3).tolist()) == {0, 1, 2, 3}  # and every alignment of a message's rows
    lens = np.diff(batch.offsets)
    cap = 128 if group == "MS128" else 256
    assert ((lens % 16 == 0) & (lens < cap)).any()               # a lane's carried character is the neighbour's
    for n in SIZES:
        for b in _rotations(msgs, n)[:: max(1, len(msgs) // 8)]:
            _check(kind, route, b)


def _neighbours(group):
    """The crafted messages with 0xFE or a non-digit directly before the deciding pair, directly after
    it, and between its two characters (then there is no pair)."""
    out = []
    kind, cases = CASES[group]
    for c in cases:
        msg, _, key = _craft(kind, *c)
        d, p = msg["data"], c[1]
        for x in (FE, NONDIGIT):
            if p > 0:
                out.append(dict(msg, data=d[:p - 1] + x + d[p:]))
            if p + 2 < len(d):
                out.append(dict(msg, data=d[:p + 2] + x + d[p + 3:]))
            out.append(dict(msg, data=d[:p + 1] + x + d[p + 2:]))                 # in place of the second character
            out.append(dict(msg, data=(d[:p + 1] + x + d[p + 1:])[:len(d)]))      # between the two
    return out


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("group,tm", _params())
def test_non_digit_neighbours(monkeypatch, group, tm, route):
    """0xFE (isdigit() in packing.py, no id) and a non-digit character around and inside the pair."""
    monkeypatch.setenv("SDX_MS_TILE", str(tm))
    kind = CASES[group][0]
    msgs = _neighbours(group)
    got = _oracle(kind, msgs)
    assert any(isinstance(r, list) and len(r) > 0 for r in got)    # some of them still decode
    for n in SIZES:
        for b in _rotations(msgs, n)[:: max(1, len(msgs) // 8)]:
            _check(kind, route, b)
