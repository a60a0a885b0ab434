"""Inputs and references of tests/test_mu_bin_payload.py, built on the CPU alone (the C oracle is the
reference), so that tests/test_mu_result_path_inputs.py can check their preconditions without a GPU.

A reference is a list with one entry per message: an int (the raise kind, the reference raises on that
message) or the ordered list of its results as (protocol id, payload bytes, bit length)."""
import copy
import functools
import os

import numpy as np

from oracle import c_oracle as CO
from pysignalduino_amd import bank as B
from pysignalduino_amd import packing, runtime

# ---- binary-dispatch payloads ----------------------------------------------------------------------
# protocol 82 (Fernotron: dispatchBin, a float symbol, paddingbits 1) and copies of it under new ids
BIN_COPIES = {
    "82.4": {"paddingbits": "4"},
    "82.8": {"paddingbits": "8"},
    "82.9": {"postamble": "#Z9"},                                  # longer than the descriptor's inline two
    "82.7": {"modulematch": "^P82#[01]{8}[01F]{92}"},              # any modulematch walks a binary payload bytewise
    "82.5": {"paddingbits": "8", "postamble": "xyz", "modulematch": "^P82#[01F]*xyz$"},   # ... through the postamble
}
BIN_IDS = ("82",) + tuple(BIN_COPIES)
FRAME_BITS = (100, 103, 104, 105, 111, 112, 113, 120, 127, 128)
FLOAT_AT = (0, 7, 8, 63, 64, -1)   # -1: the frame's last bit
BATCHES = (1, 65, 129)
UNIT = {"1": "01", "0": "23", "F": "04"}   # one [1, -2], zero [2, -1], float [1, -8] at clockabs 400
PHEAP_MU = 10240                            # TileLds<4, 64, 1>: the MU lane tile's LDS heap (sdx_tile.h)


def _threads():
    return max(1, min(16, len(os.sched_getaffinity(0))))


@functools.lru_cache(None)
def bin_protocols():
    P = copy.deepcopy(B.load_protocols())
    for pid, edit in BIN_COPIES.items():
        P[pid] = dict(copy.deepcopy(P["82"]), id=pid, **edit)
    return P


def fernotron_msg(bits):
    """One MU message whose data is a separator pulse and the frame `bits` (a string over 0, 1, F); a frame
    of 128 bits fills the 256 pulses by itself."""
    d = ("5" if len(bits) < 128 else "") + "".join(UNIT[b] for b in bits)
    assert len(d) <= 256
    return {"MU": "", "P0": "400", "P1": "-800", "P2": "800", "P3": "-400", "P4": "-3200", "P5": "-12000",
            "D": d, "data": d, "CP": "0", "R": "30"}


def _from_msgs(msgs):
    pk = packing.PulsePacker("MU")
    for m in msgs:
        pk.add(m)
    return pk.batch()


def reference(kind, pb, protocols=None):
    """The C oracle's results on a PulseBatch, with the bank `protocols` (default: the shipped one)."""
    cb = CO.CBank(protocols)
    st, rk, rb, nr, rec, heap = CO.run(kind, CO.pack_batch(pb), _threads())
    hb = heap.tobytes()
    out = []
    for i in range(pb.n):
        if st[i]:
            out.append(int(rk[i]))
            continue
        rs = rec[int(rb[i]): int(rb[i]) + int(nr[i])]
        out.append([(cb.pids[int(r["proto"])], hb[int(r["off"]): int(r["off"]) + int(r["len"])], int(r["bitlen"]))
                    for r in rs])
    return out


@functools.lru_cache(None)
def bin_frames():
    """129 messages: every frame length of FRAME_BITS without a float symbol and with one at each position of
    FLOAT_AT (70 messages, the plain ones first), then random frames of 100..128 bits, some with floats.
    Returns (frames, batch, reference); the batches of the test are its first 1, 65 and 129 messages."""
    rng = np.random.default_rng(8201)
    frames = []
    for at in (None,) + FLOAT_AT:
        for nb in FRAME_BITS:
            bits = [str(int(b)) for b in rng.integers(0, 2, size=nb)]
            if at is not None:
                bits[at] = "F"
            frames.append("".join(bits))
    while len(frames) < max(BATCHES):
        nb = int(rng.integers(100, 129))
        bits = [str(int(b)) for b in rng.integers(0, 2, size=nb)]
        for at in rng.integers(0, nb, size=int(rng.integers(0, 4))):
            bits[int(at)] = "F"
        frames.append("".join(bits))
    pb = _from_msgs([fernotron_msg(f) for f in frames])
    return tuple(frames), pb, reference("MU", pb, bin_protocols())


@functools.lru_cache(None)
def bin_heavy():
    """64 messages (one tile), each a 112-bit frame that all six binary protocols decode: more payload than
    the tile's LDS heap holds, so most binary payloads go through the spilled writer."""
    rng = np.random.default_rng(8202)
    frames = []
    for i in range(64):
        bits = [str(int(b)) for b in rng.integers(0, 2, size=112)]
        if i % 2:
            bits[int(rng.integers(8, 112))] = "F"
        frames.append("".join(bits))
    pb = _from_msgs([fernotron_msg(f) for f in frames])
    return tuple(frames), pb, reference("MU", pb, bin_protocols())


def bin_results(entry):
    """The binary-dispatch results of one reference entry."""
    return [r for r in entry if r[0] in BIN_IDS] if isinstance(entry, list) else []


# ---- comparison ------------------------------------------------------------------------------------
def compare(desc, rec, heap, ref, pids):
    """Device outputs against a reference: status, raise kind, record order, protocol, payload, bit length,
    the record's message, and rec_begin / n_rec contiguity (the messages' ranges tile [0, records)).
    Returns the record count."""
    OK, RAISED = runtime.ST_OK, runtime.ST_RAISED
    hb = heap.tobytes()
    ranges = []
    for i, e in enumerate(ref):
        d = desc[i]
        if not isinstance(e, list):
            assert d["status"] == RAISED and d["raise_kind"] == e, (i, int(d["status"]), int(d["raise_kind"]), e)
            continue
        assert d["status"] == OK, (i, int(d["status"]))
        b, n = int(d["rec_begin"]), int(d["n_rec"])
        assert n == len(e), (i, n, len(e))
        if n:
            ranges.append((b, b + n))
        for q, x in zip(range(b, b + n), e):
            r = rec[q]
            off, ln = int(r["payload_off"]), int(r["payload_len"])
            got = (str(pids[int(r["proto"])]), hb[off: off + ln], int(r["bit_length"]))
            assert got == x and int(r["msg"]) == i, (i, q, got, x, int(r["msg"]))
    ranges.sort()
    total = sum(b - a for a, b in ranges)
    assert all(a[1] <= b[0] for a, b in zip(ranges, ranges[1:])), "record ranges of two messages overlap"
    assert total == len(rec), (total, len(rec))
    return total
