"""Inputs and references of tests/test_out_capacity.py (the output-capacity overflow contract), built on
the CPU alone so that tests/test_out_capacity_inputs.py can check their preconditions without a GPU.

A reference is a list with one entry per message: an int (the raise kind of include/sdx.h, the
reference raises on that message) or the ordered list of its results as (protocol, payload bytes,
bit length or None where the kernel does not report one).  `protocol` is the protocol id string, or
the method index in sdx_demod_mn's method mode."""
import functools
import os

import numpy as np

from oracle import c_oracle as CO
from oracle import mn_oracle as M
from oracle import sd_oracle as O
from pysignalduino_amd import bank as B
from pysignalduino_amd import packing, runtime, synth

RAISE_KIND = {v: k for k, v in runtime.RAISE_NAMES.items()}
MN_METHOD = "ConvLaCrosse"
HEAVY_N, HEAVY_SEED = 8192, 9601


def _threads():
    return max(1, min(16, len(os.sched_getaffinity(0))))


@functools.lru_cache(None)
def protocols():
    return B.load_protocols()


def _from_msgs(kind, msgs):
    pk = packing.PulsePacker(kind)
    for m in msgs:
        pk.add(m)
    return pk.batch()


def c_run(kind, pb):
    """The C oracle's raw outputs on a PulseBatch: (status, raise_kind, rec_begin, n_rec, rec, heap)."""
    CO.CBank()
    return CO.run(kind, CO.pack_batch(pb), _threads())


def c_reference(kind, pb):
    cb = CO.CBank()
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


# ---- the batches ---------------------------------------------------------------------------------
@functools.lru_cache(None)
def mu_short():
    """8 batch-order tiles of 64 MU messages, noise-free (result-heavy), raising messages present."""
    pb = synth.mu_corpus(protocols(), 512, seed=9611, noise_frac=0.0)
    return pb, c_reference("MU", pb)


@functools.lru_cache(None)
def mu_grouped():
    """Just above the grouping threshold: the launch sorts the messages before it tiles them."""
    pb = synth.mu_corpus(protocols(), runtime.GROUP_MIN + 64, seed=9612, noise_frac=0.0)
    return pb, c_reference("MU", pb)


@functools.lru_cache(None)
def mu_long():
    """64 messages of 257..1000 pulses: the long variant, 4 messages per tile."""
    msgs = []
    for npulse in (257, 300, 512, 1000):
        pb = synth.mu_corpus(protocols(), 16, seed=npulse, npulse=npulse)
        msgs += [pb.to_msg_dict(i) for i in range(pb.n)]
    pb = _from_msgs("MU", msgs)
    return pb, c_reference("MU", pb)


@functools.lru_cache(None)
def ms_classes():
    """600 MS messages, half of them stretched to 120..136 pulses around the 128-pulse class boundary, so
    that tiles of both length classes flush."""
    n = 600
    pb = synth.ms_corpus(protocols(), n, seed=9613)
    msgs = [pb.to_msg_dict(i) for i in range(pb.n)]
    rng = np.random.default_rng(n)
    for i in rng.choice(n, n // 2, replace=False):
        d = msgs[int(i)]["data"]
        L = int(rng.integers(120, 137))
        msgs[int(i)] = dict(msgs[int(i)], data=(d * (L // max(1, len(d)) + 1))[:L])
    pb = _from_msgs("MS", msgs)
    return pb, c_reference("MS", pb)


def mc_reference(frames):
    ob = O.OracleBank()
    out = []
    for h, c, L, t, v in frames:
        try:
            out.append([(r["protocol_id"], r["payload"].encode("latin-1"), None)
                        for r in O.demod_mc_fixed(ob, h, c, L, t, v)])
        except Exception as e:  # noqa: BLE001
            out.append(RAISE_KIND[type(e)])
    return out


@functools.lru_cache(None)
def mc_both():
    """1024 planted frames (accept paths of the MC methods) and 256 corpus frames padded past 64
    characters: both launches of sdx_demod_mc."""
    P = protocols()
    frames = list(synth.mc_planted_frames(P, 1024, seed=9614))
    rng = np.random.default_rng(9615)
    mb = synth.mc_corpus(P, 256, seed=9616)
    for i in range(mb.n):
        hx = mb.hex(i)
        lo = 65 - len(hx) if len(hx) < 65 else 1
        hx += "".join("0123456789ABCDEF"[int(v)] for v in rng.integers(0, 16, size=int(rng.integers(lo, 129 - len(hx)))))
        frames.append((hx, int(mb.clock[i]), int(mb.mcbitnum[i]), "Mc" if mb.mtype[i] else "MC", None))
    frames = tuple(frames)
    return frames, packing.mc_batch_from_frames(frames), mc_reference(frames)


@functools.lru_cache(None)
def mc_step():
    """The first 600 planted frames of <= 64 characters (three 256-frame blocks): the MC part of a
    fused step."""
    frames, _, ref = mc_both()
    rows = [i for i in range(1024) if len(frames[i][0]) <= 64][:600]
    frames = tuple(frames[i] for i in rows)
    return frames, packing.mc_batch_from_frames(frames), [ref[i] for i in rows]


@functools.lru_cache(None)
def mc_general():
    """64 frames of more than 128 characters.  Such frames rarely decode; the seed is one for which the
    oracle gives six results of equal size, so that no single frame needs more than half the capacity
    (most seeds give one or two results)."""
    frames = tuple(synth.general_mc_frames(protocols(), 64, seed=9630))
    return frames, packing.mc_batch_from_frames(frames), mc_reference(frames)


@functools.lru_cache(None)
def general_pulses(kind):
    """The general-path messages of synth.general_pulse_messages(n=200) that reach the device, their
    packer and the oracle's results."""
    from pysignalduino_amd.sd_protocols import SDProtocols
    msgs = synth.general_pulse_messages(protocols(), kind, 200, seed=9618 if kind == "MU" else 9619)
    _, _, rows, err = SDProtocols._pack_pulses(msgs, kind)
    msgs = [msgs[i] for i in rows if i not in err]
    gen = packing.GeneralPacker(kind)
    for m in msgs:
        gen.add(m)
    ob = O.OracleBank()
    ref = []
    for m in msgs:
        try:
            ref.append([(r["protocol_id"], r["payload"].encode("latin-1"), int(r["meta"]["bit_length"]))
                        for r in O.demod(ob, dict(m), kind)])
        except Exception as e:  # noqa: BLE001
            ref.append(RAISE_KIND[type(e)])
    return msgs, gen, ref


@functools.lru_cache(None)
def mn_both():
    """1024 MN frames with the parser-mode reference (every protocol eligible: rfmode None) and the
    method-mode reference of MN_METHOD."""
    frames = tuple(synth.mn_frames(1024, seed=9620))
    ob = O.OracleBank()
    parser = [[(pid, p.encode("latin-1"), None) for pid, p, _ in M.mn_parse(ob, f[0], None, None, None)] for f in frames]
    k = B.MN_METHODS[MN_METHOD]
    method = [[(k, r["payload"].encode("latin-1"), None)
               for r in M.call_method(MN_METHOD, {"data": f[0], "protocol_id": "100"})] for f in frames]
    return frames, parser, method


@functools.lru_cache(None)
def heavy(min_rec):
    """The messages of mu_corpus(8192, noise-free) with >= min_rec results in the C oracle, as firmware
    lines: (lines, the sub-batch, the oracle's record count per line)."""
    pb = synth.mu_corpus(protocols(), HEAVY_N, seed=HEAVY_SEED, noise_frac=0.0)
    st, _, _, nr, _, _ = c_run("MU", pb)
    idx = np.nonzero((st == 0) & (nr >= min_rec))[0]
    sub = pb.subset(idx)
    lines = [synth.frame(synth.pulse_payload(sub, i)) for i in range(sub.n)]
    return lines, sub, nr[idx].astype(np.int64)


def heavy_texts(lines):
    """J.published of the reference's first result per line (the oracle's parse + demodulation)."""
    from oracle import json_oracle as J
    from oracle import lines_oracle as LO
    ob = O.OracleBank()
    out = []
    for ln in lines:
        r = LO.parse_line(ln)
        assert r["status"] == LO.OK and r["kind"] == LO.MU
        res = O.demod(ob, dict(r["msg"]), "MU")
        out.append(J.published([(res[0]["protocol_id"], res[0]["payload"], res[0]["meta"])]) if res else None)
    return out


# ---- reservation units ---------------------------------------------------------------------------
def demand(ref):
    """Per message (records, payload bytes) of a reference."""
    nrec = np.array([len(e) if isinstance(e, list) else 0 for e in ref], np.int64)
    nbytes = np.array([sum(len(r[1]) for r in e) if isinstance(e, list) else 0 for e in ref], np.int64)
    return nrec, nbytes


def largest_unit(ref, unit, any_order=False):
    """(largest unit's records, its payload bytes, total records, total bytes): the units are `unit`
    consecutive messages in batch order, or -- any_order, for a launch that sorts its messages first --
    the `unit` heaviest messages, a bound for every order."""
    nrec, nbytes = demand(ref)
    if any_order:
        r, b = int(np.sort(nrec)[-unit:].sum()), int(np.sort(nbytes)[-unit:].sum())
    else:
        cuts = np.arange(0, len(nrec), unit)
        r, b = int(np.add.reduceat(nrec, cuts).max()), int(np.add.reduceat(nbytes, cuts).max())
    return r, b, int(nrec.sum()), int(nbytes.sum())


# a unit's heap reservation is rounded up to 16-byte pieces (twice for a tile with a spill region)
UNIT_PAD = 32


def half_fits(ref, unit, any_order=False):
    """The largest reservation unit needs at most half the batch's records and half its payload bytes,
    so a launch with half the capacity still places at least the first unit that reserves."""
    r, b, tr, tb = largest_unit(ref, unit, any_order)
    return tr > 0 and 2 * r <= tr and 2 * (b + UNIT_PAD) <= tb
