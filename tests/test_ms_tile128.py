"""The 128-message MS tile (pulses_tile<MS, 2, 128>, ms_tile_by_class with tm = 128) and the
64-message tiles it replaces on large batches, both against the plain-C oracle: every case runs
under SDX_MS_TILE=128 and SDX_MS_TILE=64, through sdx_demod_pulses(MS) (k_ms_classes) and through
sdx_demod_step (k_step).  Inputs are small: tile positions, the two halves of a 128-message tile,
the workgroup that falls back to two NW = 4 tiles because of one long message, and the pools."""
import functools
import os

import numpy as np
import pytest

from test_full_size import _compare_with_c_oracle

pytestmark = pytest.mark.gpu

TILES = (128, 64)
ROUTES = ("pulses", "step")
# the 128-message tile's pools (TileLds<2, 128, 2> in sdx_tile.h): staged records, payload bytes
PREC_128, PHEAP_128 = 512, 16384


@functools.lru_cache(maxsize=None)
def _env():
    from pysignalduino_amd import bank as B, runtime
    bk = B.Bank()
    return bk, runtime.Engine(bk, 0)


@functools.lru_cache(maxsize=None)
def _corpus(n, seed):
    from pysignalduino_amd import synth
    return synth.ms_corpus(_env()[0].protocols, n, seed=seed)


@functools.lru_cache(maxsize=None)
def _oracle(n, seed):
    """(status, n_rec, lengths) of _corpus(n, seed) from the C oracle: the inputs are chosen with it."""
    from oracle import c_oracle as CO
    cb = CO.CBank()   # (kept alive: the C oracle reads the bank through a pointer)  # noqa: F841
    pb = _corpus(n, seed)
    st, rk, rb, nr, rec, heap = CO.run("MS", CO.pack_batch(pb), max(1, min(16, len(os.sched_getaffinity(0)))))
    return st, nr, np.diff(pb.offsets)


def _launch(route, batch, group=False, mrec=False, work=True, mu=None):
    """One launch of `batch` through sdx_demod_pulses(MS) or sdx_demod_step; host (desc, rec, heap)."""
    import torch
    from pysignalduino_amd import runtime
    bk, eng = _env()
    n = batch.n
    bd = eng.to_device_pulses(batch)
    out = eng.alloc_out(n, 8 * n + 1024, 256 * n + 65536, eng.pulses_work_bytes(n) if work else 0)
    eng.use_mrec = mrec
    try:
        if route == "pulses":
            eng.launch_pulses(runtime.KIND_MS, bd, out, group=group)
        elif mu is not None:   # grouped step: sdx_group_step for both orders, then one k_step
            mbd = eng.to_device_pulses(mu)
            mout = eng.alloc_out(mu.n, 40 * mu.n + 4096, 1024 * mu.n + 65536, eng.pulses_work_bytes(mu.n))
            gmu, gms = eng.group_buffers(mu.n), eng.group_buffers(n)
            o_mu, o_ms = eng.group_step(mbd, bd, gmu, gms)
            eng.launch_step(mu=(mbd, mout, o_mu, gmu[2] if mrec else None), ms=(bd, out, o_ms, gms[2] if mrec else None))
        else:
            eng.launch_step(ms=(bd, out, None, None))
        torch.cuda.synchronize()
    finally:
        eng.use_mrec = False
    return eng.fetch(out)


def _check(route, batch, **kw):
    desc, rec, heap = _launch(route, batch, **kw)
    return _compare_with_c_oracle("MS", _env()[0], batch, desc, rec, heap)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("tm", TILES)
@pytest.mark.parametrize("short_only", [True, False])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 128, 129, 191, 257])
def test_tile_edges_vs_c_oracle(monkeypatch, n, short_only, tm, route):
    """Ungrouped (positions known): the last tile ends inside the first half, at its end, inside the
    second half, at the tile's end, and just past it.  short_only: the corpus' messages of <= 128
    pulses, so that with tm = 128 every workgroup runs the 128-message tile; otherwise the corpus as it
    is, where every workgroup holds a longer message and runs as two NW = 4 tiles."""
    monkeypatch.setenv("SDX_MS_TILE", str(tm))
    st, nr, lens = _oracle(400, 1290)
    idx = np.nonzero(lens <= 128)[0][:257] if short_only else np.arange(257)
    assert len(idx) == 257 and nr[idx[0]] > 0 and st[idx[0]] == 0      # n = 1 still has a result to compare
    if not short_only:
        assert all((lens[idx[w:w + 128]] > 128).any() for w in (0, 128))
    batch = _corpus(400, 1290).subset(idx[:n])
    assert _check(route, batch) == int(nr[idx[:n]].sum()) > 0


@pytest.mark.parametrize("mrec", [False, True])
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("tm", TILES)
def test_grouped_batch_vs_c_oracle(monkeypatch, tm, route, mrec):
    """n >= GROUP_MIN: the grouped order (long messages last), with and without message records;
    the step route groups MU and MS together (sdx_group_step) and runs both in one k_step."""
    from pysignalduino_amd import runtime, synth
    monkeypatch.setenv("SDX_MS_TILE", str(tm))
    n = 4096 + 37
    assert n >= runtime.GROUP_MIN
    st, nr, lens = _oracle(n, 1291)
    assert (lens > 128).sum() > 128 and (lens <= 128).sum() > 1024
    mu = synth.mu_corpus(_env()[0].protocols, n, seed=1292) if route == "step" else None
    assert _check(route, _corpus(n, 1291), group=True, mrec=mrec, mu=mu) == int(nr.sum()) > n // 2


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("tm", TILES)
@pytest.mark.parametrize("pos", [0, 63, 64, 127])
def test_one_long_message_in_a_workgroup_vs_c_oracle(monkeypatch, pos, tm, route):
    """256 messages of <= 128 pulses but one: with tm = 128 the first workgroup runs as two NW = 4
    tiles of 64 (the long message in either, at its first and last position), its neighbour as one
    128-message tile."""
    monkeypatch.setenv("SDX_MS_TILE", str(tm))
    st, nr, lens = _oracle(2000, 1297)
    short = np.nonzero(lens <= 128)[0][:255]
    long_ = np.nonzero((lens > 128) & (nr > 0))[0][:1]
    assert len(short) == 255 and len(long_) == 1
    idx = np.concatenate([short[:pos], long_, short[pos:]])
    assert len(idx) == 256 and nr[idx[:128]].sum() > 64 and nr[idx[128:]].sum() > 64
    assert _check(route, _corpus(2000, 1297).subset(idx)) == int(nr[idx].sum())


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("tm", TILES)
def test_pool_overflow_reruns_exactly(monkeypatch, tm, route):
    """128 copies of a message with five results fill a 128-message tile's record pool (PREC_128)
    without a workspace to spill into: the tile is marked ST_OVF_TILE, its neighbours are not, and
    Engine.run's re-run equals the oracle."""
    from pysignalduino_amd import runtime
    monkeypatch.setenv("SDX_MS_TILE", str(tm))
    st, nr, lens = _oracle(20000, 43)
    rich = np.nonzero((nr >= 5) & (lens <= 128) & (st == 0))[0][:1]
    assert len(rich) == 1
    plain = np.nonzero((lens <= 128) & (nr <= 2))[0][:128]
    idx = np.concatenate([np.repeat(rich, 128), plain])
    assert nr[idx[:128]].sum() > PREC_128 and nr[idx[128:]].sum() < PREC_128 // 2   # against the chosen caps
    batch = _corpus(20000, 43).subset(idx)
    desc, rec, heap = _launch(route, batch, work=False)
    assert (desc["status"][:128] == runtime.ST_OVF_TILE).all()    # 64-message tiles: 320 > their 256 records
    assert (desc["status"][128:] == runtime.ST_OK).all()
    _, eng = _env()
    d2, r2, h2 = eng.run(runtime.KIND_MS, eng.to_device_pulses(batch), workspace=False)
    assert _compare_with_c_oracle("MS", _env()[0], batch, d2, r2, h2) == int(nr[idx].sum())


@pytest.mark.parametrize("route", ROUTES)
def test_tile_size_override_takes_effect(monkeypatch, route):
    """SDX_MS_TILE is read per call: 64 copies of the five-result message overflow a 64-message tile's
    256 records, while the 128-message tile pools them with the 64 plain messages behind them (its 512
    records hold both halves)."""
    from pysignalduino_amd import runtime
    st, nr, lens = _oracle(20000, 43)
    rich = np.nonzero((nr >= 5) & (lens <= 128) & (st == 0))[0][:1]
    plain = np.nonzero((lens <= 128) & (nr <= 2))[0][:64]
    idx = np.concatenate([np.repeat(rich, 64), plain])
    assert 256 < nr[idx[:64]].sum() and nr[idx].sum() < PREC_128
    batch = _corpus(20000, 43).subset(idx)
    monkeypatch.setenv("SDX_MS_TILE", "64")
    desc, _, _ = _launch(route, batch, work=False)
    assert (desc["status"][:64] == runtime.ST_OVF_TILE).all() and (desc["status"][64:] == runtime.ST_OK).all()
    monkeypatch.setenv("SDX_MS_TILE", "128")
    desc, rec, heap = _launch(route, batch, work=False)
    assert (desc["status"] == runtime.ST_OK).all()
    assert _compare_with_c_oracle("MS", _env()[0], batch, desc, rec, heap) == int(nr[idx].sum())


# ---- raising messages.  No MS message raises on the shipped bank: the only MS protocol with a
# postDemodulation method (74.1) has no float symbol, and no generator of the suite (ms_corpus at 300k
# messages, planted_pulse_messages, the goldens) produces a raise on the C oracle.  So these cases
# give 74.1 a float symbol, after which its planted frames raise ValueError (int('F'),
# message_synced.py:203-219) on the oracle, and compare with the oracle on that same edited bank
# (the signature comparison of test_full_size, with the edited CBank instead of the default one).
@functools.lru_cache(maxsize=None)
def _raise_env():
    import copy
    from oracle import c_oracle as CO
    from pysignalduino_amd import bank as B, packing, runtime, synth
    P = copy.deepcopy(_env()[0].protocols)
    P["74.1"]["float"] = [1.5, -1]
    bk = B.Bank(P)
    planted = [m for m in synth.planted_pulse_messages(_env()[0].protocols, "MS", 400, seed=34, corrupt_frac=0.0)
               if len(m["data"]) <= 128][:64]
    pb = _corpus(400, 1290)
    quiet = [pb.to_msg_dict(int(i)) for i in np.nonzero(np.diff(pb.offsets) <= 128)[0][:64]]
    return bk, runtime.Engine(bk, 0), P, planted, quiet


def _compare_edited_bank(bk, P, batch, desc, rec, heap):
    from oracle import c_oracle as CO
    from pysignalduino_amd import runtime
    from test_full_size import _signatures
    cb = CO.CBank(P)
    st, rk, rb, nr, crec, cheap = CO.run("MS", CO.pack_batch(batch), 1)
    gid = {p: i for i, p in enumerate(cb.pids)}
    dev_gid = np.array([gid[p] for p in bk.ms_pids], np.int64)
    dstatus = np.where(desc["status"] == runtime.ST_RAISED, 1, np.where(desc["status"] == runtime.ST_OK, 0, 2))
    assert (dstatus != 2).all()
    sd = _signatures(batch.n, dstatus, desc["raise_kind"], desc["rec_begin"], desc["n_rec"],
                     dev_gid[rec["proto"].astype(np.int64)], rec["bit_length"], rec["payload_off"], rec["payload_len"], heap)
    sc = _signatures(batch.n, st.astype(np.int64), rk, rb, np.where(st == 0, nr, 0), crec["proto"].astype(np.int64),
                     crec["bitlen"], crec["off"], crec["len"], cheap)
    bad = np.nonzero(sd != sc)[0]
    assert len(bad) == 0, f"{len(bad)} of {batch.n} messages differ from the C oracle; first: {bad[:5].tolist()}"
    return st, nr


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("tm", TILES)
@pytest.mark.parametrize("raising_half", [1, 0])
def test_raising_messages_in_one_half_vs_c_oracle(monkeypatch, raising_half, tm, route):
    """128 messages, one half of which raises: message p raises and message p +- 64 (the same lane of
    the other half's waves, the same tile position mod 64) does not."""
    import torch
    from pysignalduino_amd import packing, runtime
    monkeypatch.setenv("SDX_MS_TILE", str(tm))
    bk, eng, P, planted, quiet = _raise_env()
    assert len(planted) == 64 and len(quiet) == 64
    pk = packing.PulsePacker("MS")
    for m in (quiet + planted if raising_half else planted + quiet):
        pk.add(m)
    batch = pk.batch()
    bd = eng.to_device_pulses(batch)
    out = eng.alloc_out(128, 8 * 128 + 1024, 256 * 128 + 65536, eng.pulses_work_bytes(128))
    if route == "pulses":
        eng.launch_pulses(runtime.KIND_MS, bd, out, group=False)
    else:
        eng.launch_step(ms=(bd, out, None, None))
    torch.cuda.synchronize()
    st, nr = _compare_edited_bank(bk, P, batch, *eng.fetch(out))
    r, q = (slice(64, 128), slice(0, 64)) if raising_half else (slice(0, 64), slice(64, 128))
    assert (st[r] == 1).all() and (st[q] == 0).all() and nr[q].sum() > 16   # the oracle raises / returns results
