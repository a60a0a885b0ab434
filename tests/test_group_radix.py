"""The grouping's radix sort (sdx_group.hip) at the sizes where its structure changes: a wave's
sub-chunk (64), a wave's share of a partition (256), a workgroup (512), a partition (2048), several
partitions with a ragged tail -- and with ties that span waves and partitions, `sel` subsets and the
MS length-class bit.

Every case checks, for sdx_group_pulses (Engine.group) and for sdx_group_step (Engine.group_step):
the order is a permutation of the input positions, the sorted keys left in the workspace's first
array are non-decreasing, equal keys keep their input order; and the two entries' orders are equal
byte for byte."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049, 4095, 4097, 3 * 2048 + 300]
N_TIES = 5000


@functools.lru_cache(maxsize=None)
def _engine():
    from pysignalduino_amd import bank as B, runtime
    bk = B.Bank()
    eng = runtime.Engine(bk, 0)
    eng.use_mrec = True
    return bk, eng


@functools.lru_cache(maxsize=None)
def _corpus(kind):
    """One host corpus per kind, as large as the largest case; never modified."""
    from pysignalduino_amd import synth
    bk, _ = _engine()
    gen = synth.mu_corpus if kind == "MU" else synth.ms_corpus
    return gen(bk.protocols, max(SIZES), seed=1301 if kind == "MU" else 1302)


@functools.lru_cache(maxsize=None)
def _device(kind, n, period=0):
    """The corpus' first n messages on the device; period > 0: its first `period` messages repeated."""
    _, eng = _engine()
    idx = np.arange(n) % period if period else np.arange(n)
    return eng.to_device_pulses(_corpus(kind).subset(idx))


def _kd(kind):
    from pysignalduino_amd import runtime
    return runtime.KIND_MU if kind == "MU" else runtime.KIND_MS


def _host(order, bufs, n):
    return (order.cpu().numpy().astype(np.int64),
            bufs[1][: 4 * n].cpu().numpy().view(np.uint32).astype(np.int64))


def _check_sorted(o, keys, n, n_batch, sel=None):
    """permutation of the input positions, keys non-decreasing, ties in input order; -> positions"""
    assert o.shape == (n,) and keys.shape == (n,)
    assert ((o >= 0) & (o < n_batch)).all()
    if sel is None:
        pos = o
    else:
        pos_of = np.full(n_batch, -1, np.int64)
        pos_of[sel] = np.arange(n)
        pos = pos_of[o]
    assert np.array_equal(np.sort(pos), np.arange(n))
    assert (np.diff(keys) >= 0).all()
    assert (np.diff(pos)[np.diff(keys) == 0] > 0).all()
    return pos


def _both(mu_bd, ms_bd, mu_sel=None, ms_sel=None):
    """Both groupings through Engine.group and through Engine.group_step, checked and compared;
    -> {kind: (order, sorted keys)} as host arrays."""
    import torch
    from pysignalduino_amd import runtime
    _, eng = _engine()
    bd = {"MU": mu_bd, "MS": ms_bd}
    sel = {"MU": mu_sel, "MS": ms_sel}
    dsel = {k: None if s is None else torch.from_numpy(np.ascontiguousarray(s, dtype=np.int32)).to(eng.dev)
            for k, s in sel.items()}
    n = {k: bd[k]["n"] if sel[k] is None else len(sel[k]) for k in bd}
    one = {k: eng.group_buffers(n[k], bd[k]["n"]) for k in bd}
    two = {k: eng.group_buffers(n[k], bd[k]["n"]) for k in bd}
    for k in bd:  # the comparison below must not pass on what an earlier case left in recycled memory
        for b in (one[k], two[k]):
            b[0].fill_(-1)
            b[2].zero_()
    o1 = {k: eng.group(_kd(k), bd[k], sel=dsel[k], bufs=one[k]) for k in bd}
    o2 = dict(zip(("MU", "MS"), eng.group_step(bd["MU"], bd["MS"], two["MU"], two["MS"], dsel["MU"], dsel["MS"])))
    torch.cuda.synchronize()
    res = {}
    for k in bd:
        assert o1[k].numel() == n[k] and o2[k].numel() == n[k], k
        assert torch.equal(o1[k], o2[k]), k
        nb = bd[k]["n"] * runtime.MREC_BYTES
        assert torch.equal(one[k][2][:nb], two[k][2][:nb]), k   # the message records (zero outside sel)
        for order, bufs in ((o1[k], one[k]), (o2[k], two[k])):
            o, keys = _host(order, bufs, n[k])
            _check_sorted(o, keys, n[k], bd[k]["n"], sel[k])
        res[k] = (o, keys)
    return res


@pytest.mark.parametrize("n_mu,n_ms", list(zip(SIZES, reversed(SIZES))))
def test_sizes_around_the_structure(n_mu, n_ms):
    """Every size is an MU side once and an MS side once; the sides of a step are never equal and
    the extreme pairs have a one-message side."""
    assert n_mu != n_ms
    _both(_device("MU", n_mu), _device("MS", n_ms))


@pytest.mark.parametrize("period", [1, 3, 64, 65])
def test_ties_across_waves_and_partitions(period):
    """`period` distinct messages repeated up to n = 5000: every class of equal messages has one key
    and lies in several waves and partitions; it must come out in ascending position.  One message
    (a single digit bin holds whole partitions in all four passes) gives the identity order."""
    res = _both(_device("MU", N_TIES, period), _device("MS", N_TIES - 1, period))
    for k, (o, keys) in res.items():
        cls = o % period
        by_class = np.argsort(cls, kind="stable")
        inside = np.diff(cls[by_class]) == 0
        assert (np.diff(o[by_class])[inside] > 0).all(), k
        if period == 1:
            assert np.array_equal(o, np.arange(len(o))), k
            assert (keys == keys[0]).all(), k


def test_sel_subsets_keep_sel_order_and_the_keys():
    """A descending and a shuffled `sel` of 3000 (2999) of 5000 messages: ties keep the order of
    `sel`, not of the messages, and every message gets the key it has in the full-batch run."""
    rng = np.random.default_rng(1303)
    bd = {"MU": _device("MU", N_TIES), "MS": _device("MS", N_TIES)}
    full = _both(bd["MU"], bd["MS"])
    key_of = {}
    for k, (o, keys) in full.items():
        key_of[k] = np.empty(N_TIES, np.int64)
        key_of[k][o] = keys
        assert len(np.unique(keys)) > 1, k
    desc = np.sort(rng.permutation(N_TIES)[:3000])[::-1].copy()
    shuf = rng.permutation(N_TIES)[:2999]
    for mu_sel, ms_sel in ((desc, shuf), (shuf, desc)):
        res = _both(bd["MU"], bd["MS"], mu_sel, ms_sel)
        for k, (o, keys) in res.items():
            assert np.array_equal(key_of[k][o], keys), k


def test_keys_do_not_depend_on_the_neighbours_pattern_count():
    """k_sig tests 8 pattern slots in a wave whose messages all have at most 8 patterns and all 10
    otherwise.  Giving one message in each of two waves two more patterns switches those waves to the
    10-slot form; every other message must keep its key."""
    n = 512
    _, eng = _engine()
    keys = {}
    for kind in ("MU", "MS"):
        base = _corpus(kind).subset(np.arange(n))
        assert base.npat.max() <= 8
        wide = _corpus(kind).subset(np.arange(n))
        changed = [5, 200]                                   # waves 0 and 3 of the first 256 messages
        for j in changed:
            used = set(wide.pat_id[j, : wide.npat[j]].tolist())
            free = [d for d in range(ord("0"), ord("9") + 1) if d not in used]
            for slot in range(int(wide.npat[j]), 10):
                wide.pat_id[j, slot] = free.pop()
                wide.pat_val[j, slot] = 1234.0 * (slot - 3)
            wide.npat[j] = 10
        keys[kind] = [eng.to_device_pulses(base), eng.to_device_pulses(wide)]
    key_of = []
    for v in (0, 1):
        res = _both(keys["MU"][v], keys["MS"][v])
        key_of.append({k: np.empty(n, np.int64) for k in res})
        for k, (o, ks) in res.items():
            key_of[v][k][o] = ks
    same = np.ones(n, bool)
    same[changed] = False
    for k in ("MU", "MS"):
        assert len(np.unique(key_of[0][k])) > 1, k
        assert np.array_equal(key_of[0][k][same], key_of[1][k][same]), k


def test_ms_long_class_comes_last():
    """MS messages of more than 128 pulses carry the key's top bit: mixed with shorter ones they all
    come after them (ms_tile_by_class relies on it)."""
    bd = _device("MS", N_TIES)
    long_ = np.asarray(bd["lengths"]) > 128
    assert 0 < long_.sum() < N_TIES
    o, keys = _both(_device("MU", 300), bd)["MS"]
    assert (np.diff(long_[o].astype(np.int64)) >= 0).all()
    assert np.array_equal(keys >> 31, long_[o].astype(np.int64))
