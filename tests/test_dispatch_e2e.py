"""Dispatch rules end to end: the recorded lines of tests/golden/lines_golden.json.gz through
parse_lines(dispatch=), parse_lines_json_all and parse_bytes_json_all.

Expected values: the reference-recorded "e2e" message lists pushed through DispatchRules.reduce (the definition on
the host, which test_dispatch_host.py holds against an independent restatement) and the reference's publication of
every message that is left (oracle/json_oracle.message_to_json).  Every line is compared: the ContractError slots must
be exactly those of parse_lines(lines) without the argument, every other line must equal its expectation."""
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import json_oracle as J
from oracle import sd_oracle as O

from test_lines import _flat_msgs
from test_profiles_host import restate_filter

pytestmark = pytest.mark.gpu

KINDS = ("MU", "MS", "MC", "MN")
BLACK = ["61", "15", "1", "40", "113"]


def texts_of(msgs):
    return [J.message_to_json(m[0], m[1], m[2]) for m in msgs]


@pytest.fixture(scope="module")
def sp():
    from pysignalduino_amd.frontend import SignalParser
    return SignalParser()


@pytest.fixture(scope="module")
def setup(golden, sp):
    """lines, the recorded lists, the lists reduced by the default rules, and the ContractError slots of the plain
    parse_lines call (at most 5 % of the corpus, the bound test_lines.py holds it to)."""
    from pysignalduino_amd import bank as bankmod
    from pysignalduino_amd.dispatch import DispatchRules
    from pysignalduino_amd.packing import ContractError
    cases = golden("lines_golden.json.gz")
    lines = [c["line"] for c in cases]
    e2e = [c.get("e2e", []) for c in cases]
    bank = bankmod.Bank()
    rules = DispatchRules()
    red = [rules.reduce(bank, e[0][3][1], e) if e else [] for e in e2e]
    # the preconditions: the rules do change this corpus (test_dispatch_host.py pins the figures: 132 lines, 305 records)
    assert sum(a != b for a, b in zip(red, e2e)) == 132 and sum(len(b) - len(a) for a, b in zip(red, e2e)) == 305
    plain = sp.parse_lines(lines)
    ce = [isinstance(g, ContractError) for g in plain]
    assert sum(ce) <= 0.05 * len(lines)
    assert sum(a != b for a, b, x in zip(red, e2e, ce) if not x) >= 100         # ... on the lines the device decodes, too
    return SimpleNamespace(lines=lines, e2e=e2e, red=red, ce=ce, bank=bank, rules=rules, plain=plain, ContractError=ContractError)


def compare(s, got, exp, flat=lambda x: x):
    """Every line: a ContractError exactly where the plain call has one, the expectation everywhere else."""
    assert len(got) == len(s.lines)
    assert [isinstance(g, s.ContractError) for g in got] == s.ce
    bad = [(i, s.lines[i][:60], exp[i][:2], flat(got[i])[:2]) for i in range(len(got)) if not s.ce[i] and flat(got[i]) != exp[i]]
    assert not bad, (len(bad), bad[:3])


def test_parse_lines_dispatch(setup, sp):
    from pysignalduino_amd.dispatch import DispatchRules
    s = setup
    compare(s, sp.parse_lines(s.lines, dispatch=True), s.red, _flat_msgs)
    compare(s, s.plain, s.e2e, _flat_msgs)                                      # without the argument: every message
    off = DispatchRules(max_repeat=0, drop_equal=False)
    compare(s, sp.parse_lines(s.lines, dispatch=off), s.e2e, _flat_msgs)        # no rule: the pass re-orders records, no more
    cap1 = DispatchRules(max_repeat=1, keep_equal=())
    exp = [cap1.reduce(s.bank, e[0][3][1], e) if e else [] for e in s.e2e]
    assert sum(len(x) for x in exp) < sum(len(x) for x in s.red)
    compare(s, sp.parse_lines(s.lines, dispatch=cap1), exp, _flat_msgs)
    with pytest.raises(ValueError):
        sp.parse_lines(s.lines[:4], dispatch="yes")


def test_parse_lines_json_all_without_and_with_rules(setup, sp):
    s = setup
    every = sp.parse_lines_json_all(s.lines)
    compare(s, every, [texts_of(e) for e in s.e2e])
    assert max(len(x) for x, c in zip(every, s.ce) if not c) == 8
    got = sp.parse_lines_json_all(s.lines, dispatch=True)
    compare(s, got, [texts_of(r) for r in s.red])
    assert sum(len(x) for x, c in zip(got, s.ce) if not c) < sum(len(x) for x, c in zip(every, s.ce) if not c)
    # for every line, the one text parse_lines_json publishes is the first of the list
    one = sp.parse_lines_json(s.lines)
    for lists in (every, got):
        assert [isinstance(x, s.ContractError) for x in one] == s.ce
        assert [x for x, c in zip(one, s.ce) if not c] == [(x[0] if x else None) for x, c in zip(lists, s.ce) if not c]
    assert sp.parse_lines_json_all([]) == [] and sp.parse_lines_json_all([], dispatch=True, collapse_repeats=True) == []
    with pytest.raises(ValueError):
        sp.parse_lines_json_all(s.lines[:4], dispatch=1)
    with pytest.raises(ValueError):
        sp.parse_lines_json_all(s.lines[:4], sources=[0, 0, 0, 0])              # without collapse_repeats or profiles
    with pytest.raises(ValueError):
        sp.parse_lines_json_all(s.lines[:4], repeat_window=1.0)                 # a window needs collapse_repeats and times
    with pytest.raises(TypeError):
        sp.parse_lines_json_all(s.lines[:4], output="wire")                     # no such argument
    with pytest.raises(TypeError):
        sp.stream(chunk_lines=64, dispatch=True)                                # the stream has no dispatch rules


def test_profiles_run_in_front_of_the_rules(setup, sp):
    """Four receivers (g % 4) with four profiles: a disabled protocol never runs, so it neither counts towards the cap
    nor stands between two equal messages."""
    from pysignalduino_amd.profiles import Profile, ReceiverProfiles
    s = setup
    P = O.OracleBank().p
    ids = sorted({m[0] for e in s.e2e for m in e}, key=float)
    kws = [dict(whitelist=ids[::2]), dict(blacklist=BLACK), dict(skip_development=True), dict()]
    src = np.arange(len(s.lines), dtype=np.int32) % 4
    filt = [restate_filter(P, KINDS.index(e[0][3][1]), e, **kws[int(k)]) if e else [] for e, k in zip(s.e2e, src)]
    exp = [s.rules.reduce(s.bank, f[0][3][1], f) if f else [] for f in filt]
    # (on this corpus the other order gives the same lists; test_dispatch_host.py has the hand case where it does not)
    assert sum(a != b for a, b in zip(exp, filt)) >= 100 and sum(a != b for a, b in zip(filt, s.e2e)) >= 200
    rp = ReceiverProfiles([Profile(**kw) for kw in kws], [0, 1, 2, 3])
    compare(s, sp.parse_lines_json_all(s.lines, dispatch=True, profiles=rp, sources=src), [texts_of(x) for x in exp])
    compare(s, sp.parse_lines(s.lines, dispatch=True, profiles=rp, sources=src), exp, _flat_msgs)
    compare(s, sp.parse_lines_json_all(s.lines, profiles=rp, sources=src), [texts_of(x) for x in filt])


def test_collapse_repeats_on_the_reduced_lists(setup, sp):
    """Every result-bearing line twice in a row: the repeat mask is repeats.py's host restatement run on the reduced
    lists (a ContractError slot has no result), and a repeat line gives []."""
    from pysignalduino_amd import repeats
    s = setup
    idx = [i for i in range(len(s.lines)) for _ in range(2 if s.e2e[i] else 1)]
    lines = [s.lines[i] for i in idx]
    objs = [[] if s.ce[i] else [SimpleNamespace(protocol_id=m[0], payload=m[1], raw=SimpleNamespace(message_type=m[3][1]))
                               for m in s.red[i]] for i in idx]
    exp_mask = repeats.collapse_objects(objs).tolist()
    assert sum(exp_mask) > 1000
    got = sp.parse_lines_json_all(lines, dispatch=True, collapse_repeats=True)
    assert sp.last_repeat_mask.tolist() == exp_mask
    assert [isinstance(g, s.ContractError) for g in got] == [s.ce[i] for i in idx]
    exp = [[] if m else texts_of(s.red[i]) for i, m in zip(idx, exp_mask)]
    bad = [(j, lines[j][:60]) for j, i in enumerate(idx) if not s.ce[i] and got[j] != exp[j]]
    assert not bad, (len(bad), bad[:3])
    # the objects path: the same mask, the reduced lists
    got = sp.parse_lines(lines, dispatch=True, collapse_repeats=True)
    assert sp.last_repeat_mask.tolist() == exp_mask
    assert all(_flat_msgs(got[j]) == ([] if exp_mask[j] else s.red[i]) for j, i in enumerate(idx) if not s.ce[i])


def test_parse_bytes_json_all(setup, sp):
    s = setup
    one = [i for i in range(len(s.lines)) if s.lines[i].endswith("\n") and s.lines[i].count("\n") == 1]
    assert len(one) > 3000
    data = "".join(s.lines[i] for i in one).encode("latin-1")
    sub = SimpleNamespace(lines=[s.lines[i] for i in one], ce=[s.ce[i] for i in one], ContractError=s.ContractError)
    compare(sub, sp.parse_bytes_json_all(data, dispatch=True), [texts_of(s.red[i]) for i in one])
    compare(sub, sp.parse_bytes_json_all(data), [texts_of(s.e2e[i]) for i in one])
    compare(sub, sp.parse_bytes(data, dispatch=True), [s.red[i] for i in one], _flat_msgs)
    got, tail = sp.parse_bytes_json_all(data + b"MU;P0=1", final=False, dispatch=True)
    assert tail == b"MU;P0=1" and len(got) == len(one)
    assert sum(len(x) for x, c in zip(got, sub.ce) if not c) == sum(len(s.red[i]) for i in one if not s.ce[i])
