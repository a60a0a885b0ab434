"""Dispatch rules on the host: DispatchRules.reduce against an independent restatement of the
definition, the hand cases, the mask compiler, the figures of tests/golden/lines_golden.json.gz, the ABI, and
the struct's validator under the sanitizers.  No GPU."""
import collections
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from pysignalduino_amd import bank as bankmod
from pysignalduino_amd import runtime
from pysignalduino_amd.dispatch import DispatchRules, as_rules

ROOT = os.path.dirname(runtime.HERE)
COUNTS = (129, 66, 12, 19)      # this bank's class counts (test_profiles_host.py pins them)
BANK_KEEP = {"72", "72.1", "101"}


@pytest.fixture(scope="module")
def bank():
    return bankmod.Bank()


def restate(msgs, cap=4, drop_equal=True, keep=frozenset(BANK_KEEP)):
    """The definition written a second way: first the cap as a filter over (run index within the run of equal
    protocols), then the equal-drop over what passed it.  msgs: (protocol_id, payload) pairs -> kept indices."""
    passed, j = [], 0
    while j < len(msgs):
        e = j
        while e < len(msgs) and msgs[e][0] == msgs[j][0]:
            e += 1
        passed += list(range(j, e if cap == 0 else min(e, j + cap)))
        j = e
    out = []
    for x, i in enumerate(passed):
        before = msgs[passed[x - 1]] if x else None
        equal = before is not None and before[0] == msgs[i][0] and before[1] == msgs[i][1]
        if not (drop_equal and equal and msgs[i][0] not in keep):
            out.append(i)
    return out


def run(bank, msgs, **kw):
    kept = DispatchRules(**kw).reduce(bank, "MU", [(p, d, i) for i, (p, d) in enumerate(msgs)])
    return [m[2] for m in kept]


# ---- hand cases -------------------------------------------------------------------------------------------
def test_hand_cases(bank):
    A, B, K = "7", "61", "72"           # 72 carries dispatchequals
    a5 = [(A, "x")] * 5
    assert run(bank, a5) == [0]                                             # nrDispatch counts the equal ones too
    assert run(bank, a5, drop_equal=False) == [0, 1, 2, 3]
    assert run(bank, a5, max_repeat=1) == [0] and run(bank, a5, max_repeat=1, drop_equal=False) == [0]
    assert run(bank, a5, max_repeat=0, drop_equal=False) == [0, 1, 2, 3, 4] and run(bank, a5, max_repeat=0) == [0]
    assert run(bank, [(A, "1"), (A, "1"), (A, "2")]) == [0, 2]              # A1 A1 A2
    assert run(bank, [(A, "1"), (B, "1"), (A, "1")]) == [0, 1, 2]           # A B A: the predecessor alone counts
    assert run(bank, [(A, "1"), (B, "1")]) == [0, 1]                        # an equal payload under another protocol
    assert run(bank, [(K, "x")] * 6) == [0, 1, 2, 3]                        # dispatchequals: the cap alone
    assert run(bank, [(K, "x")] * 6, keep_equal=()) == [0]
    assert run(bank, [(A, "x")] * 3, keep_equal=[7]) == [0, 1, 2]           # ids are compared as str(id)
    # a record beyond the cap does not become ``last``: x x x x | y(capped) then B, then A y is a new run
    six = [(A, "1"), (A, "2"), (A, "3"), (A, "4"), (A, "5"), (B, "5"), (A, "4")]
    assert run(bank, six) == [0, 1, 2, 3, 5, 6]
    # ... and the run index restarts with the protocol: cap + 1 of A, B, cap + 1 of A again
    assert run(bank, [(A, str(i)) for i in range(5)] + [(B, "b")] + [(A, str(i)) for i in range(5)]) == [0, 1, 2, 3, 5, 6, 7, 8, 9]
    # profiles first: with B disabled A B A is A A to the rules (one A left); the rules first would leave A A
    aba = [(A, "1"), (B, "1"), (A, "1")]
    enabled = [m for m in aba if m[0] != B]
    assert run(bank, enabled) == [0] and [aba[i] for i in run(bank, aba) if aba[i][0] != B] == [aba[0], aba[2]]
    # the key has no bit_length / metadata: objects with other attributes are reduced by id and payload alone
    M = collections.namedtuple("M", "protocol_id payload metadata")
    objs = [M("7", "x", {"bit_length": 8}), M("7", "x", {"bit_length": 9}), M(7, "x", {})]
    assert DispatchRules().reduce(bank, 0, objs) == objs[:1]
    assert DispatchRules().reduce(bank, "MS", []) == []


def test_against_the_restatement_on_random_lists(bank):
    rng = np.random.default_rng(18)
    ids = ["7", "61", "72", "72.1", "1", "101"]
    n_changed = 0
    for trial in range(3000):
        m = int(rng.integers(0, 14))
        msgs, p = [], None
        for _ in range(m):
            if p is None or rng.random() < 0.35:
                p = ids[int(rng.integers(0, len(ids)))]
            msgs.append((p, "ab"[int(rng.integers(0, 2))] * int(rng.integers(0, 3))))
        cap = int(rng.choice([0, 1, 2, 4, 5]))
        drop = bool(rng.integers(0, 2))
        keep = [frozenset(BANK_KEEP), frozenset(), frozenset({"7", "61"})][trial % 3]
        kw = dict(max_repeat=cap, drop_equal=drop, keep_equal="bank" if trial % 3 == 0 else sorted(keep))
        got = run(bank, msgs, **kw)
        assert got == restate(msgs, cap, drop, keep), (msgs, kw)
        n_changed += len(got) != m
        if m:
            assert got[0] == 0                                              # r_0 is always kept
        again = DispatchRules(**kw).reduce(bank, "MU", [msgs[i] for i in got])
        assert again == [msgs[i] for i in got]                              # idempotent
    assert n_changed > 800


# ---- arguments and the mask compiler --------------------------------------------------------------------------
def test_arguments(bank):
    assert as_rules(None) is None and isinstance(as_rules(True), DispatchRules)
    r = DispatchRules(max_repeat=2)
    assert as_rules(r) is r and as_rules(True).max_repeat == 4 and as_rules(True).drop_equal and as_rules(True).keep_equal == "bank"
    for bad in (False, 1, "bank", [r]):
        with pytest.raises(ValueError):
            as_rules(bad)
    for kw in (dict(max_repeat=-1), dict(max_repeat=1.5), dict(max_repeat=True), dict(max_repeat=1 << 31), dict(keep_equal="all"),
               dict(keep_equal=72), dict(keep_equal=None)):
        with pytest.raises(ValueError):
            DispatchRules(**kw)
    for call in (lambda x: x.struct(bank), lambda x: x.reduce(bank, "MU", []), lambda x: x.masks(bank)):
        with pytest.raises(ValueError, match="no protocol id"):
            call(DispatchRules(keep_equal=["7", "nope"]))
    with pytest.raises(ValueError):
        DispatchRules().reduce(bank, "XX", [])
    with pytest.raises(ValueError):
        DispatchRules().reduce(bank, 4, [])


def test_mask_compiler(bank):
    from pysignalduino_amd.profiles import class_lists
    lists = class_lists(bank)
    assert tuple(len(x) for x in lists) == COUNTS
    assert all(len({str(p) for p in x}) == len(x) for x in lists)          # a class index names one id: proto == id inside a kind
    assert {str(pid) for pid, p in bank.protocols.items() if p.get("dispatchequals") == "true"} == BANK_KEEP
    s = DispatchRules().struct(bank)
    set_bits = {(kd, str(lists[kd][64 * w + b])) for kd in range(4) for w in range(4) for b in range(64)
                if (s.keep_equal[kd][w] >> b) & 1}
    # 72 and 72.1 in MU's mask, 101 in MN's.  The bank also lists 72.1 (which has a sync: it IS an MS protocol) and 101
    # (whose rfmode entry carries a "sync" key) among the MS classes, and a mask is by id in every kind; no other id is set
    assert {(0, "72"), (0, "72.1"), (3, "101")} <= set_bits
    assert set_bits == {(0, "72"), (0, "72.1"), (1, "72.1"), (1, "101"), (3, "101")}
    assert list(s.max_repeat) == [4] * 4 and s.drop_equal == 1 and s.res == 0
    s = DispatchRules(max_repeat=0, drop_equal=False, keep_equal=[lists[0][63], lists[0][64], lists[0][128], lists[2][11]]).struct(bank)
    assert s.keep_equal[0][0] >> 63 == 1 and s.keep_equal[0][1] & 1 and s.keep_equal[0][2] & 1 and s.keep_equal[0][3] == 0
    assert (s.keep_equal[2][0] >> 11) & 1 and list(s.max_repeat) == [0] * 4 and s.drop_equal == 0
    assert DispatchRules(keep_equal=()).masks(bank) == [[0] * 4] * 4


# ---- the corpus ------------------------------------------------------------------------------------------------
def test_lines_golden_figures(golden, bank):
    cases = golden("lines_golden.json.gz")
    lists = [c["e2e"] for c in cases if c.get("e2e")]
    assert len(cases) == 4169 and len(lists) == 1267
    assert sum(len(x) >= 2 for x in lists) == 536 and max(len(x) for x in lists) == 8 and sum(len(x) for x in lists) == 2526
    same = lambda a, b: a[0] == b[0] and a[1] == b[1]       # noqa: E731
    assert sum(any(same(x[j], x[j - 1]) for j in range(1, len(x))) for x in lists) == 132
    assert any([m[:2] for m in x] == [["46", "P46#BAFB0"]] * 4 for x in lists)
    assert sum(max(collections.Counter(m[0] for m in x).values()) > 4 for x in lists) == 3
    assert all(len({m[3][1] for m in x}) == 1 for x in lists)                           # one kind per list
    # the records of one protocol are contiguous: a run of the definition is FHEM's per-protocol nrDispatch
    assert all(len({m[0] for m in x}) == sum(1 for j in range(len(x)) if j == 0 or x[j][0] != x[j - 1][0]) for x in lists)
    assert sum(m[0] in BANK_KEEP for x in lists for m in x) == 80
    rules = DispatchRules()
    red = [rules.reduce(bank, x[0][3][1], x) for x in lists]
    assert sum(a != b for a, b in zip(red, lists)) == 132 and sum(len(b) - len(a) for a, b in zip(red, lists)) == 305
    for a, b in zip(red, lists):
        assert a[0] is b[0] and rules.reduce(bank, b[0][3][1], a) == a
    idx = [[i for i, m in enumerate(b) if any(m is k for k in a)] for a, b in zip(red, lists)]
    assert idx == [restate([(m[0], m[1]) for m in b]) for b in lists]


# ---- ABI -----------------------------------------------------------------------------------------------------------
def test_abi_declares_the_dispatch_entries():
    hdr = open(os.path.join(ROOT, "include", "sdx.h")).read()
    for name in ("sdx_dispatch_scratch_bytes", "sdx_dispatch_records"):
        assert name in runtime.EXPORTED and re.search(r"\b%s\(" % name, hdr), name
    assert "#define SDX_ABI_VERSION 14" in hdr and runtime.ABI_VERSION == 14     # only new entries: the version stays
    assert ctypes.sizeof(runtime.SdxDispatchRules) == 152 and "/* 152 bytes */" in hdr
    f = runtime.SdxDispatchRules
    assert (f.keep_equal.offset, f.max_repeat.offset, f.drop_equal.offset, f.res.offset) == (0, 128, 144, 148)
    lib = runtime.load_library()
    assert lib.sdx_abi_version() == 14
    assert lib.sdx_dispatch_scratch_bytes(0, 10) == 0 and lib.sdx_dispatch_scratch_bytes(5, 10) == 0
    assert lib.sdx_dispatch_scratch_bytes(1, -1) == 0
    a, b = lib.sdx_dispatch_scratch_bytes(1, 65537), lib.sdx_dispatch_scratch_bytes(4, 65537)
    assert a >= 8 * 65537 + 4 * 257 and b >= 4 * (a - 16) and a % 16 == 0 and lib.sdx_dispatch_scratch_bytes(1, 0) > 0
    assert a <= 16 + 8 * 65537 + 4 * 257 + 32                # 8 B a line and 4 B a block per kind: no flag per record
    from pysignalduino_amd import build
    assert any(s.endswith("sdx_dispatch.hip") for s in build.SRCS) and any(d.endswith("sdx_dispatch_layout.h") for d in build.DEPS)
    # the entry refuses bad rules on the host before any device call (a null bank is tested first: no GPU is needed)
    assert lib.sdx_dispatch_records(None, None, None, 1, 0, None, None, None, None, None, None) == -1
    assert b"sdx_dispatch_records" in lib.sdx_last_error()


def test_rules_validator_under_sanitizers(tmp_path, bank):
    """tools/dispatch_rules_check.cpp: sdx_dispatch_validate over good structs and systematically damaged ones as a
    stand-alone host program built with -fsanitize=address,undefined."""
    src = os.path.join(ROOT, "tools", "dispatch_rules_check.cpp")
    exe = str(tmp_path / "dispatch_rules_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    src, "-o", exe], check=True)
    from pysignalduino_amd.profiles import class_lists
    lists = class_lists(bank)
    cases = {"default": DispatchRules(), "off": DispatchRules(max_repeat=0, drop_equal=False, keep_equal=()),
             "edges": DispatchRules(max_repeat=2 ** 31 - 1, keep_equal=[lists[0][0], lists[0][63], lists[0][64], lists[0][128],
                                                                        lists[1][65], lists[2][11], lists[3][18]])}
    counts = [str(c) for c in COUNTS]
    for name, rules in cases.items():
        f = tmp_path / (name + ".bin")
        f.write_bytes(bytes(rules.struct(bank)))
        r = subprocess.run([exe, str(f), *counts], capture_output=True, text=True)
        assert r.returncode == 0 and "dispatch_rules_check: ok (sizeof 152," in r.stdout, (name, r.stdout, r.stderr[-2000:])
    bad = runtime.SdxDispatchRules()
    bad.res = 1
    f = tmp_path / "bad.bin"
    f.write_bytes(bytes(bad))
    assert subprocess.run([exe, str(f), *counts], capture_output=True).returncode != 0      # the program does refuse
    f.write_bytes(bytes(DispatchRules().struct(bank)))
    assert subprocess.run([exe, str(f), "129", "62", "12", "19"], capture_output=True).returncode != 0   # 72.1 is MS class 62
