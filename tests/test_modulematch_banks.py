"""The MU ``modulematch`` filter on the device for patterns the shipped bank does not have: a bank whose
``modulematch`` entries are replaced before first use, as a user's own protocols.json would, against the oracle
on the same edited bank (the method of test_general_modified_bank_repetition_bounds_vs_oracle).

The shipped bank gives ``mm_on`` 3 (digit-count interval) to 64 protocols, 1 (LDS hex-table walk) to 3 that
share two patterns, and 2 (byte walk through t256) to none.  The edits below give each mode to several of the
MU protocols that synth.planted_pulse_messages reaches, with counted tails, unanchored windows, alternations,
anchored prefixes with counted bodies and pure digit counts; the windows' tables together exceed MMTAB_LDS, so
the later ones keep mode 2.  The shipped bank has one MU protocol with a postamble and the planted messages do
not reach it, so two planted protocols are also given a postamble (in both oracle runs alike): ``$`` then
stands behind it, and one pattern asks for its characters.

The oracle is run twice, with the edited modulematches and with them removed; the difference says what the
filter keeps and removes, per mode and on the general path, from the oracle alone.  As measured: mm_on 1 / 2 / 3
on 4 / 10 / 3 of the 17 edited protocols; kept and removed 290 / 277 (mode 1), 384 / 532 (mode 2), 96 / 140
(mode 3), 646 / 1176 (general path); every edited protocol has both."""
import collections

import numpy as np
import pytest

from oracle import sd_oracle as O

pytestmark = pytest.mark.gpu

# pid -> pattern; the payload is preamble + upper-case hex digits + postamble
EDITS = {
    # counted tails and `$`, content-dependent: the hex-table walk (or, once LDS is full, the byte walk)
    "70": r"[0-9A-F]{3}[0-7]F0$",                  # `$` behind the postamble given below, which the pattern names
    "67": r"^TX[0-9A-F]{5}[0-7]",                  # an anchored prefix with a counted body
    "66": r"(?:[0-7][0-9A-F]|[89A-F][0-7]){2,3}$",    # an alternation under a count, at the end
    "1": r"^P1#(?:[0-9A-F]{2}){4}[0-7]",
    "74": r"[0-9A-F]{2}[0-7][0-9A-F]$",
    "63": r"[0-7]{3}$",                            # `$` behind a postamble the pattern does not name
    # unanchored windows of 2^6 and 2^7 states: 17 bytes of LDS table a state
    "45": r"[0-3].{6}[C-F]", "74.1": r"[A-F].{6}[A-F]", "73": r"[C-F].{6}[89AB]",
    "80": r"[0-3].{5}[4-7]", "88": r"[0-7].{6}[0-3]", "35": r"[0-7].{5}[89A-F]",
    "72.1": r"[0-3].{6}[0-7]",
    # pure digit counts: an interval of lengths, no walk on the device up to 64 digits
    "39": r"^.{13}", "60": r"^K.{7}", "40": r"^u40#.{9,14}$",
    "82": r"^P82#.{108}",                          # more than 64 digits: the interval does not reach, the table is walked
}
POSTAMBLES = {"70": "F0", "63": "07"}


def _flat(res):
    if isinstance(res, BaseException):
        return {"raise": type(res).__name__}
    return {"results": [[r["protocol_id"], r["payload"], r["meta"]["bit_length"], r["meta"]["rssi"],
                         r["meta"]["clock"]] for r in res]}


def _oracle(ob, msg):
    try:
        return _flat(O.demod(ob, dict(msg), "MU"))
    except Exception as e:
        return {"raise": type(e).__name__}


def messages(P):
    """-> [(path, msg)]: planted messages of the edited protocols, the same stretched beyond 256 pulses (the long
    variant), and re-keyed ones for the general path, interleaved."""
    from pysignalduino_amd import synth
    short = synth.planted_pulse_messages(P, "MU", 420, seed=71, corrupt_frac=0.0)
    long_ = []
    for m in synth.planted_pulse_messages(P, "MU", 120, seed=72, corrupt_frac=0.0):
        d = m["D"] * (1 + 300 // max(len(m["D"]), 1))
        long_.append(dict(m, D=d, data=d))
    general = synth.general_pulse_messages(P, "MU", 140, seed=73)
    out = [("short", m) for m in short] + [("long", m) for m in long_] + [("general", m) for m in general]
    np.random.default_rng(74).shuffle(out)
    return out


@pytest.fixture(scope="module")
def edited():
    """-> (SDProtocols with the edits, its protocol list, the same list without the edited modulematches)."""
    import copy
    from pysignalduino_amd.sd_protocols import SDProtocols
    p = SDProtocols()
    for pid, post in POSTAMBLES.items():
        p._protocols[pid]["postamble"] = post
    plain = copy.deepcopy(p.get_protocol_list())
    for pid in EDITS:
        plain[pid].pop("modulematch", None)
    for pid, pat in EDITS.items():
        p._protocols[pid]["modulematch"] = pat
    return p, p.get_protocol_list(), plain


def test_edited_bank_filters_as_the_oracle(edited):
    from pysignalduino_amd import bank
    p, P, plain = edited
    # ---- the modes the bank compiler gives the edits (host)
    b = bank.Bank(P)
    mode = {pid: int(b.mu_desc["mm_on"][r]) for r, pid in enumerate(b.mu_pids) if pid in EDITS}
    assert set(mode) == set(EDITS)
    hist = collections.Counter(mode.values())
    print("mm_on of the edited protocols:", sorted(mode.items()), dict(hist))
    assert all(hist[k] >= 3 for k in (1, 2, 3)), hist
    intervals = {(int(b.mu_desc["res"][r][0]), int(b.mu_desc["res"][r][1])) for r, pid in enumerate(b.mu_pids)
                 if mode.get(pid) == 3}
    assert len(intervals) >= 2, intervals
    assert all(d[0] <= 256 for d in b.dfa_host[1])
    # ---- what the filter keeps and removes, from the oracle alone
    msgs = messages(P)
    assert sum(len(m["D"]) > 256 for path, m in msgs if path == "long") >= 100
    ob, ob_plain = O.OracleBank(P), O.OracleBank(plain)
    exp = [_oracle(ob, m) for _, m in msgs]
    kept, removed = collections.Counter(), collections.Counter()
    by_pid = collections.defaultdict(lambda: [0, 0])
    digits64 = 0
    for (path, m), e in zip(msgs, exp):
        with_mm = collections.Counter(r[0] for r in e.get("results", []) if r[0] in EDITS)
        without = collections.Counter(r[0] for r in _oracle(ob_plain, m).get("results", []) if r[0] in EDITS)
        digits64 += sum(r[0] == "82" and len(r[1]) > 4 + 64 for r in e.get("results", []))
        for pid in without:
            assert with_mm[pid] <= without[pid]
            key = "general" if path == "general" else mode[pid]
            kept[key] += with_mm[pid]
            removed[key] += without[pid] - with_mm[pid]
            by_pid[pid][0] += with_mm[pid]
            by_pid[pid][1] += without[pid] - with_mm[pid]
    print("kept:", dict(kept), "removed:", dict(removed), "per protocol (kept, removed):", dict(by_pid))
    for key in (1, 2, 3, "general"):
        assert kept[key] >= 50 and removed[key] >= 50, (key, kept[key], removed[key])
    both = sum(1 for pid in EDITS if by_pid[pid][0] and by_pid[pid][1])
    assert 3 * both >= 2 * len(EDITS), (both, len(EDITS))
    assert digits64 >= 5          # kept results of more than 64 digits under a digit-count pattern
    # ---- the device: every slot of one interleaved call
    got = p.demodulate_batch([m for _, m in msgs], "MU")
    bad = [(i, msgs[i][0], e, _flat(g)) for i, (e, g) in enumerate(zip(exp, got)) if _flat(g) != e]
    assert not bad, f"{len(bad)}/{len(msgs)} mismatches; first: {bad[:2]}"
