"""Receiver profiles on the host: the profile compiler against the definition restated here, the
blob through the host validator, the ABI, the validator under the sanitizers as a stand-alone program, and the
equivalence that lets a filtered list stand for a restricted bank: for every recorded message the reference
does not raise on, the oracle on a bank restricted to the enabled ids gives the full list filtered.

Nothing here needs a GPU."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from oracle import lines_oracle as LO
from oracle import mn_oracle as M
from oracle import sd_oracle as O
from pysignalduino_amd import bank as bankmod
from pysignalduino_amd import profiles as PF
from pysignalduino_amd import runtime
from pysignalduino_amd.profiles import Profile, ReceiverProfiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVELOP = {"75", "77", "82", "5", "63", "2", "72.1"}


@pytest.fixture(scope="module")
def bank():
    return bankmod.Bank()


@pytest.fixture(scope="module")
def obank():
    return O.OracleBank()


# ---- the definition, restated ------------------------------------------------------------------------
def restate_enabled(P, pid, kind, whitelist=None, blacklist=(), rfmode=None, skip_development=False):
    wl = None if whitelist is None else {str(i) for i in whitelist}
    bl = {str(i) for i in blacklist}
    pid = str(pid)
    return ((wl is None or pid in wl) and pid not in bl
            and (not skip_development or "developId" not in P[pid] or (wl is not None and pid in wl))
            and (kind != 3 or rfmode is None or P[pid].get("rfmode") == rfmode))


def restate_filter(P, kind, messages, **kw):
    """A line's (protocol_id, ...) messages -> the ones the profile keeps, in order."""
    return [m for m in messages if restate_enabled(P, m[0], kind, **kw)]


def class_lists(bank):
    return [bank.mu_pids, bank.ms_pids, bank.mc_pids, bank.mn_pids]


CASES = [
    dict(),
    dict(whitelist=["7", "61", "72.1", "100"]),
    dict(blacklist=[61, 15, 1, 40, 113]),
    dict(whitelist=["7", "61", "1", "2"], blacklist=["61", "2"]),
    dict(skip_development=True),
    dict(skip_development=True, whitelist=["5", "72.1", "7"]),          # whitelisted develop ids stay on
    dict(skip_development=True, whitelist=["7", "13"]),
    dict(rfmode="Lacrosse_mode1"),
    dict(rfmode="Bresser_5in1", blacklist=["7"]),
    dict(rfmode="NoSuchMode"),
    dict(whitelist=[]),
]


def test_class_counts_and_develop_ids(bank):
    assert [len(x) for x in class_lists(bank)] == [129, 66, 12, 19]
    assert {pid for pid, p in bank.protocols.items() if "developId" in p} == DEVELOP


@pytest.mark.parametrize("kw", CASES, ids=[str(i) for i in range(len(CASES))])
def test_compile_is_the_definition(bank, kw):
    P = bank.protocols
    got = Profile(**kw).compile(bank)
    for kd, pids in enumerate(class_lists(bank)):
        exp = [c for c, pid in enumerate(pids) if restate_enabled(P, pid, kd, **kw)]
        assert got[kd] == exp, (kd, kw)
    rp = ReceiverProfiles([Profile(), Profile(**kw)], of_source=[1, 0, 1])
    m = rp.masks(bank)
    for kd, pids in enumerate(class_lists(bank)):
        bits = [c for c in range(256) if (int(m[1, kd, c >> 6]) >> (c & 63)) & 1]
        assert bits == got[kd]
        assert [c for c in range(256) if (int(m[0, kd, c >> 6]) >> (c & 63)) & 1] == list(range(len(pids)))
        for s, prof in ((0, 1), (1, 0), (2, 1)):
            exp = {str(pids[c]) for c in (got[kd] if prof else range(len(pids)))}
            assert rp.enabled_ids(bank, s, kd) == exp
    assert rp.enabled_ids(bank, 3, 0) == frozenset() and rp.enabled_ids(bank, -1, "MU") == frozenset()


def test_compile_cases_cover_the_issue(bank):
    P = bank.protocols
    lists = class_lists(bank)
    two = [pid for pid in lists[0] if pid in lists[1]]                      # ids that are in two kinds
    assert two, "no protocol id in both MU and MS"
    got = Profile(whitelist=[two[0]]).compile(bank)
    assert got[0] == [lists[0].index(two[0])] and got[1] == [lists[1].index(two[0])] and got[2] == got[3] == []
    got = Profile(blacklist=[two[0]]).compile(bank)
    assert lists[0].index(two[0]) not in got[0] and lists[1].index(two[0]) not in got[1]
    # an rfmode that two MN protocols share: this bank has none, so a bank with its protocols and one rfmode changed
    import copy
    from types import SimpleNamespace
    P2 = copy.deepcopy(P)
    a_pid, b_pid = lists[3][4], lists[3][10]
    assert P2[a_pid]["rfmode"] != P2[b_pid]["rfmode"]
    P2[b_pid]["rfmode"] = P2[a_pid]["rfmode"]
    bank2 = SimpleNamespace(protocols=P2, mu_pids=lists[0], ms_pids=lists[1], mc_pids=lists[2], mn_pids=lists[3])
    got = Profile(rfmode=P2[a_pid]["rfmode"]).compile(bank2)
    assert got[3] == [4, 10] == [c for c, pid in enumerate(lists[3]) if restate_enabled(P2, pid, 3, rfmode=P2[a_pid]["rfmode"])]
    assert Profile(rfmode=P2[a_pid]["rfmode"], blacklist=[a_pid]).compile(bank2)[3] == [10]
    assert Profile(rfmode=P[a_pid]["rfmode"]).compile(bank)[3] == [4]
    assert got[0] == list(range(129)) and got[1] == list(range(66))         # rfmode is an MN matter
    # skip_development with and without a whitelisted develop id
    dev_mu = [c for c, pid in enumerate(lists[0]) if "developId" in P[pid]]
    assert dev_mu
    assert not set(Profile(skip_development=True).compile(bank)[0]) & set(dev_mu)
    pid = lists[0][dev_mu[0]]
    assert Profile(skip_development=True, whitelist=[pid, "7"]).compile(bank)[0].count(dev_mu[0]) == 1
    assert Profile().compile(bank) == [list(range(len(x))) for x in lists]  # the default enables everything
    # dotted ids are compared as strings; numbers are accepted
    assert Profile(whitelist=[72.1]).compile(bank) == Profile(whitelist=["72.1"]).compile(bank)
    assert sum(map(len, Profile(whitelist=[72.1]).compile(bank))) >= 1
    for bad in (dict(whitelist=["7", "9999"]), dict(blacklist=["no"]), dict(whitelist=[72])):
        if "72" in P and bad == dict(whitelist=[72]):
            continue
        with pytest.raises(ValueError):
            Profile(**bad).compile(bank)
    with pytest.raises(ValueError):
        ReceiverProfiles([Profile(whitelist=["nope"])]).blob(bank)


def test_receiver_profiles_arguments(bank):
    rp = ReceiverProfiles([Profile()])
    assert rp.n_sources == 1 and rp.of_source.tolist() == [0] and rp.is_default
    assert not ReceiverProfiles([Profile(), Profile(blacklist=["7"])], [0, 1]).is_default
    for args in (([],), ([Profile()] * 65,), ([Profile()], [1]), ([Profile()], [-1]), ([Profile()], []),
                 ([Profile()], [0] * 4097), (["x"],), ([Profile()], [0.5])):
        with pytest.raises(ValueError):
            ReceiverProfiles(*args)
    assert ReceiverProfiles([Profile()] * 64, [63] * 4096).n_sources == 4096
    x, y = bank.ms_pids[0], bank.ms_pids[1]
    both = ReceiverProfiles([Profile(rfmode="Bresser_5in1"), Profile(rfmode="Lacrosse_mode1", blacklist=[x])], [0, 1])
    P = bank.protocols
    exp = 0
    for c, pid in enumerate(bank.mn_pids):
        if P[pid].get("rfmode") in ("Bresser_5in1", "Lacrosse_mode1"):
            exp |= 1 << c
    assert both.mn_elig(bank) == exp and exp
    assert ReceiverProfiles([Profile()]).mn_elig(bank) == (1 << len(bank.mn_pids)) - 1
    msgs = [(x, "a"), (y, "b"), (x, "c")]
    assert both.filter(bank, 1, "MS", msgs) == [(y, "b")] and both.filter(bank, 0, 1, msgs) == msgs
    assert both.filter(bank, 2, "MS", msgs) == []


# ---- blob and validator --------------------------------------------------------------------------------
def test_blob_layout_and_validator(bank):
    rp = ReceiverProfiles([Profile(), Profile(whitelist=["7", "61"]), Profile(skip_development=True)], [0, 2, 1, 1, 0])
    blob = rp.blob(bank)
    h = struct.unpack_from("<12I", blob)
    assert h == (PF.MAGIC, PF.VERSION, len(blob), 3, 5, 129, 66, 12, 19, 0, 0, 0) and len(blob) % 16 == 0
    assert len(blob) == (48 + 3 * 128 + 5 + 15) // 16 * 16
    assert np.frombuffer(blob, "<u8", 48, 48).reshape(3, 4, 4).tolist() == rp.masks(bank).tolist()
    assert blob[48 + 384: 48 + 384 + 5] == bytes([0, 2, 1, 1, 0]) and not any(blob[48 + 384 + 5:])
    assert runtime.profile_check(blob) is None

    def damaged(off, data):
        b = bytearray(blob)
        b[off: off + len(data)] = data
        return runtime.profile_check(bytes(b))

    for cut in (0, 47, 48, 48 + 128, 48 + 384, len(blob) - 16, len(blob) - 1):
        assert runtime.profile_check(blob[:cut]) is not None, cut
        if cut >= 48:
            b = bytearray(blob[:cut])
            struct.pack_into("<I", b, 8, cut)
            assert runtime.profile_check(bytes(b)) is not None, cut
    m_mc = 48 + 2 * 32                                            # profile 0, kind MC: 12 classes
    assert "mask bit" in damaged(m_mc + 1, bytes([0x1F]))         # bit 12
    assert damaged(m_mc + 1, bytes([0x0F])) is None
    assert "mask bit" in damaged(48 + 128 + 31, bytes([0x80]))    # profile 1, MU, bit 255
    assert "mask bit" in damaged(48 + 2 * 128 + 32 + 8, bytes([4]))   # profile 2, MS, bit 66
    assert "of_source" in damaged(48 + 384 + 4, bytes([3]))       # = P
    assert "mask bit" in damaged(20, struct.pack("<I", 128))      # the counts of another bank: MU bit 128 beyond them
    assert damaged(20, struct.pack("<I", 257)) is not None
    assert damaged(0, b"XXXX") is not None and damaged(4, struct.pack("<I", 2)) is not None
    assert damaged(12, struct.pack("<I", 0)) is not None and damaged(12, struct.pack("<I", 65)) is not None
    assert damaged(16, struct.pack("<I", 0)) is not None and damaged(16, struct.pack("<I", 4097)) is not None
    assert damaged(len(blob) - 1, b"\x01") is not None            # padding
    # the largest table
    big = ReceiverProfiles([Profile()] * 64, [63] * 4096).blob(bank)
    assert len(big) == 48 + 64 * 128 + 4096 and runtime.profile_check(big) is None


def test_abi_declares_the_profile_entries():
    hdr = open(os.path.join(ROOT, "include", "sdx.h")).read()
    for name in ("sdx_profile_table_create", "sdx_profile_table_destroy", "sdx_profile_scratch_bytes", "sdx_filter_records",
                 "sdx_profile_check"):
        assert name in runtime.EXPORTED and re.search(r"\b%s\(" % name, hdr), name
    assert "#define SDX_ABI_VERSION 14" in hdr and runtime.ABI_VERSION == 14     # only new entries: the version stays
    lib = runtime.load_library()
    assert lib.sdx_abi_version() == 14
    assert lib.sdx_profile_scratch_bytes(0, 10) == 0 and lib.sdx_profile_scratch_bytes(5, 10) == 0
    assert lib.sdx_profile_scratch_bytes(1, -1) == 0
    a, b = lib.sdx_profile_scratch_bytes(1, 65537), lib.sdx_profile_scratch_bytes(4, 65537)
    assert a >= 8 * 65537 + 4 * 257 and b >= 4 * (a - 16) and a % 16 == 0 and lib.sdx_profile_scratch_bytes(1, 0) > 0
    lay = open(os.path.join(runtime.HERE, "csrc", "sdx_profile_layout.h")).read()
    for name, val in (("SDX_PROFILE_MAGIC", "0x%08Xu" % PF.MAGIC), ("SDX_PROFILE_VERSION", "%du" % PF.VERSION),
                      ("SDX_PROFILE_MAX", str(PF.PROFILES_MAX)), ("SDX_PROFILE_SOURCES_MAX", str(PF.SOURCES_MAX)),
                      ("SDX_PROFILE_CLASS_MAX", str(PF.CLASS_MAX))):
        assert re.search(r"#define %s %s\s" % (name, re.escape(val)), lay), name
    assert PF.SOURCES_MAX == runtime.REPEAT_SOURCES_MAX
    from pysignalduino_amd import build
    assert any(s.endswith("sdx_profile.hip") for s in build.SRCS) and any(d.endswith("sdx_profile_layout.h") for d in build.DEPS)


def test_blob_validator_under_sanitizers(tmp_path, bank):
    """tools/profile_blob_check.cpp: sdx_profile_validate over good blobs and systematically damaged ones as a
    stand-alone host program built with -fsanitize=address,undefined."""
    src = os.path.join(ROOT, "tools", "profile_blob_check.cpp")
    exe = str(tmp_path / "profile_blob_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    src, "-o", exe], check=True)
    tables = {"one": ReceiverProfiles([Profile()]),
              "four": ReceiverProfiles([Profile(whitelist=["7", "61", "72.1"]), Profile(blacklist=[61, 15]),
                                        Profile(skip_development=True), Profile(rfmode="PCA301")], [0, 1, 2, 3, 3, 0, 1]),
              "full": ReceiverProfiles([Profile()] * 64, [i % 64 for i in range(4096)])}
    for name, rp in tables.items():
        blob = tmp_path / (name + ".blob")
        blob.write_bytes(rp.blob(bank))
        r = subprocess.run([exe, str(blob)], capture_output=True, text=True)
        assert r.returncode == 0 and "profile_blob_check: ok" in r.stdout, (name, r.stdout, r.stderr[-2000:])
    bad = tmp_path / "bad.blob"
    bad.write_bytes(b"\0" * 64)
    assert subprocess.run([exe, str(bad)], capture_output=True).returncode != 0      # the program does refuse


# ---- a filtered list stands for a restricted bank ------------------------------------------------------
def golden_profiles(golden):
    """Profiles A (a whitelist of every second decoded id, by float(id)), B (a blacklist), C (skip_development)."""
    ids = sorted({m[0] for c in golden("lines_golden.json.gz") for m in c.get("e2e") or []}, key=float)
    return [dict(whitelist=ids[::2]), dict(blacklist=["61", "15", "1", "40", "113"]), dict(skip_development=True)], ids


def test_lines_golden_figures(golden, obank):
    cases = golden("lines_golden.json.gz")
    assert len(cases) == 4169 and sum("e2e_raise" in c for c in cases) == 0     # no line raises in the reference
    lists = [c["e2e"] for c in cases if c.get("e2e")]
    assert sum(len(x) >= 2 for x in lists) == 536
    ids = {m[0] for x in lists for m in x}
    assert len(ids) == 104 and len(ids & DEVELOP) == 5


def _results(res):
    return [[r["protocol_id"], r["payload"], r["meta"]["bit_length"], r["meta"]["rssi"], r["meta"]["clock"]] for r in res]


@pytest.mark.parametrize("kind,fname", [("MU", "mu_golden.json.gz"), ("MS", "ms_golden.json.gz")])
def test_restricted_bank_equals_filtered_list(golden, obank, kind, fname):
    kd = PF.KIND_NAMES.index(kind)
    profs, _ = golden_profiles(golden)
    P = obank.p
    n_cmp = n_changed = 0
    for kw in profs:
        small = O.OracleBank({pid: p for pid, p in P.items() if restate_enabled(P, pid, kd, **kw)})
        assert 0 < len(small.p) < len(P)
        for c in golden(fname):
            if "results" not in c["exp"] or not c["exp"]["results"]:
                continue     # the full call raises (the line stays raised), or decodes nothing (nothing to filter)
            exp = restate_filter(P, kd, c["exp"]["results"], **kw)
            got = _results(O.demod(small, dict(c["msg"]), kind))
            assert got == exp, (kw, c["src"], c["msg"])
            n_cmp += 1
            n_changed += exp != c["exp"]["results"]
    assert n_cmp > 500 and n_changed > 50, (n_cmp, n_changed)


def test_mn_rfmode_equals_filtered_list(golden, obank):
    g = golden("mn_golden.json.gz")
    P = obank.p
    modes = sorted({p["rfmode"] for p in P.values() if "modulation" in p and p.get("rfmode")})
    n_cmp = n_kept = 0
    seen = set()
    for src, line, rf, exp in g["lines"]:
        if rf is not None or src not in ("test", "synth") or line in seen or not exp.get("out"):
            continue
        seen.add(line)
        r = LO.parse_line(line.encode("latin-1"))
        if r["status"] != LO.OK or r["kind"] != LO.MN:
            continue
        args = (r["data"].decode("ascii"), M.rssi_of(r["R"]), M.afc_of(r["F"]))
        full = M.mn_parse(obank, *args, None)
        assert [m[0] for m in full] == [m[0] for m in exp["out"]]
        for mode in modes + ["NoSuchMode"]:
            want = restate_filter(P, 3, full, rfmode=mode)
            assert M.mn_parse(obank, *args, mode) == want, (line, mode)
            n_cmp += 1
            n_kept += bool(want)
    assert n_cmp > 2000 and n_kept > 100, (n_cmp, n_kept)
