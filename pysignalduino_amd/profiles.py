"""Receiver profiles: per-source protocol lists and rfmode.

A stream of lines merges several receivers; every line carries its source id.  A ``Profile`` is what a FHEM
user sets per stick: ``whitelist_IDs``, ``blacklist_IDs``, whether ``developId`` protocols run, and the
``rfmode`` of an FSK stick.  ``ReceiverProfiles`` maps every source id to one profile and compiles, against a
bank, the blob ``sdx_filter_records`` reads (csrc/sdx_profile_layout.h): per profile and kind a 256-bit mask
over the bank's class list (``bank.mu_pids`` / ``ms_pids`` / ``mc_pids`` / ``mn_pids``, what
``sdx_result.proto`` indexes), then ``of_source``.

A protocol id ``pid`` is enabled by ``Profile(whitelist, blacklist, rfmode, skip_development)`` when
  whitelist is None or pid in whitelist;  pid not in blacklist;
  not skip_development or "developId" not in P[pid] or (whitelist is not None and pid in whitelist);
  for MN only: rfmode is None or P[pid].get("rfmode") == rfmode.
Ids are compared as ``str(id)``.  The default ``Profile()`` enables everything (the reference's behaviour);
``skip_development=True`` is FHEM's default.

``ReceiverProfiles.filter`` is the definition on the host: a line's messages -> the ones its source's profile
enables, in order.  Every host path that builds a line's messages without the device records uses it.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

MAGIC = 0x46505853        # SDX_PROFILE_MAGIC "SXPF"
VERSION = 1               # SDX_PROFILE_VERSION
PROFILES_MAX = 64         # SDX_PROFILE_MAX
SOURCES_MAX = 4096        # SDX_PROFILE_SOURCES_MAX = SDX_REPEAT_SOURCES_MAX
CLASS_MAX = 256           # SDX_PROFILE_CLASS_MAX
HDR_FMT = "<12I"          # sdx_profile_hdr, 48 bytes
KIND_NAMES = ("MU", "MS", "MC", "MN")


def _ids(ids, what: str) -> Optional[frozenset]:
    if ids is None:
        return None
    if isinstance(ids, (str, bytes, int, float)):
        raise ValueError(f"{what}: a list of protocol ids, not {ids!r}")
    return frozenset(str(i) for i in ids)


@dataclass(frozen=True)
class Profile:
    """One receiver's configuration; see the module text for what it enables."""
    whitelist: Optional[Iterable] = None
    blacklist: Iterable = ()
    rfmode: Optional[str] = None
    skip_development: bool = False

    def __post_init__(self):
        object.__setattr__(self, "whitelist", _ids(self.whitelist, "whitelist"))
        object.__setattr__(self, "blacklist", _ids(self.blacklist, "blacklist") or frozenset())
        if self.rfmode is not None and not isinstance(self.rfmode, str):
            raise ValueError("rfmode: a string or None")

    def enables(self, protocols: dict, pid, kind: int) -> bool:
        """Is ``pid`` of ``kind`` (0 MU, 1 MS, 2 MC, 3 MN) enabled, by the definition."""
        pid = str(pid)
        p = protocols[pid]
        listed = self.whitelist is not None and pid in self.whitelist
        if self.whitelist is not None and not listed:
            return False
        if pid in self.blacklist:
            return False
        if self.skip_development and "developId" in p and not listed:
            return False
        if kind == 3 and self.rfmode is not None and p.get("rfmode") != self.rfmode:
            return False
        return True

    def compile(self, bank) -> List[List[int]]:
        """-> per kind the sorted class indices the profile enables; ValueError for an id the bank does not know."""
        known = {str(p) for p in bank.protocols}
        for ids in (self.whitelist or (), self.blacklist):
            for pid in ids:
                if pid not in known:
                    raise ValueError(f"profile: the bank has no protocol id {pid!r}")
        return [[c for c, pid in enumerate(pids) if self.enables(bank.protocols, pid, kd)]
                for kd, pids in enumerate(class_lists(bank))]


def class_lists(bank) -> Tuple[Sequence, Sequence, Sequence, Sequence]:
    return (bank.mu_pids, bank.ms_pids, bank.mc_pids, bank.mn_pids)


class ReceiverProfiles:
    """``profiles``: 1 to 64 Profile objects; ``of_source[s]``: the profile index of source id s (1 to 4,096
    sources).  ``of_source=None``: one source on profile 0."""

    def __init__(self, profiles: Sequence[Profile], of_source: Optional[Sequence[int]] = None):
        profiles = list(profiles)
        if not 1 <= len(profiles) <= PROFILES_MAX or not all(isinstance(p, Profile) for p in profiles):
            raise ValueError(f"profiles: 1 to {PROFILES_MAX} Profile objects")
        src = np.asarray([0] if of_source is None else of_source)
        if src.ndim != 1 or src.dtype.kind not in "iu" or not 1 <= len(src) <= SOURCES_MAX:
            raise ValueError(f"of_source: 1 to {SOURCES_MAX} integer profile indices")
        if int(src.min()) < 0 or int(src.max()) >= len(profiles):
            raise ValueError(f"of_source: every entry must be inside [0, {len(profiles)})")
        self.profiles = profiles
        self.of_source = src.astype(np.uint8)
        self._compiled = {}

    @property
    def n_sources(self) -> int:
        return len(self.of_source)

    @property
    def is_default(self) -> bool:
        """Does every profile enable everything (then the pass changes nothing but the records' order)."""
        return all(p == Profile() for p in self.profiles)

    def _for(self, bank):
        c = self._compiled.get(id(bank))
        if c is None or c[0] is not bank:
            counts = [len(x) for x in class_lists(bank)]
            if max(counts) > CLASS_MAX:
                raise ValueError(f"profiles: a kind of the bank has more than {CLASS_MAX} classes")
            enabled = [p.compile(bank) for p in self.profiles]
            masks = np.zeros((len(self.profiles), 4, 4), np.uint64)
            for pi, per_kind in enumerate(enabled):
                for kd, cls in enumerate(per_kind):
                    for ci in cls:
                        masks[pi, kd, ci >> 6] |= np.uint64(1) << np.uint64(ci & 63)
            pid_sets = [[frozenset(str(pids[ci]) for ci in cls) for cls, pids in zip(per_kind, class_lists(bank))]
                        for per_kind in enabled]
            c = (bank, counts, masks, pid_sets)
            self._compiled[id(bank)] = c
        return c

    def masks(self, bank) -> np.ndarray:
        """uint64[P][4][4]: bit c of [p][kind] = class c of the kind is enabled by profile p."""
        return self._for(bank)[2]

    def blob(self, bank) -> bytes:
        """The table as sdx_profile_table_create takes it (csrc/sdx_profile_layout.h)."""
        _, counts, masks, _ = self._for(bank)
        body = masks.astype("<u8").tobytes() + self.of_source.tobytes()
        total = (struct.calcsize(HDR_FMT) + len(body) + 15) & ~15
        hdr = struct.pack(HDR_FMT, MAGIC, VERSION, total, len(self.profiles), len(self.of_source), *counts, 0, 0, 0)
        return (hdr + body).ljust(total, b"\0")

    def mn_elig(self, bank) -> int:
        """The OR of the profiles' MN masks as sdx_mn_batch.elig takes it: an MN protocol no profile enables is
        never run (the host ANDs it with the parser's own rfmode eligibility)."""
        m = 0
        for w in self.masks(bank)[:, 3, 0]:
            m |= int(w)
        return m

    def enabled_ids(self, bank, source: int, kind) -> frozenset:
        """The protocol ids (str) of ``kind`` (0..3 or "MU".."MN") that ``source``'s profile enables; an id outside
        [0, n_sources) enables nothing."""
        kd = KIND_NAMES.index(kind) if isinstance(kind, str) else int(kind)
        if not 0 <= int(source) < len(self.of_source):
            return frozenset()
        return self._for(bank)[3][int(self.of_source[int(source)])][kd]

    def filter(self, bank, source: int, kind, messages: list) -> list:
        """The definition on the host: the messages (objects with ``protocol_id``, or (protocol_id, ...) tuples)
        of a line of ``source`` and ``kind`` that the source's profile enables, in order."""
        on = self.enabled_ids(bank, source, kind)
        return [m for m in messages if str(m.protocol_id if hasattr(m, "protocol_id") else m[0]) in on]


def as_profiles(profiles) -> Optional[ReceiverProfiles]:
    """None, a ReceiverProfiles, a Profile (one source) or a list of Profile objects (one source on the first)."""
    if profiles is None or isinstance(profiles, ReceiverProfiles):
        return profiles
    if isinstance(profiles, Profile):
        return ReceiverProfiles([profiles])
    return ReceiverProfiles(profiles)
