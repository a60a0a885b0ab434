"""Dispatch rules: every message of a line, repeats reduced as FHEM's dispatch stage does.

One line often carries a telegram several times, and the reference's demodulators return every match.  FHEM
dispatches every message of such a list, but stops after ``maxMuMsgRepeat`` (4) messages of one protocol and drops
a message equal to the one just dispatched, unless the protocol carries ``dispatchequals``.

``DispatchRules(max_repeat=4, drop_equal=True, keep_equal="bank")`` on one line's list r_0 .. r_{m-1} of one kind,
in the reference's order:

    run = 0; prev_proto = none; last = none
    for j in 0 .. m-1:
        run = run + 1 if proto(r_j) == prev_proto else 1;  prev_proto = proto(r_j)
        if max_repeat > 0 and run > max_repeat:  drop r_j          # does not become ``last``
        else:
            eq = last exists and proto(r_j) == proto(last) and payload(r_j) == payload(last)
            last = r_j
            drop r_j if drop_equal and eq and proto(r_j) not in keep_equal, keep it otherwise

``max_repeat=0``: no cap.  ``keep_equal``: an iterable of protocol ids (compared as ``str(id)``), or "bank" for
the ids whose protocol has ``dispatchequals == "true"``.  The key is (protocol, payload), DESIGN.md §4k's key
inside one kind; ``bit_length`` and the metadata are not part of it.  r_0 is always kept; the reduction is
idempotent.

``DispatchRules.struct`` fills the ``sdx_dispatch_rules`` that ``sdx_dispatch_records`` takes (include/sdx.h);
``DispatchRules.reduce`` is the definition on the host, for every path that builds a line's messages without the
device records.
"""
from __future__ import annotations

from typing import Iterable, List, Union

from .profiles import CLASS_MAX, KIND_NAMES, class_lists


def _pid(m) -> str:
    return str(m.protocol_id if hasattr(m, "protocol_id") else m[0])


def _payload(m):
    return m.payload if hasattr(m, "payload") else m[1]


class DispatchRules:
    """See the module text.  Immutable once built; compiled per bank on demand."""

    def __init__(self, max_repeat: int = 4, drop_equal: bool = True, keep_equal: Union[str, Iterable] = "bank"):
        if isinstance(max_repeat, bool) or not isinstance(max_repeat, int) or not 0 <= max_repeat < 1 << 31:
            raise ValueError(f"max_repeat: an integer >= 0 (0 = no cap), not {max_repeat!r}")
        if isinstance(keep_equal, str):
            if keep_equal != "bank":
                raise ValueError(f'keep_equal: "bank" or a list of protocol ids, not {keep_equal!r}')
        elif isinstance(keep_equal, (bytes, int, float)) or keep_equal is None:
            raise ValueError(f'keep_equal: "bank" or a list of protocol ids, not {keep_equal!r}')
        else:
            keep_equal = frozenset(str(i) for i in keep_equal)
        self.max_repeat, self.drop_equal, self.keep_equal = max_repeat, bool(drop_equal), keep_equal
        self._compiled = {}

    def __repr__(self):
        keep = self.keep_equal if isinstance(self.keep_equal, str) else sorted(self.keep_equal)
        return f"DispatchRules(max_repeat={self.max_repeat}, drop_equal={self.drop_equal}, keep_equal={keep!r})"

    def keep_ids(self, bank) -> frozenset:
        """The protocol ids (str) exempt from the equal-message drop; ValueError for an id the bank does not know."""
        c = self._compiled.get(id(bank))
        if c is None or c[0] is not bank:
            if self.keep_equal == "bank":
                ids = frozenset(str(pid) for pid, p in bank.protocols.items() if p.get("dispatchequals") == "true")
            else:
                known = {str(p) for p in bank.protocols}
                for pid in self.keep_equal:
                    if pid not in known:
                        raise ValueError(f"dispatch rules: the bank has no protocol id {pid!r}")
                ids = self.keep_equal
            if max(len(x) for x in class_lists(bank)) > CLASS_MAX:
                raise ValueError(f"dispatch rules: a kind of the bank has more than {CLASS_MAX} classes")
            c = (bank, ids)
            self._compiled[id(bank)] = c
        return c[1]

    def masks(self, bank) -> List[List[int]]:
        """[kind][word]: bit c of the kind's 256 = class c (sdx_result.proto) is exempt from the equal-message drop."""
        ids = self.keep_ids(bank)
        out = [[0, 0, 0, 0] for _ in range(4)]
        for kd, pids in enumerate(class_lists(bank)):
            for ci, pid in enumerate(pids):
                if str(pid) in ids:
                    out[kd][ci >> 6] |= 1 << (ci & 63)
        return out

    def struct(self, bank):
        """The rules as ``sdx_dispatch_records`` takes them: a runtime.SdxDispatchRules."""
        from .runtime import SdxDispatchRules
        s = SdxDispatchRules()
        for kd, words in enumerate(self.masks(bank)):
            for w, v in enumerate(words):
                s.keep_equal[kd][w] = v
            s.max_repeat[kd] = self.max_repeat
        s.drop_equal = 1 if self.drop_equal else 0
        s.res = 0
        return s

    def reduce(self, bank, kind_name, messages: list) -> list:
        """The definition on the host: the messages (objects with ``protocol_id`` / ``payload``, or
        (protocol_id, payload, ...) tuples) of one line of kind ``kind_name`` ("MU" .. "MN" or 0 .. 3) that the rules
        keep, in order.  The kind only names the list; the ids are the key."""
        if isinstance(kind_name, str):
            if kind_name not in KIND_NAMES:
                raise ValueError(f"kind: one of {KIND_NAMES}, not {kind_name!r}")
        elif not 0 <= int(kind_name) < 4:
            raise ValueError(f"kind: 0 .. 3, not {kind_name!r}")
        keep_ids = self.keep_ids(bank)
        out, run, prev, last = [], 0, None, None
        for m in messages:
            pid = _pid(m)
            run = run + 1 if pid == prev else 1
            prev = pid
            if self.max_repeat > 0 and run > self.max_repeat:
                continue
            key = (pid, _payload(m))
            eq = last is not None and key == last
            last = key
            if not (self.drop_equal and eq and pid not in keep_ids):
                out.append(m)
        return out


def as_rules(x):
    """None, a DispatchRules, or True (the defaults: cap 4, equal-drop, the bank's dispatchequals)."""
    if x is None or isinstance(x, DispatchRules):
        return x
    if x is True:
        return DispatchRules()
    raise ValueError(f"dispatch: None, True or a DispatchRules, not {x!r}")
