"""Repeat suppression, host side.

The definition, in line order within one stream of lines (one LineStream, or one parse_lines* /
parse_bytes* call): a line is RESULT-BEARING when the reference's parse_line returns a non-empty list
for it; its KEY is (kind, protocol, payload) of ``decoded[0]``, the message the controller publishes
(signalduino/controller.py:252-257); it is a REPEAT when its key equals the key of the previous
result-bearing line.  Lines without results -- noise, ignored lines, a ContractError slot, ``[]`` --
neither start nor break a run.  There is no time-based expiry.

The device decides this for the lines it demodulates (sdx_mark_repeats, csrc/sdx_repeat.hip).  Lines the
batch API resolves on the host (the general path, lines outside the contract, re-runs after an
overflow) are invisible to it, so around them its mask can be wrong: :class:`RepeatTracker` re-decides
exactly those places and carries the last key from chunk to chunk.  Host keys name the protocol by its
id, device keys by its table index; inside one kind the two correspond one to one (bank.py).
"""
from __future__ import annotations

import json
from typing import Callable, Dict, Iterable, Optional, Tuple

import numpy as np

Key = Tuple[str, str, str]   # (kind name, protocol_id, payload)


class _Unknown:
    def __repr__(self) -> str:   # pragma: no cover
        return "UNKNOWN"


UNKNOWN = _Unknown()   # the device's carried key after lines it may or may not have seen results for


def text_key(kind_name: str, text: str) -> Key:
    """The key of a line from the JSON text published for it."""
    d = json.loads(text)
    return (kind_name, str(d["protocol_id"]), d["payload"])


def objects_key(msgs) -> Optional[Key]:
    """The key of a line from parse_lines' slot: None unless it is a non-empty DecodedMessage list."""
    if not isinstance(msgs, list) or not msgs:
        return None
    m = msgs[0]
    return (str(m.raw.message_type), str(m.protocol_id), m.payload)


def collapse_objects(out: list) -> np.ndarray:
    """parse_lines' list with every repeat's slot replaced by [] (in place) -> the mask uint8[n]."""
    mask = np.zeros(len(out), np.uint8)
    prev = None
    for i, msgs in enumerate(out):
        k = objects_key(msgs)
        if k is None:
            continue
        if k == prev:
            mask[i] = 1
            out[i] = []
        prev = k
    return mask


class RepeatTracker:
    """One stream's carried keys: ``true_key`` of the last result-bearing line by the definition,
    ``dev_key`` of the last one the device saw (what its state buffer holds)."""

    def __init__(self):
        self.true_key: Optional[Key] = None
        self.dev_key = None

    def fix_chunk(self, rep: np.ndarray, has_key: np.ndarray, dev_key_of: Callable[[int], Key],
                  host_keys: Dict[int, Optional[Key]], redo: Iterable[int] = (),
                  fetch_key: Optional[Callable[[int], Optional[Key]]] = None, end_key=None) -> np.ndarray:
        """The exact mask of a chunk.  ``rep``: the device's mask; ``has_key[i]``: dev_key_of(i) can give
        line i's key from what came back (its text, its wire records) -- a device line is
        result-bearing when has_key or rep is set; ``host_keys``: the host-resolved rows -> their key,
        None for a row without results; ``redo``: those of them the device may have seen results for
        (re-runs after an overflow); ``fetch_key(i)``: line i's key through the batch API, for a line
        the device flagged whose predecessor's key the host does not know; ``end_key``: the key the
        device's state holds after this chunk, when the caller read it back (spares looking it up)."""
        n = len(rep)
        mask = np.array(rep, np.uint8, copy=True)
        rb = np.asarray(has_key, bool) | (mask != 0)
        hrows = sorted(host_keys)
        if hrows:
            rb[hrows] = False
            mask[hrows] = 0
        redo = set(redo)
        a = 0
        for h in hrows + [n]:
            self._device_segment(a, h, mask, rb, has_key, dev_key_of, fetch_key, end_key if h == n else None)
            if h == n:
                break
            k = host_keys[h]
            if k is not None:
                if k == self.true_key:
                    mask[h] = 1
                self.true_key = k
            if h in redo:
                self.dev_key = UNKNOWN
            a = h + 1
        return mask

    def _device_segment(self, a, b, mask, rb, has_key, dev_key_of, fetch_key, end_key=None) -> None:
        idx = np.flatnonzero(rb[a:b]) + a
        if not len(idx):
            return
        if self.dev_key is UNKNOWN or self.dev_key != self.true_key:
            # the device compared the segment's first result-bearing line with another key than the
            # definition's predecessor: decide it again
            r0 = int(idx[0])
            if has_key[r0]:
                k = dev_key_of(r0)
            else:   # flagged: the key of the device's predecessor
                k = self.dev_key
                if k is UNKNOWN or k is None:
                    if fetch_key is None:
                        raise RuntimeError(f"line {r0}: a flagged line whose key is unknown and no fetch_key")
                    k = fetch_key(r0)
            mask[r0] = 1 if (k is not None and k == self.true_key) else 0
            self.true_key = self.dev_key = k
        # the rest of the segment compares with device lines the host agrees on: the key at its end is
        # that of its last line with a key (the flagged lines after it repeat it)
        if end_key is not None:
            self.true_key = self.dev_key = end_key
            return
        keyed = idx[np.asarray(has_key, bool)[idx]]
        if len(keyed):
            self.true_key = self.dev_key = dev_key_of(int(keyed[-1]))
