"""Repeat suppression: the definition, the argument checks, the trackers that make the device's
mask exact around host-resolved rows, and :class:`RepeatPass`, which drives the device pass for stream and front end.

The definition, in line order within one stream of lines (one LineStream, or one parse_lines* /
parse_bytes* call): a line is RESULT-BEARING when the reference's parse_line returns a non-empty list
for it; its KEY is (kind, protocol, payload) of ``decoded[0]``, the message the controller publishes
(signalduino/controller.py:252-257); it is a REPEAT when its key equals the key of the previous
result-bearing line.  Lines without results -- noise, ignored lines, a ContractError slot, ``[]`` --
neither start nor break a run.

With a time window W (``repeat_window``, FHEM's dispatch rule: a telegram is dispatched again when it
differs from the last one or more than 2 s have passed since the last one dispatched) every line has an
arrival time, non-decreasing over the stream, and the stream carries (K, T): K the key of the previous
result-bearing line, T the time of the last result-bearing line that was NOT marked.  A result-bearing
line with key k and time t is a repeat when K exists, k == K and t - T <= W; otherwise it is published
and T = t; K = k in both cases.  The anchor is the last published line, not the predecessor: with times
0 s, 1.5 s, 2.5 s of one key and W = 2 s the third line is published.  Times are int64 microseconds;
``repeat_window`` is given in seconds and becomes ``window_to_us(repeat_window)``.  Without a window
there is no time-based expiry.

A stream that merges several receivers gives every line a source id (``sources``, 0 <= id < S <= 4096): for
each source the subsequence of lines with that id is a stream of its own by the two definitions above, with
its own (K, T); lines of other sources neither start, break nor time out a run, and the times are
non-decreasing within a source only (sdx_mark_repeats_by_source; :class:`SourceTrackers` on the host).

The device decides this for the lines it demodulates (sdx_mark_repeats, with a window
sdx_mark_repeats_timed; csrc/sdx_repeat.hip).  Lines the
batch API resolves on the host (the general path, lines outside the contract, re-runs after an
overflow) are invisible to it, so around them its mask can be wrong: :class:`RepeatTracker` re-decides
exactly those places and carries the last key -- with a window (K, T) -- from chunk to chunk.  Host keys name the protocol by its
id, device keys by its table index; inside one kind the two correspond one to one (bank.py).
"""
from __future__ import annotations

import json
from types import SimpleNamespace
from typing import Callable, Dict, Iterable, Optional, Tuple

import numpy as np

from . import runtime

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


def window_to_us(repeat_window) -> Optional[int]:
    """``repeat_window`` in seconds -> W in microseconds (None stays None)."""
    if repeat_window is None:
        return None
    w = int(round(float(repeat_window) * 1e6))
    if w < 0:
        raise ValueError("repeat_window must not be negative")
    return w


SOURCES_MAX = 4096   # SDX_REPEAT_SOURCES_MAX


def check_sources(sources, n: int, n_sources: Optional[int] = None) -> np.ndarray:
    """One call's or chunk's source ids as int32[n]; ValueError unless there are n integers inside
    [0, n_sources).  ``n_sources`` None (a one-shot call): the largest id + 1, at most SOURCES_MAX."""
    if sources is None:
        raise ValueError("the lines' source ids are missing (sources=)")
    s = np.asarray(sources)
    if s.dtype.kind not in "iu" or s.ndim != 1:
        raise ValueError("sources: one integer id per line")
    if len(s) != n:
        raise ValueError(f"sources: {len(s)} ids for {n} lines")
    top = SOURCES_MAX if n_sources is None else int(n_sources)
    if n and (int(s.min()) < 0 or int(s.max()) >= top):
        raise ValueError(f"sources: ids must be inside [0, {top})")
    return s.astype(np.int32, copy=False)


def count_sources(sources: np.ndarray) -> int:
    """S of a one-shot call: the largest id + 1."""
    return int(sources.max()) + 1 if len(sources) else 1


def by_source(sources: np.ndarray):
    """-> [(source id, the indices of its lines in line order)] for the ids present, in id order."""
    order = np.argsort(sources, kind="stable")
    ss = sources[order]
    cuts = np.flatnonzero(ss[1:] != ss[:-1]) + 1
    return [(int(sources[g[0]]), g) for g in np.split(order, cuts)] if len(order) else []


def check_times(times, n: int, last=None, sources: Optional[np.ndarray] = None) -> np.ndarray:
    """One call's or chunk's arrival times as int64[n]; ValueError unless there are n of them, they do not
    decrease, and the first is not earlier than ``last`` (the previous chunk's last time).  With ``sources``
    (check_sources' array) all of this holds within each source, not over the merged lines, and ``last`` is
    a dict source -> that source's last time."""
    if times is None:
        raise ValueError("a repeat window needs the lines' arrival times (times=)")
    t = np.asarray(times)
    if t.dtype.kind not in "iu" or t.ndim != 1:
        raise ValueError("times: one integer (microseconds) per line")
    t = t.astype(np.int64, copy=False)   # an int64 array is taken as it is: the caller keeps it unchanged
    if len(t) != n:
        raise ValueError(f"times: {len(t)} times for {n} lines")
    if sources is not None:
        order = np.argsort(sources, kind="stable")
        ts, ss = t[order], sources[order]
        if n and bool(((ts[1:] < ts[:-1]) & (ss[1:] == ss[:-1])).any()):
            raise ValueError("times must not decrease over a source's lines")
        if n and last:
            first = np.concatenate([[True], ss[1:] != ss[:-1]])
            for sid, t0 in zip(ss[first].tolist(), ts[first].tolist()):
                if last.get(sid) is not None and t0 < last[sid]:
                    raise ValueError("times must not decrease over a source's lines")
        return t
    if n and (bool((t[1:] < t[:-1]).any()) or (last is not None and int(t[0]) < last)):
        raise ValueError("times must not decrease over a stream's lines")
    return t


def collapse_objects(out: list, times=None, window_us: Optional[int] = None, carry: Optional[list] = None,
                     sources=None) -> np.ndarray:
    """parse_lines' list with every repeat's slot replaced by [] (in place) -> the mask uint8[n].
    ``window_us``: the time window W with the lines' ``times`` (microseconds); None: no expiry.
    ``carry``: [K, T, last time] of the stream so far ([None, 0, None] starts one), updated in place: the
    call continues that stream instead of starting one.  ``sources``: one source id per line; every
    source's lines are a stream of their own, and ``carry`` is a dict source -> [K, T, last time]."""
    if sources is not None:
        src = check_sources(sources, len(out))
        if window_us is not None:
            times = check_times(times, len(out), {s: c[2] for s, c in (carry or {}).items()}, src)
        mask = np.zeros(len(out), np.uint8)
        for sid, idx in by_source(src):
            sub = [out[i] for i in idx]
            c = carry.setdefault(sid, [None, 0, None]) if carry is not None else None
            mask[idx] = collapse_objects(sub, None if window_us is None else times[idx], window_us, c)
            for i, x in zip(idx.tolist(), sub):
                out[i] = x
        return mask
    if window_us is not None:
        times = check_times(times, len(out), carry[2] if carry else None).tolist()
    mask = np.zeros(len(out), np.uint8)
    prev, anchor = (carry[0], carry[1]) if carry else (None, 0)
    for i, msgs in enumerate(out):
        k = objects_key(msgs)
        if k is None:
            continue
        if k == prev and (window_us is None or times[i] - anchor <= window_us):
            mask[i] = 1
            out[i] = []
        elif window_us is not None:
            anchor = times[i]
        prev = k
    if carry:
        carry[:] = [prev, anchor, times[-1] if window_us is not None and len(out) else carry[2]]
    return mask


class RepeatTracker:
    """One stream's carried keys: ``true_key`` of the last result-bearing line by the definition,
    ``dev_key`` of the last one the device saw (what its state buffer holds).  With a window
    (fix_chunk's ``times`` / ``window_us``) ``true_t`` and ``dev_t`` carry T beside them: the time of the
    last line published by the definition, and of the last one the device left unmarked."""

    def __init__(self):
        self.true_key: Optional[Key] = None
        self.dev_key = None
        self.true_t = self.dev_t = 0

    def fix_chunk(self, rep: np.ndarray, has_key: np.ndarray, dev_key_of: Callable[[int], Key],
                  host_keys: Dict[int, Optional[Key]], redo: Iterable[int] = (),
                  fetch_key: Optional[Callable[[int], Optional[Key]]] = None, end_key=None,
                  times=None, window_us: Optional[int] = None) -> np.ndarray:
        """The exact mask of a chunk.  ``rep``: the device's mask; ``has_key[i]``: dev_key_of(i) can give
        line i's key from what came back (its text, its wire records) -- a device line is
        result-bearing when has_key or rep is set; ``host_keys``: the host-resolved rows -> their key,
        None for a row without results; ``redo``: those of them the device may have seen results for
        (re-runs after an overflow); ``fetch_key(i)``: line i's key through the batch API, for a line
        the device flagged whose predecessor's key the host does not know; ``end_key``: the key the
        device's state holds after this chunk, when the caller read it back (spares looking it up);
        ``times`` / ``window_us``: the chunk's arrival times and W, when the device ran the timed pass."""
        if window_us is not None:
            return self._fix_timed(rep, has_key, dev_key_of, host_keys, set(redo), fetch_key, times, window_us)
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

    def _fix_timed(self, rep, has_key, dev_key_of, host_keys, redo, fetch_key, times, w) -> np.ndarray:
        """fix_chunk with a window.  While the definition and the device hold the same (K, T) the device's
        mask is exact and whole stretches are taken as they are.  From a host-resolved row on the lines are
        re-decided one by one, the device's (K, T) followed beside the definition's, until both hold the
        same again -- at the latest at the next line that both publish: there both hold (that key, that
        time).  A line the device marked has its device predecessor's key."""
        n = len(rep)
        t = np.asarray(times)           # checked where the chunk was submitted (check_times)
        mask = np.array(rep, np.uint8, copy=True)
        has_key = np.asarray(has_key, bool)
        hrows = sorted(host_keys)
        if not hrows and self.dev_key is not UNKNOWN and (self.dev_key, self.dev_t) == (self.true_key, self.true_t):
            # the common chunk: no host row, both sides agree -- the device's mask is exact; K is the last
            # keyed line's key, T the last unmarked result-bearing line's time (searched from the end)
            i = n - 1 - int(has_key[::-1].argmax()) if n else 0
            if n and has_key[i]:
                self.true_key = self.dev_key = dev_key_of(i)
                pub = has_key & (mask == 0)
                j = n - 1 - int(pub[::-1].argmax())
                if pub[j]:
                    self.true_t = self.dev_t = int(t[j])
            return mask
        rb = has_key | (mask != 0)
        ishost = np.zeros(n, bool)
        if hrows:
            ishost[hrows] = True
            rb[hrows] = False
            mask[hrows] = 0
        ev = np.flatnonzero(rb | ishost)      # the lines that can carry a result, in line order
        hpos = np.searchsorted(ev, hrows)     # where the host rows stand among them
        p, nh = 0, 0
        while p < len(ev):
            if self.dev_key is not UNKNOWN and (self.dev_key, self.dev_t) == (self.true_key, self.true_t):
                while nh < len(hpos) and hpos[nh] < p:
                    nh += 1
                q = int(hpos[nh]) if nh < len(hpos) else len(ev)
                if q > p:   # device lines in agreement: K = the last keyed line's, T = the last unmarked line's
                    span = ev[p:q]
                    keyed = span[has_key[span]]
                    if len(keyed):
                        self.true_key = self.dev_key = dev_key_of(int(keyed[-1]))
                    pub = span[mask[span] == 0]
                    if len(pub):
                        self.true_t = self.dev_t = int(t[pub[-1]])
                    p = q
                    continue
            i = int(ev[p])
            p += 1
            if ishost[i]:
                k = host_keys[i]
                if i in redo:   # the device may have seen a result here: what it holds is not known
                    self.dev_key = self.dev_t = UNKNOWN
            else:
                if has_key[i]:
                    k = dev_key_of(i)
                else:       # marked by the device, no text: the key of the device's predecessor
                    k = self.dev_key
                    if k is UNKNOWN or k is None:
                        if fetch_key is None:
                            raise RuntimeError(f"line {i}: a flagged line whose key is unknown and no fetch_key")
                        k = fetch_key(i)
                if k is not None:
                    self.dev_key = k
                    if not rep[i]:
                        self.dev_t = int(t[i])
            if k is None:
                continue
            if self.true_key is not None and k == self.true_key and int(t[i]) - self.true_t <= w:
                mask[i] = 1
            else:
                mask[i] = 0
                self.true_t = int(t[i])
            self.true_key = k
        return mask


class SourceTrackers:
    """One RepeatTracker per source id of a stream that merges several receivers: every source's lines of a
    chunk are that source's stream, so the repair around host-resolved rows runs over each source's
    subsequence of the chunk with the source's own carried keys."""

    def __init__(self):
        self.trackers: Dict[int, RepeatTracker] = {}

    def fix_chunk(self, sources: np.ndarray, rep: np.ndarray, has_key: np.ndarray, dev_key_of: Callable[[int], Key],
                  host_keys: Dict[int, Optional[Key]], redo: Iterable[int] = (),
                  fetch_key: Optional[Callable[[int], Optional[Key]]] = None, table=None,
                  times=None, window_us: Optional[int] = None) -> np.ndarray:
        """RepeatTracker.fix_chunk per source -> the chunk's exact mask.  ``sources``: int32[n], the lines'
        ids; ``table``: the compact per-source table the device left behind this chunk
        (runtime.REPEAT_SOURCE_ENTRY per source): its ``last`` names the source's last result-bearing device
        line, whose key is the one the source's slot holds; the other arguments as RepeatTracker.fix_chunk,
        by line index of the chunk."""
        rep = np.asarray(rep)
        has_key = np.asarray(has_key, bool)
        mask = np.array(rep, np.uint8, copy=True)
        redo = set(redo)
        t = None if window_us is None else np.asarray(times)
        hrows = np.fromiter(host_keys, np.int64, len(host_keys))
        hsrc = set(sources[hrows].tolist()) if len(hrows) else set()
        for sid, idx in by_source(np.asarray(sources)):
            tr = self.trackers.get(sid)
            if tr is None:
                tr = self.trackers[sid] = RepeatTracker()
            pos = None
            if sid in hsrc:   # chunk index -> index inside the source's subsequence, for its host rows
                pos = {int(g): j for j, g in enumerate(idx.tolist()) if g in host_keys}
            hk = {j: host_keys[g] for g, j in pos.items()} if pos else {}
            rd = [j for g, j in pos.items() if g in redo] if pos else []
            at = idx.tolist()
            end_key = None
            if window_us is None and table is not None and not hk:
                last = int(table[sid]["last"])
                if 0 <= last < len(rep) and has_key[last]:
                    end_key = dev_key_of(last)
            mask[idx] = tr.fix_chunk(rep[idx], has_key[idx], lambda j: dev_key_of(at[j]), hk, rd,
                                     None if fetch_key is None else (lambda j: fetch_key(at[j])), end_key,
                                     **({} if window_us is None else {"times": t[idx], "window_us": window_us}))
        return mask


def apply_mask(mask, rep, host_keys, drop: Callable[[int], None], republish: Callable[[int], None]) -> None:
    """A chunk's published lines follow the exact ``mask`` where it differs from the device's (``rep``, by which
    it skipped texts) and on the host rows (``host_keys``): ``drop(i)`` for a repeat that was published -- a host
    row, or a device line behind one --, ``republish(i)`` for a line the device skipped behind a host row."""
    for i in sorted(set(np.nonzero(mask != rep)[0].tolist()) | set(host_keys)):
        if mask[i]:
            drop(i)
        elif i not in host_keys and rep[i]:
            republish(i)


STATE_HEAD = 16 + 240   # bytes of the untimed state read back per chunk: its header + a payload of up to 240 bytes
_KINDS = ("MU", "MS", "MC", "MN")   # enum sdx_kind


class RepeatPass:
    """The device pass of one stream of lines and the tracker that makes its mask exact -- the only place that
    knows which of the three modes runs: plain (sdx_mark_repeats), ``window_us`` (sdx_mark_repeats_timed),
    ``n_sources`` with or without a window (sdx_mark_repeats_by_source).  It owns the carried device state
    (allocated with the first chunk buffers) and the RepeatTracker / SourceTrackers that follow it."""

    def __init__(self, eng, window_us: Optional[int] = None, n_sources: Optional[int] = None):
        self.eng, self.window_us, self.n_sources = eng, window_us, n_sources
        self.tracker = SourceTrackers() if n_sources is not None else RepeatTracker()
        self.state = None

    def alloc(self, cap: int, pinned: bool) -> SimpleNamespace:
        """The buffers of one chunk of up to ``cap`` lines: ``mask`` (device uint8[cap]) and the mode's ``scratch``.
        ``pinned``: a stream's slot -- where the mode takes times / ids, device ``d_times`` / ``d_src`` beside
        their pinned host copies ``h_times`` / ``h_src``, and ``h_read``, the pinned buffer of the chunk's one
        readback; False: a one-shot call, which hands enqueue its own arrays and reads nothing back."""
        import torch as t    # here, not at the top: the module is imported where there is no torch
        eng, S = self.eng, self.n_sources
        b = SimpleNamespace(d_times=None, d_src=None, h_times=None, h_src=None, h_read=None)
        if S is not None:
            b.mask, b.scratch = eng.alloc_repeat_sources(cap, S)
            read = runtime.REPEAT_SOURCE_ENTRY.itemsize * S    # the compact table: every source's header and last line
        elif self.window_us is not None:
            b.mask, b.scratch = eng.alloc_repeat_timed(cap)
            read = 0    # the tracker follows (K, T) from the mask, the keys and the times
        else:
            b.mask, b.scratch = eng.alloc_repeat(cap)
            read = STATE_HEAD
        if self.state is None:
            self.state = (eng.alloc_repeat_state(sources=S) if S is not None else
                          eng.alloc_repeat_state() if self.window_us is None else eng.alloc_repeat_state(timed=True))
        if pinned:
            if S is not None:
                b.d_src = t.zeros(cap, dtype=t.int32, device=eng.dev)
                b.h_src = t.zeros(cap, dtype=t.int32).pin_memory()
            if self.window_us is not None:
                b.d_times = t.zeros(cap, dtype=t.int64, device=eng.dev)
                b.h_times = t.zeros(cap, dtype=t.int64).pin_memory()
            if read:
                b.h_read = t.zeros(read, dtype=t.uint8).pin_memory()
        return b

    def enqueue(self, b, json_ins, n: int, stream=None, times=None, sources=None) -> None:
        """The one Engine.mark_* call on ``stream`` (None: the current one): b.mask[:n] and the carried state;
        with b.h_read, the one copy behind it.  The times / ids are those in b.d_times / b.d_src (a stream
        uploads them with the chunk's bytes), or the one-shot call's own host arrays ``times`` / ``sources``."""
        eng, w = self.eng, self.window_us
        d_times = b.d_times if times is None or w is None else eng.torch.from_numpy(times).to(eng.dev)
        if self.n_sources is not None:
            d_src = b.d_src if sources is None else eng.torch.from_numpy(sources).to(eng.dev)
            eng.mark_repeats_by_source(json_ins, n, d_src, self.n_sources, d_times, w, b.mask, b.scratch, self.state,
                                       stream=stream)
        elif w is not None:
            eng.mark_repeats_timed(json_ins, n, d_times, w, b.mask, b.scratch, self.state, stream=stream)
        else:
            eng.mark_repeats(json_ins, n, b.mask, b.scratch, self.state, stream=stream)
        if b.h_read is not None:   # the sources' compact table, or the untimed state's head
            runtime.copy_async(b.h_read, eng.repeat_sources_table(b.scratch, self.n_sources)
                               if self.n_sources is not None else self.state[:STATE_HEAD], stream)

    def exact_mask(self, b, rep, has_key, dev_key_of, host_keys, redo=(), fetch=None,
                   times=None, sources=None, bank=None) -> np.ndarray:
        """The chunk's exact mask from the device's (``rep``, on the host by now): the tracker's fix_chunk (see
        there for has_key .. fetch) with what the pass read back.  ``b``: the chunk's buffers (None: no pass ran);
        ``times`` / ``sources``: the chunk's host arrays; ``bank``: names the protocol ids in an untimed state."""
        wkw = {} if self.window_us is None else {"times": times, "window_us": self.window_us}
        if self.n_sources is not None:
            table = None
            if b is not None:   # a stream's copy, or a one-shot call's read now
                raw = b.h_read if b.h_read is not None else self.eng.repeat_sources_table(b.scratch, self.n_sources).cpu()
                table = raw.numpy().view(runtime.REPEAT_SOURCE_ENTRY)
            return self.tracker.fix_chunk(sources, rep, has_key, dev_key_of, host_keys, redo, fetch, table=table, **wkw)
        end_key = None
        if self.window_us is None and b is not None and b.h_read is not None:
            # what the device's state held after this chunk (read back behind its state pass)
            hs = b.h_read.numpy()
            valid, kd, proto, ln = (int(x) for x in hs[:16].view(np.uint32))
            if valid and ln <= STATE_HEAD - 16:
                pids = (bank.mu_pids, bank.ms_pids, bank.mc_pids, bank.mn_pids)[kd]
                end_key = (_KINDS[kd], str(pids[proto]), hs[16: 16 + ln].tobytes().decode("latin-1"))
        return self.tracker.fix_chunk(rep, has_key, dev_key_of, host_keys, redo, fetch, end_key, **wkw)
