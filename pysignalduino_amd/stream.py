"""Streaming front end: raw firmware lines -> decoded results, chunk after chunk, over PCIe.

The reference decodes one line at a time in its controller's parser task
(signalduino/controller.py:245-264: ``parser.parse_line(line)`` in a worker thread, then the first
decoded message to the callback and the MQTT publisher, signalduino/mqtt.py:227-272).
:class:`LineStream` is the device-rate form of that loop: chunks of raw lines in
pinned host memory go to HBM, are parsed, demodulated and serialised there, and only the results
come back -- with every stage of chunk k overlapping other chunks' stages on four HIP streams:

  copy-in   chunk k's line bytes + offsets H2D                    (stage A, at submit(k))
  parse     sdx_parse_lines + sdx_select_lines, class counts D2H  (stage A)
  demod     the MU / MS short+long, MC ('fixed'), MN launches over the selection lists, then either
            the publish-ready JSON texts (sdx_serialize_json, sparse: all kinds into one buffer)
            or the exchange's wire form (sdx_exchange_count/pack), their sizes D2H   (stage B;
            consecutive chunks alternate between two demodulation streams, so one chunk's
            kernels fill the CUs that the tail of the previous chunk's leaves idle)
  copy-out  the texts (or wire) + per-line kind/status D2H, sized from the device sizes  (stage C)

The host only waits for events of chunks enqueued ``lag`` submits earlier (stage B of chunk k-1
waits for k-1's class counts, stage C of k-2 for its sizes, the collection of k-3 for its copy),
so the GPU always has a chunk queued behind the one it runs.  Lines the fast path does not finish
-- the general path (multi-digit pattern ids, > 4096 pulses), lines outside the device contract,
messages whose results overflowed their buffers (MC frames of > 128 hex characters, ST_OVF_*) --
are taken by ``SignalParser.parse_lines_json`` / ``parse_lines`` on those lines only, so every
line's result is exactly the batch API's.

``submit_bytes`` takes a transport's read buffer as it was read (the reference splits it with
StreamReader.readline(), signalduino/transport.py:113-123): stage A then uploads the bytes only and
runs sdx_split_lines in front of the parse, which writes the offsets on the device; the host cuts the
buffer at line ends into chunks (cut_bytes: rfind + a count, no Python loop over bytes), carries the
unterminated tail into the next call, and gets the chunk's offsets back in stage C.
"""
from __future__ import annotations

import collections
import json
import os
from typing import Any, Deque, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import runtime
from .packing import ContractError

_KINDS = (("MU", runtime.KIND_MU, runtime.SEL_MU_SHORT, runtime.SEL_MU_LONG),
          ("MS", runtime.KIND_MS, runtime.SEL_MS_SHORT, runtime.SEL_MS_LONG),
          ("MC", runtime.KIND_MC, runtime.SEL_MC, runtime.SEL_MC_LONG),
          ("MN", runtime.KIND_MN, runtime.SEL_MN, None))


_FUSE = os.environ.get("SDX_STREAM_FUSE", "1") != "0"
_GROUP2 = os.environ.get("SDX_STREAM_GROUP2", "1") != "0"   # A/B: one sdx_group_step vs two groupings
_MC_SEP = os.environ.get("SDX_STREAM_MC_SEP") == "1"   # A/B: MC's short class in its own launch


class _NlView:
    """rfind / find / count of b"\\n" over a numpy uint8 array, with bytes' signatures: what cut_bytes
    needs of a buffer that is no bytes object (a pinned tensor's memory, a memoryview)."""

    BLOCK = 1 << 16
    PART = 1 << 20      # count(): what one thread takes at a time
    _pool = None

    def __init__(self, a: np.ndarray):
        if not a.flags.c_contiguous:
            raise ValueError("a contiguous uint8 buffer")
        self.a = a
        self.ptr = a.ctypes.data
        self.lib = runtime.load_library()

    def __len__(self) -> int:
        return len(self.a)

    def _count(self, lo: int, hi: int) -> int:
        return int(self.lib.sdx_host_count_byte(self.ptr + lo, hi - lo, 10)) if hi > lo else 0

    def count(self, _nl, lo: int, hi: int) -> int:
        """A chunk's count is the host's one pass over every byte (sdx_host_count_byte, a vectorised C
        loop); large ranges go over a few threads (ctypes releases the GIL), 1 MB parts each."""
        if hi - lo <= 2 * self.PART:
            return self._count(lo, hi)
        if _NlView._pool is None:
            from concurrent.futures import ThreadPoolExecutor
            _NlView._pool = ThreadPoolExecutor(max_workers=8, thread_name_prefix="sdx-nl")
        return sum(_NlView._pool.map(lambda s: self._count(s, min(hi, s + self.PART)), range(lo, hi, self.PART)))

    def rfind(self, _nl, lo: int, hi: int) -> int:
        while hi > lo:      # from the back, a block at a time: the last newline is near the end
            b = max(lo, hi - self.BLOCK)
            hit = np.flatnonzero(self.a[b:hi] == 10)
            if len(hit):
                return b + int(hit[-1])
            hi = b
        return -1

    def find(self, _nl, lo: int, hi: int) -> int:
        while lo < hi:
            e = min(hi, lo + self.BLOCK)
            hit = np.flatnonzero(self.a[lo:e] == 10)
            if len(hit):
                return lo + int(hit[0])
            lo = e
        return -1


def cut_bytes(view, lo: int, carry_len: int, C: int, B: int) -> Tuple[int, int]:
    """The next chunk of a byte buffer: (hi, n) such that view[lo:hi] ends on a '\\n' (or hi == lo: no
    line ends in reach), holds n <= C newlines and, behind a carried line start of ``carry_len`` bytes,
    fits B bytes.  ``view``: bytes-like with rfind / find / count (the host never walks the bytes in
    Python).  A line that cannot fit B bytes raises ValueError."""
    N = len(view)
    room = B - carry_len
    hi = view.rfind(b"\n", lo, min(N, lo + max(room, 0))) + 1
    if hi <= lo:
        if N - lo > room:
            raise ValueError(f"a line of more than {B} bytes (the stream's chunk_bytes)")
        return lo, 0         # only an unterminated tail is left
    n = view.count(b"\n", lo, hi)
    while n > C:             # too many lines: halve the piece and try again
        h2 = view.rfind(b"\n", lo, lo + (hi - lo) // 2) + 1
        if h2 <= lo:         # the first line alone is longer than half the piece
            h2 = view.find(b"\n", lo, hi) + 1
        hi = h2
        n = view.count(b"\n", lo, hi)
    return hi, n


class _ChunkBytes:
    """The raw bytes of a submit_bytes chunk on the host: the carried line start + the piece of the
    caller's buffer (or of the slot's pinned buffer), never joined."""

    def __init__(self, carry: np.ndarray, body: np.ndarray):
        self.carry, self.body = carry, body

    def slice(self, a: int, b: int) -> bytes:
        c = len(self.carry)
        if a >= c:
            return self.body[a - c: b - c].tobytes()
        if b <= c:
            return self.carry[a:b].tobytes()
        return self.carry[a:].tobytes() + self.body[: b - c].tobytes()

    def copy(self) -> "_ChunkBytes":
        return _ChunkBytes(self.carry.copy(), self.body.copy())


class ChunkResult:
    """One chunk's results in host memory.  json output: ``texts()`` -> per line the MQTT text the
    reference publishes for it (``_message_to_json(parse_line(line)[0])``), None (nothing decoded) or
    the line's ContractError.  wire output: ``sections(kind)`` -> the (msg, wire records, wire heap)
    of that kind's launch (include/sdx.h wire v3, per line), ``decode(kind)`` -> (desc, rec, heap);
    ``host`` holds the lines the batch API took (line index -> its parse_lines result).

    The arrays are views of the stream's pinned buffers (no host copy on the critical path): they
    stay valid until the stream's next submit(); ``detach()`` copies them out.  A result the stream
    still holds (finished, not yet returned by poll / drain) is detached by the stream itself before its
    slot's buffers are written again, so submitting several chunks between polls loses nothing."""

    def __init__(self, cid: int, n: int, kind: np.ndarray, status: np.ndarray):
        self.id, self.n, self.kind, self.status = cid, n, kind, status
        self.slot = None          # the _Slot whose pinned buffers the arrays view (None once detached)
        self.json = self.off = self.len = None
        # json_all output: uint32[n + 1], line i's records are [first[i], first[i + 1]) of off / len,
        # which are then indexed by record; host[i] holds a list of texts
        self.first = None
        self.overflow = False     # json_all: the chunk's texts or index overflowed, every decoding line came from the host
        self.wire = self.layout = None
        self.host = {}            # line -> result of the batch API (fallback lines)
        self.repeat = None        # collapse_repeats: uint8[n], 1 = the line repeats the previous result-bearing one
        self.route = None         # routes: int16[n], the line's route (index into the stream's table), -1 = none / no result
        self.pick = None          # route_match="any": uint16[n], the index of the line's published message
        self.source = None        # repeat_sources: int32[n], the lines' source ids as submitted (a copy)
        self.affix = {}
        # the chunk's text, for line(i): the submitted sequence, or packed (data, offsets), or a
        # submit_bytes chunk's bytes (_ChunkBytes) + the device's offsets
        self.src_lines = self.src_data = self.src_offsets = None

    def line(self, i: int) -> bytes:
        """The raw bytes of line i as submitted (a submit_bytes line keeps its terminator)."""
        if not 0 <= i < self.n:
            raise IndexError(i)
        if self.src_lines is not None:
            ln = self.src_lines[i]
            return ln.encode("latin-1") if isinstance(ln, str) else bytes(ln)
        a, b = int(self.src_offsets[i]), int(self.src_offsets[i + 1])
        if isinstance(self.src_data, _ChunkBytes):
            return self.src_data.slice(a, b)
        d = self.src_data.numpy() if hasattr(self.src_data, "numpy") else self.src_data
        return d[a:b].tobytes()

    def lines(self) -> List[bytes]:
        return [self.line(i) for i in range(self.n)]

    def detach(self) -> "ChunkResult":
        if self.slot is None:
            return self
        self.slot = None
        if isinstance(self.src_data, _ChunkBytes):   # views of the slot's or the caller's pinned memory
            self.src_data, self.src_offsets = self.src_data.copy(), self.src_offsets.copy()
        for f in ("kind", "status", "off", "len", "first", "wire", "repeat", "route", "pick"):
            v = getattr(self, f)
            if isinstance(v, np.ndarray):
                setattr(self, f, v.copy())
        if isinstance(self.json, memoryview):
            self.json = self.json.tobytes()
        return self

    def texts(self) -> List[Union[Optional[str], Exception]]:
        out: List[Any] = [None] * self.n
        for i, r in self.items():
            out[i] = r
        return out

    def items(self) -> List[Tuple[int, Union[str, Exception]]]:
        """(line, text or ContractError) for the lines that publish something, in line order: the
        sparse form of texts() (one ASCII decode of the chunk's text buffer, one slice per text)."""
        if self.first is not None:
            raise ValueError("a json_all chunk: texts_all() / items_all()")
        rows = np.nonzero(self.len)[0]
        blob = bytes(self.json).decode("ascii")
        dev = zip(rows.tolist(), [blob[o: o + ln] for o, ln in zip(self.off[rows].tolist(), self.len[rows].tolist())])
        if not self.host:
            return list(dev)
        d = dict(dev)
        d.update(self.host)
        return [(i, d[i]) for i in sorted(d) if d[i] is not None]

    def texts_all(self) -> List[Union[List[str], Exception]]:
        """A json_all chunk: per line the MQTT texts of every message it publishes, in order
        (``parse_lines_json_all``'s slot): [] where nothing is published, the line's ContractError in its slot."""
        out: List[Any] = [[] for _ in range(self.n)]
        for i, r in self.items_all():
            out[i] = r
        return out

    def items_all(self) -> List[Tuple[int, Union[List[str], Exception]]]:
        """(line, its list of texts or its ContractError) for the lines with at least one text or an exception, in
        line order: one ASCII decode of the chunk's text buffer, one slice per text.  A record of length 0 is no
        text."""
        if self.first is None:
            raise ValueError("no json_all chunk: texts() / items()")
        first = self.first.astype(np.int64)
        total = int(first[self.n])
        ln = self.len[:total]
        recs = np.nonzero(ln)[0]
        blob = bytes(self.json).decode("ascii")
        texts = [blob[o: o + k] for o, k in zip(self.off[:total][recs].tolist(), ln[recs].tolist())]
        lines = (np.searchsorted(first, recs, side="right") - 1).tolist()   # first is non-decreasing
        d: dict = {}
        for i, x in zip(lines, texts):
            if i not in self.host:
                d.setdefault(i, []).append(x)
        for i, x in self.host.items():
            if isinstance(x, BaseException) or x:
                d[i] = x
        return [(i, d[i]) for i in sorted(d)]

    def items_routed(self) -> List[Tuple[int, int, Union[str, Exception]]]:
        """items() with every line's route: (line, route, text or ContractError), route -1 = unrouted (a
        stream with ``routes``)."""
        route = self.route
        return [(i, int(route[i]), x) for i, x in self.items()]

    def sections(self, k: int):
        offs, nb, T = self.layout
        o = offs[0, k]
        b = self.wire
        return (b[o[0]: o[0] + nb[0, k, 0]].view(np.uint32), b[o[1]: o[1] + nb[0, k, 1]].view(runtime.WIRE_REC_DT),
                b[o[2]: o[2] + nb[0, k, 2]])

    def decode(self, k: int):
        from . import dist as sdist
        return sdist.wire_decode([self.sections(k)], self.affix.get(k))


class _Slot:
    """Device + pinned host buffers of one chunk in flight."""

    def __init__(self, ls: "LineStream"):
        from .frontend import LineBatch
        t, eng = ls.torch, ls.eng
        C, B = ls.C, ls.B
        self.lb = LineBatch(eng, np.zeros(B, np.uint8), np.linspace(0, B, C + 1).astype(np.int64))
        self.h_bytes = t.empty(B + 16, dtype=t.uint8).pin_memory()
        self.h_offs = t.empty(C + 1, dtype=t.int64).pin_memory()
        self.h_cnt = t.zeros(8, dtype=t.int32).pin_memory()
        self.outs = {}
        nmn = max(1, len(ls.bank.mn_pids))
        caps = {"MU": (8 * C + 4096, 200 * C + 65536), "MS": (4 * C + 4096, 64 * C + 65536),
                "MC": (4 * C + 4096, 96 * C + 65536), "MN": (nmn * C + 4096, 4 * B + 64 * C + 65536)}
        for name, kd, _, _ in _KINDS:
            if name == "MC" and not ls.mc:
                continue
            rc, hc = caps[name]
            # wire output: k_pulses / k_mc write the exchange's counts (k_mn does not)
            self.outs[name] = eng.alloc_out(C, rc, hc, eng.pulses_work_bytes(C) if name in ("MU", "MS") else 0,
                                            wire=ls.output == "wire" and name != "MN")
        self.gbufs = {name: eng.group_buffers(C) for name in ("MU", "MS")}
        # what a chunk resets before its launches -- the cursors, every kind's descriptors (lines of other
        # classes keep an empty one) and exchange counts -- in ONE block, reset by one fill per chunk
        # (seven hipMemsetAsync blit kernels per chunk before)
        parts, off = [], 0
        for name, o in self.outs.items():
            parts.append((name, "desc", off, 8 * C))
            off = (off + 8 * C + 255) & ~255
            if o.get("wire") is not None:
                parts.append((name, "wire", off, 8 * C))
                off = (off + 8 * C + 255) & ~255
        self.zblock = t.zeros(off + 16 * len(self.outs), dtype=t.uint8, device=eng.dev)
        for name, field, o0, nb in parts:
            v = self.zblock[o0: o0 + nb]
            self.outs[name][field] = v.view(t.int64) if field == "wire" else v
        self.cursors = self.zblock[off:].view(t.int32).view(len(self.outs), 4)
        for j, o in enumerate(self.outs.values()):
            o["cursor"] = self.cursors[j]
        if ls.output == "json":
            self.jcap = 600 * C + 65536
            self.jout = eng.alloc_json(C, self.jcap)
            self.h_sizes = t.zeros(2 + 4 * len(self.outs), dtype=t.int32).pin_memory()
            self.h_out = t.empty(self.jcap + 11 * C + 64, dtype=t.uint8).pin_memory()
        elif ls.all:
            # every message of a line: one record-indexed result for all kinds.  The index cannot
            # overflow (no pass adds records); the text buffer is twice the json stream's, the one-shot call's first try
            self.rec_max = sum(o["rec_cap"] for o in self.outs.values())
            self.jcap = 2 * (600 * C + 65536)
            self.idx = eng.alloc_line_index(C, self.rec_max, self.jcap)
            self.h_sizes = t.zeros(3 + 4 * len(self.outs), dtype=t.int32).pin_memory()   # text cursor [2], first[n], cursors
            self.h_out = t.empty(self.jcap + 4 * (C + 1) + 8 * self.rec_max + 3 * C + 64, dtype=t.uint8).pin_memory()
        else:
            from . import dist as sdist
            self.ser = sdist.Exchange.sender(eng)
            self.h_sizes = t.zeros(runtime.XCHG_COUNTS * len(self.outs) + 4 * len(self.outs), dtype=t.int32).pin_memory()
            cap = sum(16 * C + 8 * o["rec_cap"] + o["heap_cap"] + 64 for o in self.outs.values())
            self.h_out = t.empty(cap + 3 * C + 64, dtype=t.uint8).pin_memory()
        if ls.collapse:   # the repeat pass's buffers: the mask, and the pinned copies the chunk's times / ids go through
            self.rb = ls.repeats.alloc(C, pinned=True)
            self.rep, self.h_times, self.h_src = self.rb.mask, self.rb.h_times, self.rb.h_src
        if ls.profiles is not None:
            # the profile pass's outputs: per kind descriptors, records and a cursor of their own beside the
            # launch's (whose heap they share); the ids come up in the repeat pass's buffers, or in the slot's own
            self.pf = eng.alloc_profiles(C, list(self.outs.values()))
            self.fouts = dict(zip(self.outs, self.pf["outs"]))
            if ls.n_sources is None and ls.profiles.n_sources > 1:
                self.p_d_src = t.zeros(C, dtype=t.int32, device=eng.dev)
                self.p_h_src = t.zeros(C, dtype=t.int32).pin_memory()
        if ls.rules is not None:
            # the dispatch pass's outputs, behind the profile pass's where there is one
            self.dp = eng.alloc_dispatch(C, list((self.fouts if ls.profiles is not None else self.outs).values()))
            self.douts = dict(zip(self.outs, self.dp["outs"]))
        if ls.routes is not None:   # the route pass's outputs; its skip mask only where the device drops the unrouted
            extra = {"pick": True, "views": len(self.outs)} if ls.match_any else {}   # "first": the call as it was
            self.rt = eng.alloc_routes(C, mask=False, skip=ls.device_drop, **extra)
            # + int16[C] behind the rest (route_match="any": + uint16[C], the picks)
            self.h_out = t.empty(self.h_out.numel() + (4 if ls.match_any else 2) * C + 8, dtype=t.uint8).pin_memory()
        self.reset()

    def reset(self):
        self.cid = -1
        self.stage = 0
        self.n = 0
        self.lines = None
        self.ev = None
        self.src = None           # a submit_bytes chunk: its _ChunkBytes (the offsets come back in stage C)
        self.times = None         # repeat_window: the chunk's arrival times, int64[n] (a host copy for _fix_repeats)
        self.sources = None       # repeat_sources: the chunk's source ids, int32[n] (the same)


class LineStream:
    """See the module docstring.  ``parser``: a frontend.SignalParser; ``chunk_lines`` /
    ``chunk_bytes``: the capacity of one chunk; ``output``: "json" (the controller's publication) or
    "wire" (per line and kind the exchange's wire form); ``lag``: chunks the host stays behind the
    GPU (slots = lag + 1); ``collapse_repeats`` / ``repeat_window`` (seconds): repeat suppression, with a
    window every submit carries arrival times in integer microseconds, non-decreasing over the stream
    (repeats.py): ``submit(lines, times=)`` and ``submit_packed(..., times=)`` one per line,
    ``submit_bytes(buf, time=)`` one per read buffer.  ``repeat_sources`` = S (with collapse_repeats): the
    stream merges S receivers and repeat suppression runs per source id: ``submit(lines,
    sources=)`` and ``submit_packed(..., sources=)`` take one id in [0, S) per line, ``submit_bytes(buf,
    source=)`` one per read buffer -- the stream keeps one carried tail and one last time per source, so
    read buffers of different receivers may be handed over alternately; times need not decrease within a
    source only.  ChunkResult.source holds the ids beside ``repeat``.  ``routes`` (a routes.RouteTable or a list of
    (name, pattern) pairs) / ``drop_unrouted``: payload routes -- the route pass runs behind the
    repeat pass and in front of the serialiser, ChunkResult.route holds every line's route, items_routed() the
    published lines with theirs; with ``drop_unrouted`` a json stream publishes result-bearing, non-repeat,
    routed lines only (a wire stream's sections are never changed).  ``route_match="any"``: the
    line's first message that a route matches is the published one -- the match runs first (sdx_route_records), the
    repeat pass and the serialiser over its picked views; ChunkResult.pick holds the message's index.
    ``output="json_all"``: every message of a line, as ``parse_lines_json_all`` -- the chunk's texts
    are indexed by record, ChunkResult.first gives every line its range, texts_all() / items_all() the lists;
    ``rules`` (None: every message; True or a dispatch.DispatchRules: FHEM's dispatch rules) reduces
    every list on the device first.  It combines with ``profiles`` and repeat suppression (a repeat line gives []),
    not with routes.

    submit(lines) -> chunk id; ``submit_packed(data, offsets)`` the same for lines already packed as
    (uint8 bytes, int64 offsets[n + 1]); ``submit_bytes(buf)`` -> chunk ids for a transport's raw read
    buffer (split into lines on the device, the tail carried to the next call); poll() -> the finished
    chunks' ChunkResults in submission
    order (never blocks on a chunk newer than ``lag`` submits); drain() -> all of them (blocks)."""

    def __init__(self, parser, chunk_lines: int = 250_000, chunk_bytes: Optional[int] = None, output: str = "json",
                 lag: int = 3, collapse_repeats: bool = False, repeat_window: Optional[float] = None,
                 repeat_sources: Optional[int] = None, routes=None, drop_unrouted: bool = False,
                 route_match: str = "first", profiles=None, rules=None):
        if output not in ("json", "wire", "json_all"):
            raise ValueError("output must be 'json', 'json_all' or 'wire'")
        # every message of a line: ``rules``, not ``dispatch`` -- the name the one-shot calls use is
        # pinned to raise TypeError on a stream
        self.all = output == "json_all"
        from .dispatch import as_rules
        self.rules = as_rules(rules)            # dispatch rules; None: every message, no pass, no buffer
        if self.rules is not None and not self.all:
            raise ValueError("rules need output='json_all'")
        if self.all and (routes is not None or drop_unrouted or route_match != "first"):
            raise ValueError("output='json_all' takes no routes (routes per record are not covered)")
        from .profiles import as_profiles
        self.profiles = as_profiles(profiles)   # receiver profiles; None: no pass, no buffer
        if self.profiles is not None and output == "wire":
            # the exchange pack reads the demodulation kernels' own per-message counts, which the pass does not rewrite
            raise ValueError("profiles need output='json'")
        from .frontend import _check_route_match
        _check_route_match(route_match, routes)
        self.match_any = route_match == "any"
        from .routes import as_table
        self.routes = as_table(routes)    # payload routes; None: no pass, no buffer, no copy
        self.drop = bool(drop_unrouted)
        if self.drop and self.routes is None:
            raise ValueError("drop_unrouted needs routes")
        self.collapse = bool(collapse_repeats)
        from .repeats import window_to_us
        self.window_us = window_to_us(repeat_window)
        if self.window_us is not None and not self.collapse:
            raise ValueError("repeat_window needs collapse_repeats=True")
        self._last_time = None    # repeat_window: the last submitted line's time
        self.n_sources = None if repeat_sources is None else runtime._n_sources(repeat_sources)
        if self.n_sources is not None and not self.collapse:
            raise ValueError("repeat_sources needs collapse_repeats=True")
        if self.profiles is not None and self.n_sources is not None and self.profiles.n_sources != self.n_sources:
            raise ValueError(f"the profile table maps {self.profiles.n_sources} sources, repeat_sources is {self.n_sources}")
        # the ids a submit names: the repeat pass's, or (several receivers' profiles without it) the profile pass's alone
        self.id_sources = self.n_sources
        if self.id_sources is None and self.profiles is not None and self.profiles.n_sources > 1:
            self.id_sources = self.profiles.n_sources
        self._last_times = {}     # repeat_sources with a window: source -> its last submitted line's time
        self._carries = {}        # repeat_sources, submit_bytes: source -> its unterminated tail
        import torch
        self.torch = torch
        self.parser = parser
        self.eng = parser.protocols._ensure()
        self.bank = parser.protocols._bank
        if self.rules is not None:
            self.drules = self.rules.struct(self.bank)   # compiled once; an id the bank does not know raises here
        self.mc = parser.protocols.mc_mode == "fixed"   # 'strict' MC reaches no device launch
        self.output = output
        self.C = int(chunk_lines)
        self.B = int(chunk_bytes or 256 * self.C)
        self.lag = max(1, int(lag))
        if self.collapse:
            # repeat suppression: ONE state per stream (the RepeatPass's), written by every chunk's
            # state pass; rep_ev orders the next chunk's pass (on the other demodulation stream) behind it
            from .repeats import RepeatPass
            self.repeats = RepeatPass(self.eng, self.window_us, self.n_sources)
            self.rep_ev = None
        if self.routes is not None:
            self.dtable = self.eng.route_table(self.routes)
        if self.profiles is not None:
            self.ptable = self.eng.profile_table(self.profiles)
        # json: the device leaves unrouted lines out of the text buffer -- unless repeats are collapsed: the
        # host tracker then needs the key of every line that is no repeat, so those texts come back and are
        # dropped in _collect.  wire: the sections are unchanged, the route only travels beside them
        self.device_drop = self.drop and output == "json" and not self.collapse
        self.slots = [_Slot(self) for _ in range(self.lag + 1)]
        dev = self.eng.dev
        # the parse at the highest priority: the host waits for chunk k's class counts before it can
        # enqueue chunk k's demodulation, and a parse queued behind the previous chunks' demodulation
        # tiles got CUs only as those drained -- the chunks' kernels then ran one after another
        lo_prio, hi_prio = torch.cuda.Stream.priority_range()
        self.cin, self.cout = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
        self.sp = torch.cuda.Stream(dev, priority=hi_prio)
        # two demodulation streams, chunk k on sds[k % 2]: every buffer a chunk's stage B touches is
        # its slot's own, so chunk k+1's launches may run beside chunk k's (one stream
        # serialised the chunks' kernels and each chunk's tail idled the CUs)
        self.sds = (torch.cuda.Stream(dev), torch.cuda.Stream(dev))
        self.sd = self.sds[0]
        self.inflight: Deque[_Slot] = collections.deque()
        self.done: Deque[ChunkResult] = collections.deque()
        self.next_id = 0
        self.elig = parser.protocols.mn_eligibility(parser.rfmode)
        if self.profiles is not None:   # an MN protocol no profile enables is never run
            self.elig &= self.profiles.mn_elig(self.bank)
        self.h2d_bytes = self.d2h_bytes = 0
        self.kernel_events = []   # (parse start, parse end, demod start, demod end) per chunk
        self._carry = bytearray()  # submit_bytes: the unterminated tail of the calls so far

    # -- public ------------------------------------------------------------------------------------------
    def submit(self, lines: Sequence[Union[str, bytes]], times=None, sources=None) -> int:
        from .frontend import pack_lines
        sources = self._check_sources(sources, len(lines))   # before anything is packed or launched
        times = self._check_times(times, len(lines), self._rsrc(sources))
        data, offsets, bad = pack_lines(lines, copy=False)   # read once, into the slot's pinned buffer
        return self.submit_packed(data, offsets, lines=lines, bad=bad, times=times, sources=sources)

    def _check_sources(self, sources, n: int):
        """A chunk's source ids as int32[n] (None on a stream without repeat_sources or several receivers'
        profiles); ValueError when they are missing, given to a stream that takes none, or outside [0, S)."""
        if self.id_sources is None:
            if sources is not None and self.profiles is None:
                raise ValueError("sources given, but the stream has no repeat_sources")
            if sources is not None:      # one receiver's profiles: every id must be 0, and none need be given
                from .repeats import check_sources
                check_sources(sources, n, 1)
            return None
        from .repeats import check_sources
        return check_sources(sources, n, self.id_sources)

    def _rsrc(self, sources):
        """The ids as the repeat pass sees them: None unless the stream has repeat_sources."""
        return sources if self.n_sources is not None else None

    def _check_times(self, times, n: int, sources=None):
        """A chunk's arrival times as int64[n] (None without a window); ValueError when they are missing,
        decrease, or start before the previous chunk's last one -- with ``sources`` within each source."""
        if self.window_us is None:
            if times is not None:
                raise ValueError("times given, but the stream has no repeat_window")
            return None
        from .repeats import check_times
        if sources is not None:
            return check_times(times, n, self._last_times, sources)
        return check_times(times, n, self._last_time)

    def submit_packed(self, data, offsets: np.ndarray, lines=None, bad=None, times=None, sources=None) -> int:
        """``data``: the lines' bytes as a numpy uint8 array (copied into the slot's pinned buffer) or
        a PINNED torch uint8 tensor (uploaded from where it is, no host copy: keep it unchanged until
        the chunk has been collected); ``offsets``: int64[n + 1] into it; ``times``: with a
        ``repeat_window``, the n arrival times (integer microseconds); ``sources``: with
        ``repeat_sources``, the n source ids."""
        n = len(offsets) - 1
        if n > self.C or int(offsets[-1] - offsets[0]) > self.B:
            raise ValueError(f"chunk of {n} lines / {int(offsets[-1] - offsets[0])} bytes exceeds the stream's "
                             f"capacity ({self.C} lines, {self.B} bytes)")
        sources = self._check_sources(sources, n)
        times = self._check_times(times, n, self._rsrc(sources))
        s = self._take_slot(n)
        self._set_times(s, times, sources)
        s.lines, s.bad = lines, bad or {}
        s.data, s.offsets = data, offsets
        self._stage_a(s, data, offsets)
        return self._queued(s)

    def _take_slot(self, n: int) -> _Slot:
        while len(self.inflight) >= len(self.slots):     # every slot busy: finish the oldest chunk
            self._advance(self.inflight[0], 4)
        s = next(x for x in self.slots if x.stage == 0)
        for r in self.done:     # a byte chunk's result not handed out yet views this slot's input buffers
            if r.slot is s and isinstance(r.src_data, _ChunkBytes):
                r.detach()
        s.cid, s.n = self.next_id, n
        self.next_id += 1
        return s

    def _set_times(self, s: _Slot, times, sources=None) -> None:
        """The chunk's checked times (and source ids) into its slot's pinned buffers (stage A uploads them
        with the chunk)."""
        s.times = s.sources = None
        if sources is not None:
            n = len(sources)
            s.sources = (s.h_src if self.n_sources is not None else s.p_h_src).numpy()[:n]
            s.sources[:] = sources
        if times is not None:
            n = len(times)
            s.times = s.h_times.numpy()[:n]     # the slot's own copy: the caller's array may change
            s.times[:] = times
            if n and self._rsrc(sources) is not None:       # every source's last line of the chunk
                ids, back = np.unique(s.sources[::-1], return_index=True)
                for sid, j in zip(ids.tolist(), (n - 1 - back).tolist()):
                    self._last_times[sid] = int(s.times[j])
            elif n:
                self._last_time = int(times[-1])

    def _upload_times(self, s: _Slot) -> None:
        """On the input stream, in front of the chunk's h2d event: 8 bytes per line, 4 for its source id."""
        if s.times is not None and s.n:
            runtime.copy_async(s.rb.d_times[: s.n], s.h_times[: s.n], self.cin)
            self.h2d_bytes += 8 * s.n
        if s.sources is not None and s.n:
            if self.n_sources is not None:
                runtime.copy_async(s.rb.d_src[: s.n], s.h_src[: s.n], self.cin)
            else:
                runtime.copy_async(s.p_d_src[: s.n], s.p_h_src[: s.n], self.cin)
            self.h2d_bytes += 4 * s.n

    def _queued(self, s: _Slot) -> int:
        self.inflight.append(s)
        # the chunks behind: stage B for the previous one, C for the one before, collect the oldest
        for age, want in ((1, 2), (2, 3), (3, 4)):
            if len(self.inflight) > age and self.lag >= age:
                self._advance(self.inflight[-1 - age], want)
        return s.cid

    def submit_bytes(self, buf, final: bool = False, time: Optional[int] = None, source: Optional[int] = None) -> List[int]:
        """A transport's read buffer, raw: ``buf`` is bytes-like (copied into the slot's pinned buffer) or
        a PINNED torch uint8 tensor (uploaded from where it is: keep it unchanged until its chunks have
        been collected), of any size.  Every '\\n' ends a line (StreamReader.readline(),
        signalduino/transport.py:113-123); the lines are found on the device (sdx_split_lines), the host
        only cuts the buffer at line ends into chunks within ``chunk_lines`` / ``chunk_bytes`` (cut_bytes).
        The unterminated tail is carried into the next call; ``final=True`` (or close_bytes()) makes a
        non-empty tail the last line.  Returns the ids of the chunks queued (none, one or several).  A
        line longer than ``chunk_bytes`` raises ValueError: the chunks cut in front of it stay queued, the
        line and what follows it in ``buf`` are not taken.  ``time``: with a ``repeat_window``, the arrival
        time of this read buffer (integer microseconds, not earlier than the previous one's).  A line gets
        the time of the buffer that holds its terminating newline -- when StreamReader.readline() would
        have returned it --, an unterminated tail made the last line the time of the last buffer.
        ``source``: with ``repeat_sources``, the receiver this buffer was read from: every line of the chunks
        it queues has that id, the tail is carried to the next buffer of the SAME source, and ``time`` must
        not be earlier than that source's previous one."""
        t = self.torch
        if self.id_sources is None:
            if source is not None and (self.profiles is None or source != 0):
                raise ValueError("source given, but the stream has no repeat_sources" if self.profiles is None else
                                 "the stream's profile table has one source: source must be 0")
            source = None
        else:
            if source is None or int(source) != source or not 0 <= int(source) < self.id_sources:
                raise ValueError(f"a stream with repeat_sources or several receivers' profiles needs the read buffer's "
                                 f"source id (source=) inside [0, {self.id_sources})")
            source = int(source)
        tsrc = self._rsrc(source)     # times run per source only where the repeat pass does
        last_time = self._last_time if tsrc is None else self._last_times.get(tsrc)
        if self.window_us is None:
            if time is not None:
                raise ValueError("time given, but the stream has no repeat_window")
        else:
            if time is None and len(buf):   # an empty buffer ends no line: close_bytes() needs no time
                raise ValueError("a repeat window needs the read buffer's arrival time (time=)")
            if time is not None:
                if int(time) != time:
                    raise ValueError("time: integer microseconds")
                if last_time is not None and int(time) < last_time:
                    raise ValueError("times must not decrease over a stream's lines")
                if tsrc is None:
                    self._last_time = int(time)
                else:
                    self._last_times[tsrc] = int(time)
        if isinstance(buf, (bytes, bytearray)):
            arr = np.frombuffer(buf, np.uint8)
            view = buf if len(buf) <= 2 * _NlView.PART else _NlView(arr)   # a read buffer: bytes' own rfind / count
        else:
            arr = buf.numpy() if isinstance(buf, t.Tensor) else np.frombuffer(memoryview(buf).cast("B"), np.uint8)
            view = _NlView(arr)
        pinned = isinstance(buf, t.Tensor) and buf.is_pinned()
        N, lo, ids = len(arr), 0, []
        while True:
            hi, n = cut_bytes(view, lo, len(self._tail(source)), self.C, self.B)
            if hi == lo:
                break
            ids.append(self._submit_piece(buf if pinned else None, arr, lo, hi, n, False, source))
            lo = hi
        self._tail(source).extend(arr[lo:N].tobytes())     # short: less than one line
        if final and self._tail(source):
            ids.append(self._submit_piece(None, arr, N, N, 1, True, source))
        return ids

    def _tail(self, source: Optional[int]) -> bytearray:
        """The carried, unterminated tail: the stream's, with repeat_sources that of one source."""
        return self._carry if source is None else self._carries.setdefault(source, bytearray())

    def close_bytes(self, source: Optional[int] = None) -> List[int]:
        """End of the byte stream: a carried tail becomes the last line (submit_bytes(b"", final=True)).
        With ``repeat_sources``: every source's tail, in id order, or only that of ``source``."""
        if self.id_sources is None:
            return self.submit_bytes(b"", final=True, **({} if source is None else {"source": source}))
        ids = []
        for sid in (sorted(self._carries) if source is None else [source]):
            ids += self.submit_bytes(b"", final=True, source=sid)
        return ids

    def _submit_piece(self, pinned_buf, arr: np.ndarray, lo: int, hi: int, n: int, final: bool,
                      source: Optional[int] = None) -> int:
        if source is None:
            carry, self._carry = self._carry, bytearray()
        else:
            carry, self._carries[source] = self._tail(source), bytearray()
        s = self._take_slot(n)
        s.lines, s.bad = None, {}
        s.data = s.offsets = None
        when = self._last_time if self._rsrc(source) is None else self._last_times.get(source)
        self._set_times(s, None if self.window_us is None else np.full(n, when, np.int64),
                        None if source is None else np.full(n, source, np.int32))
        self._stage_a_bytes(s, np.frombuffer(bytes(carry), np.uint8), pinned_buf, arr, lo, hi, final)
        return self._queued(s)

    def poll(self) -> List[ChunkResult]:
        for s in list(self.inflight):      # stages B and C of any chunk whose previous stage is done
            while s.stage in (1, 2) and s.ev.query():
                self._advance(s, s.stage + 1)
            if self.collapse and s.stage == 1:
                break     # the chunks' repeat passes are enqueued in submission order
        while self.inflight and self.inflight[0].stage == 3 and self.inflight[0].ev.query():
            self._advance(self.inflight[0], 4)     # results leave in submission order
        return self._pop_done()

    def drain(self) -> List[ChunkResult]:
        while self.inflight:
            self._advance(self.inflight[0], 4)
        return self._pop_done()

    # -- stages --------------------------------------------------------------------------------------------
    def _pop_done(self):
        out = []
        while self.done:
            out.append(self.done.popleft())
        return out

    def _advance(self, s: _Slot, want: int) -> bool:
        if want >= 4:
            while self.inflight and self.inflight[0] is not s:   # results leave in submission order
                self._advance(self.inflight[0], 4)
        if self.collapse and want >= 2 and s.stage == 1:   # stage B in submission order (the carried state)
            for o in list(self.inflight):
                if o is s:
                    break
                if o.stage == 1:
                    self._stage_b(o)
        while 0 < s.stage < want:      # _collect frees the slot (stage 0): nothing left to advance
            if s.stage == 1:
                self._stage_b(s)
            elif s.stage == 2:
                self._stage_c(s)
            elif s.stage == 3:
                self._collect(s)
        return True

    def _stage_a(self, s: _Slot, data, offsets):
        t = self.torch
        n, o0, nb = s.n, int(offsets[0]), int(offsets[-1] - offsets[0])
        np.subtract(offsets, o0, out=s.h_offs.numpy()[: n + 1])   # rebased straight into the pinned buffer
        lb = s.lb
        pinned = isinstance(data, t.Tensor) and data.is_pinned()
        if not pinned:
            s.h_bytes.numpy()[:nb] = data[o0: o0 + nb]
        with t.cuda.stream(self.cin):
            if pinned:   # straight from the caller's pinned buffer; the 16 pad bytes zeroed on the device
                lb.bytes[:nb].copy_(data[o0: o0 + nb], non_blocking=True)   # the caller's tensor: torch tracks it
                runtime.fill_async(lb.bytes[nb: nb + 16], self.cin)
            else:
                s.h_bytes.numpy()[nb: nb + 16] = 0
                runtime.copy_async(lb.bytes[: nb + 16], s.h_bytes[: nb + 16], self.cin)
            runtime.copy_async(lb.offsets[: n + 1], s.h_offs[: n + 1], self.cin)
            self._upload_times(s)
            h2d = t.cuda.Event()
            h2d.record(self.cin)
        self.h2d_bytes += nb + 8 * (n + 1)
        lb.n = n
        lb.c_lines.n = n
        with t.cuda.stream(self.sp):
            self.sp.wait_event(h2d)
            e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
            e0.record(self.sp)
            lb.launch()
            e1.record(self.sp)
            runtime.copy_async(s.h_cnt, lb.counts, self.sp)
            ev = t.cuda.Event()
            ev.record(self.sp)
        s.parse_ev, s.ev, s.kt = e1, ev, [e0, e1]
        s.stage = 1

    def _stage_a_bytes(self, s: _Slot, carry: np.ndarray, pinned_buf, arr: np.ndarray, lo: int, hi: int, final: bool):
        """Stage A of a submit_bytes chunk: carry + arr[lo:hi] H2D (no offsets: sdx_split_lines writes them
        on the device, in front of the parse), the split's count D2H beside the class counts.  The host
        knows the chunk's n (cut_bytes), so the parse is sized without waiting for the device."""
        t, lb, n = self.torch, s.lb, s.n
        cl, m = len(carry), hi - lo
        nb = cl + m
        if not hasattr(s, "d_split"):   # the split's buffers, on the slot's first byte chunk
            # empty, not zeros: a fill kernel would run on the framework's stream, unordered against the split below,
            # which writes both words
            s.d_split = t.empty(2, dtype=t.int64, device=self.eng.dev)
            s.h_split = t.zeros(2, dtype=t.int64).pin_memory()
            s.split_scratch = t.empty(self.eng.split_work_ints(self.B), dtype=t.int32, device=self.eng.dev)
        hb = s.h_bytes.numpy()
        hb[:cl] = carry
        if pinned_buf is None:
            hb[cl:nb] = arr[lo:hi]
            hb[nb: nb + 16] = 0
            s.src = _ChunkBytes(hb[:0], hb[:nb])
        else:
            s.src = _ChunkBytes(hb[:cl], arr[lo:hi])
        with t.cuda.stream(self.cin):
            if pinned_buf is None:
                runtime.copy_async(lb.bytes[: nb + 16], s.h_bytes[: nb + 16], self.cin)
            else:   # the piece straight from the caller's pinned buffer, the carried line start in front of it
                if cl:
                    runtime.copy_async(lb.bytes[:cl], s.h_bytes[:cl], self.cin)
                lb.bytes[cl:nb].copy_(pinned_buf[lo:hi], non_blocking=True)
                runtime.fill_async(lb.bytes[nb: nb + 16], self.cin)
            self._upload_times(s)
            h2d = t.cuda.Event()
            h2d.record(self.cin)
        self.h2d_bytes += nb
        lb.n = n
        lb.c_lines.n = n
        with t.cuda.stream(self.sp):
            self.sp.wait_event(h2d)
            e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
            e0.record(self.sp)
            # cap = the host's n: a device count above it writes nothing past offsets[n]; one below it
            # leaves older offsets of this slot behind (all within the slot's buffers) -- either way the
            # counts differ and stage B raises
            self.eng.split_lines(lb.bytes, nb, final, lb.offsets, n, s.d_split, s.split_scratch, self.sp)
            lb.launch()
            e1.record(self.sp)
            runtime.copy_async(s.h_cnt, lb.counts, self.sp)
            runtime.copy_async(s.h_split, s.d_split, self.sp)
            ev = t.cuda.Event()
            ev.record(self.sp)
        s.parse_ev, s.ev, s.kt = e1, ev, [e0, e1]
        s.stage = 1

    def _stage_b(self, s: _Slot):
        """The demodulation + serialisation launches, sized by the class counts (on the host by now)."""
        t, eng = self.torch, self.eng
        s.ev.synchronize()
        if s.src is not None and int(s.h_split.numpy()[0]) != s.n:
            dn, hn, cid = int(s.h_split.numpy()[0]), s.n, s.cid
            self.inflight.remove(s)     # the chunk is dropped: its offsets are not the host's lines
            s.reset()
            raise RuntimeError(f"chunk {cid}: sdx_split_lines found {dn} lines, the host counted {hn}")
        cnt = s.h_cnt.numpy()[: runtime.SEL_NCLASS].astype(np.int64)
        start = np.concatenate([[0], np.cumsum(cnt)])
        lb, n = s.lb, s.n
        sels = [lb.sel[int(start[i]): int(start[i + 1])] for i in range(runtime.SEL_NCLASS)]
        sd = self.sds[s.cid % 2]
        with t.cuda.stream(sd):
            sd.wait_event(s.parse_ev)
            e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
            e0.record(sd)
            runtime.fill_async(s.zblock, sd)   # cursors, descriptors, exchange counts
            pb = lb.pulse_batch()
            # MU short, MS short and MC as ONE k_step launch (sdx_demod_step: each kind's tiles take the
            # slots the previous kind's last tiles free); the long variants and MN keep their own
            step = {}
            # both short classes grouped: one sdx_group_step (the two sorts' passes in the same launches)
            orders = {}
            mu_s, ms_s = runtime.SEL_MU_SHORT, runtime.SEL_MS_SHORT
            if _GROUP2 and "MU" in s.outs and "MS" in s.outs and min(cnt[mu_s], cnt[ms_s]) >= runtime.GROUP_MIN:
                orders["MU"], orders["MS"] = eng.group_step(pb, pb, s.gbufs["MU"], s.gbufs["MS"], sels[mu_s], sels[ms_s])
            for name, kd, short, long_ in _KINDS:
                o = s.outs.get(name)
                if o is None:
                    continue
                o["n"] = n
                if kd == runtime.KIND_MN:
                    if cnt[short]:
                        eng.launch_mn(lb.mn_batch(), o, elig=self.elig, sel=sels[short])
                elif kd == runtime.KIND_MC:
                    if cnt[short]:   # <= 64 characters (the class's bound): part of the fused kernel
                        step["mc"] = (dict(lb.mc_batch(), max_hex=0 if _MC_SEP else runtime.MC_SHORT_HEX), o,
                                      sels[short])
                elif cnt[short]:   # the grouped order (the slot's own grouping buffers: no shared cache)
                    sel = (orders[name] if name in orders else
                           eng.group(kd, pb, sels[short], bufs=s.gbufs[name]) if cnt[short] >= runtime.GROUP_MIN
                           else sels[short])
                    step[name.lower()] = (pb, o, sel, None)
            if step and _FUSE:
                eng.launch_step(**step)
            elif step:   # A/B (SDX_STREAM_FUSE=0): one launch per kind
                for k, kd in (("mu", runtime.KIND_MU), ("ms", runtime.KIND_MS)):
                    if k in step:
                        eng.launch_pulses(kd, pb, step[k][1], sel=step[k][2], group=False)
                if "mc" in step:
                    eng.launch_mc(step["mc"][0], step["mc"][1], sel=step["mc"][2])
            for name, kd, short, long_ in _KINDS:
                if long_ is not None and cnt[long_] and name in s.outs:
                    if kd == runtime.KIND_MC:   # 65..128 characters
                        eng.launch_mc(lb.mc_batch(), s.outs[name], sel=sels[long_])
                    else:
                        eng.launch_pulses(kd, pb, s.outs[name], sel=sels[long_], long_variant=True)
            s.cnt = cnt
            lo = {"meta": lb.meta, "pat_val": lb.pat_val, "cp_slot": lb.cp_slot}
            outs = s.outs
            if self.profiles is not None:
                # right behind the launches: every line keeps the records its source's profile enables;
                # everything below reads the filtered outputs.  The ids came up with the chunk's bytes (stage A)
                ins = [eng.json_in(kd, s.outs[name], lo, n, 2) for name, kd, _, _ in _KINDS if name in s.outs]
                for o in s.pf["outs"]:
                    o["n"] = n
                d_src = None if s.sources is None else s.rb.d_src if self.n_sources is not None else s.p_d_src
                eng.filter_records(self.ptable, ins, n, s.pf, source=d_src, stream=sd)
                outs = s.fouts
            if self.rules is not None:
                # the dispatch rules behind the profiles: a disabled protocol never counts.  A line's
                # first record stays, so the repeat pass below decides what a json stream's would
                ins = [eng.json_in(kd, outs[name], lo, n, 2) for name, kd, _, _ in _KINDS if name in outs]
                for o in s.dp["outs"]:
                    o["n"] = n
                eng.dispatch_records(self.drules, ins, n, s.dp, stream=sd)
                outs = s.douts
            if self.match_any:
                # every line's published record and the views in which it owns exactly that one;
                # nothing of this waits for the previous chunk
                ins = [eng.json_in(kd, outs[name], lo, n, 2) for name, kd, _, _ in _KINDS if name in outs]
                eng.route_records(self.dtable, ins, n, s.rt["route"], s.rt["pick"], s.rt["views"], stream=sd)
                vins = [eng.json_in_view(ji, v) for ji, v in zip(ins, s.rt["views"])]
            if self.collapse:
                # only these small kernels wait for the previous chunk (its state pass, on the other
                # demodulation stream); this chunk's demodulation above is already enqueued beside it
                if self.rep_ev is not None:
                    sd.wait_event(self.rep_ev)
                ins = vins if self.match_any else [eng.json_in(kd, outs[name], lo, n, 2)
                                                   for name, kd, _, _ in _KINDS if name in outs]
                # the chunk's times and ids came up with its bytes (stage A, in front of the parse)
                self.repeats.enqueue(s.rb, ins, n, sd)
                self.rep_ev = t.cuda.Event()
                self.rep_ev.record(sd)
            skip = {"skip": s.rep} if self.collapse else {}
            jouts = outs
            if self.match_any:   # the match came first; the serialiser reads the picked views
                jouts = {name: dict(outs[name], desc=v) for name, v in zip(outs, s.rt["views"])}
                if s.rt["skip"] is not None:
                    eng.route_skip(vins, n, s.rt["route"], s.rt["skip"], drop_unrouted=True, stream=sd)
                    skip = {"skip": s.rt["skip"]}
            elif self.routes is not None:   # behind the repeat pass, in front of the serialiser
                ins = [eng.json_in(kd, outs[name], lo, n, 2) for name, kd, _, _ in _KINDS if name in outs]
                eng.route_lines(self.dtable, ins, n, s.rt["route"], None, s.rt["skip"], drop_unrouted=self.drop, stream=sd)
                if s.rt["skip"] is not None:
                    skip = {"skip": s.rt["skip"]}
            if self.output == "json":
                jo = s.jout
                runtime.fill_async(jo["cursor"], sd)
                runtime.fill_async(jo["len"][:n], sd)
                for name, kd, short, long_ in _KINDS:
                    o = jouts.get(name)
                    if o is not None and (cnt[short] or (long_ is not None and cnt[long_])):
                        eng.launch_json(kd, o, lo, n, jo, first_only=2, **skip)
                runtime.copy_async(s.h_sizes[:2], jo["cursor"], sd)
                runtime.copy_async(s.h_sizes[2:], s.cursors.reshape(-1), sd)
            elif self.all:
                # the chunk's line -> record-range index over all kinds (a repeat line counts 0), then one text per
                # record at its chunk index: one off / len / text buffer for the chunk
                ix = s.idx
                ins = [eng.json_in(kd, outs[name], lo, n, 0) for name, kd, _, _ in _KINDS if name in outs]
                eng.index_records(ins, n, ix, skip=s.rep if self.collapse else None, stream=sd)
                runtime.fill_async(ix["cursor"], sd)
                for name, kd, short, long_ in _KINDS:
                    o = outs.get(name)
                    if o is not None and (cnt[short] or (long_ is not None and cnt[long_])):
                        eng.launch_json_lines(kd, o, lo, n, ix)
                runtime.copy_async(s.h_sizes[:2], ix["cursor"], sd)
                runtime.copy_async(s.h_sizes[2:3], ix["first"][n: n + 1], sd)
                runtime.copy_async(s.h_sizes[3:], s.cursors.reshape(-1), sd)
            else:
                from . import dist as sdist
                parts = [sdist.Part(o["desc"], o["rec"], o["heap"], n, o["cursor"], kd, wire=o.get("wire"),
                                    xrec=o.get("xrec"))
                         for name, kd, _, _ in _KINDS for o in [s.outs.get(name)] if o is not None]
                wc = s.ser._count_pack_device(sdist._flatten(parts), sd)
                k = len(parts)
                runtime.copy_async(s.h_sizes[: runtime.XCHG_COUNTS * k], wc, sd)
                runtime.copy_async(s.h_sizes[runtime.XCHG_COUNTS * k:], s.cursors.reshape(-1), sd)
            e1.record(sd)
            ev = t.cuda.Event()
            ev.record(sd)
        s.demod_ev, s.ev = e1, ev
        s.kt += [e0, e1]
        s.stage = 2

    def _stage_c(self, s: _Slot):
        """The results D2H, sized by the device sizes (on the host by now)."""
        t = self.torch
        for r in self.done:                # an earlier chunk of this slot not yet handed out: copy it out
            if r.slot is s:
                r.detach()
        s.ev.synchronize()
        n, lb = s.n, s.lb
        hs = s.h_sizes.numpy().astype(np.int64)
        k = len(s.outs)
        with t.cuda.stream(self.cout):
            self.cout.wait_event(s.demod_ev)
            ho = s.h_out
            if self.output == "json":
                T = int(min(hs[0], s.jcap))
                s.ovf_json = bool(hs[1])
                s.dcur = hs[2:].reshape(k, 4)
                runtime.copy_d2h(ho[:T], s.jout["json"][:T], self.cout)
                a = (T + 3) & ~3
                runtime.copy_async(ho[a: a + 4 * n], s.jout["off"][:n], self.cout)
                runtime.copy_async(ho[a + 4 * n: a + 8 * n], s.jout["len"][:n], self.cout)
                b = a + 8 * n
                s.lay = (T, a)
            elif self.all:
                # the texts, first[: n + 1] and off / len[: total] -- record-indexed, all kinds' -- in the same sized copy
                T = int(min(hs[0], s.jcap))
                R = int(min(max(hs[2], 0), s.rec_max))
                s.ovf_json = bool(hs[1])
                s.dcur = hs[3:].reshape(k, 4)
                ix = s.idx
                runtime.copy_d2h(ho[:T], ix["json"][:T], self.cout)
                a = (T + 3) & ~3
                runtime.copy_async(ho[a: a + 4 * (n + 1)], ix["first"][: n + 1], self.cout)
                a2 = a + 4 * (n + 1)
                if R:
                    runtime.copy_async(ho[a2: a2 + 4 * R], ix["off"][:R], self.cout)
                    runtime.copy_async(ho[a2 + 4 * R: a2 + 8 * R], ix["len"][:R], self.cout)
                b = a2 + 8 * R
                s.lay = (T, a, R)
            else:
                from . import dist as sdist
                S = hs[: runtime.XCHG_COUNTS * k].reshape(1, k, runtime.XCHG_COUNTS)
                s.dcur = hs[runtime.XCHG_COUNTS * k:].reshape(k, 4)
                s.S = S
                offs, nb, T = sdist._layout(S)
                runtime.copy_d2h(ho[:T], s.ser._bufs["send"][:T], self.cout)
                b = T
                s.lay = (offs, nb, T)
            runtime.copy_async(ho[b: b + n], lb.kind[:n], self.cout)
            runtime.copy_async(ho[b + n: b + 2 * n], lb.status[:n], self.cout)
            s.kb = b
            if self.collapse:
                runtime.copy_async(ho[b + 2 * n: b + 3 * n], s.rep[:n], self.cout)
                self.d2h_bytes += n + (s.rb.h_read.numel() if s.rb.h_read is not None else 0)
            if self.routes is not None:
                s.rp = (b + (3 if self.collapse else 2) * n + 1) & ~1
                runtime.copy_async(ho[s.rp: s.rp + 2 * n], s.rt["route"][:n].view(t.uint8), self.cout)
                self.d2h_bytes += 2 * n
                if self.match_any:
                    runtime.copy_async(ho[s.rp + 2 * n: s.rp + 4 * n], s.rt["pick"][:n].view(t.uint8), self.cout)
                    self.d2h_bytes += 2 * n
            if s.src is not None:   # a submit_bytes chunk: the offsets the device found, for line(i)
                runtime.copy_async(s.h_offs[: n + 1], lb.offsets[: n + 1], self.cout)
                self.d2h_bytes += 8 * (n + 1)
            ev = t.cuda.Event()
            ev.record(self.cout)
        self.d2h_bytes += b + 2 * n
        s.ev = ev
        s.stage = 3

    def _collect(self, s: _Slot):
        s.ev.synchronize()
        n, b = s.n, s.kb
        ho = s.h_out.numpy()
        kind = ho[b: b + n]
        status = ho[b + n: b + 2 * n]
        r = ChunkResult(s.cid, n, kind, status)
        r.slot = s
        if s.src is not None:
            s.data, s.offsets = s.src, s.h_offs.numpy()[: n + 1]
        r.src_lines, r.src_data, r.src_offsets = s.lines, s.data, s.offsets
        self.kernel_events.append(tuple(s.kt))
        names = list(s.outs)
        redo_kinds = {names[j] for j in range(len(names)) if s.dcur[j, 2]}   # ST_OVF_* in that launch
        if self.output == "json":
            T, a = s.lay
            r.json = memoryview(ho[:T])
            r.off = ho[a: a + 4 * n].view(np.uint32)
            r.len = ho[a + 4 * n: a + 8 * n].view(np.uint32)
            if s.ovf_json:
                redo_kinds = set(names)            # the text buffer overflowed: the batch API for all
        elif self.all:
            T, a, R = s.lay
            a2 = a + 4 * (n + 1)
            r.json = memoryview(ho[:T])
            r.first = ho[a: a2].view(np.uint32)
            r.off = ho[a2: a2 + 4 * R].view(np.uint32)
            r.len = ho[a2 + 4 * R: a2 + 8 * R].view(np.uint32)
            r.overflow = s.ovf_json
            if s.ovf_json:
                redo_kinds = set(names)            # the texts or the index overflowed: the batch API for all
        else:
            r.wire = ho[: s.lay[2]]
            r.layout = s.lay
            r.affix = {j: self.bank.affixes(kd) for j, (name, kd, _, _) in
                       enumerate(x for x in _KINDS if x[0] in s.outs)}
            r.names = names
            if s.S[0, :, 3].any():
                redo_kinds |= {names[j] for j in range(len(names)) if s.S[0, j, 3]}
        # the lines the fast path does not finish: the batch API on those lines only
        kname = {runtime.LINE_MU: "MU", runtime.LINE_MS: "MS", runtime.LINE_MC: "MC", runtime.LINE_MN: "MN"}
        rows = set(np.nonzero((status == runtime.LS_GENERAL) | (status == runtime.LS_UNSUPPORTED))[0].tolist())
        rows |= set(s.bad)
        if redo_kinds:
            for kk, name in kname.items():
                if name in redo_kinds:
                    rows |= set(np.nonzero((kind == kk) & (status == runtime.LS_OK))[0].tolist())
        if rows:
            rows = sorted(rows)
            lines = [self._line(s, i) for i in rows]
            host_picks = None
            pkw = self._profile_args(s, rows)
            if self.match_any and self.output == "json":   # the picked messages' texts, with their routes and picks
                res = [x[1] if isinstance(x, tuple) else x
                       for x in self.parser.parse_lines_routed(lines, self.routes, route_match="any", **pkw)]
                host_picks = dict(zip(rows, zip(self.parser.last_picks.tolist(), self.parser.last_routes.tolist())))
            elif self.all:   # every message's text, through the same passes on the host-resolved lines alone
                res = self.parser.parse_lines_json_all(lines, dispatch=self.rules, **pkw)
            else:
                res = (self.parser.parse_lines_json(lines, **pkw) if self.output == "json" else self.parser.parse_lines(lines))
            for i, x in zip(rows, res):
                r.host[i] = s.bad[i] if i in s.bad else x
        if self.routes is not None:   # the device's routes; a host-resolved line's from the same tables on the host
            r.route = ho[s.rp: s.rp + 2 * n].view(np.int16)
            if self.match_any:
                r.pick = ho[s.rp + 2 * n: s.rp + 4 * n].view(np.uint16)
                for i, x in r.host.items():
                    if self.output == "json":
                        r.pick[i], r.route[i] = host_picks[i] if isinstance(x, str) else (0, -1)
                    else:
                        r.pick[i], r.route[i], _ = self.routes.pick([m.payload for m in x] if isinstance(x, list) else [])
            else:
                for i, x in r.host.items():
                    r.route[i] = self._host_route(x)
        if s.sources is not None:
            r.source = s.sources.copy()
        if self.collapse:
            self._fix_repeats(s, r, ho[b + 2 * n: b + 3 * n], redo_kinds, kname)
        if self.drop and self.output == "json":   # published = result-bearing, no repeat, routed
            if not self.device_drop:
                r.len[(r.len > 0) & (r.route < 0)] = 0
            for i, x in r.host.items():           # host rows, and lines republished behind one
                if isinstance(x, str) and r.route[i] < 0:
                    r.host[i] = None
        self.done.append(r)
        self.inflight.remove(s)
        s.reset()
        s.stage = 0

    def _profile_args(self, s: _Slot, rows) -> dict:
        """The batch API's profile arguments for the lines ``rows`` of a chunk: a host-resolved line is filtered by
        the same table (profiles.ReceiverProfiles.filter and the one-shot calls' own pass)."""
        if self.profiles is None:
            return {}
        return {"profiles": self.profiles, "sources": None if s.sources is None else [int(s.sources[i]) for i in rows]}

    def _host_route(self, x) -> int:
        """The route of a host-resolved line from its batch-API result (a text, or parse_lines' list)."""
        if isinstance(x, str):
            return self.routes.match(json.loads(x)["payload"])[0]
        if isinstance(x, list) and x:
            return self.routes.match(x[0].payload)[0]
        return -1

    def _fix_repeats(self, s: _Slot, r: ChunkResult, rep: np.ndarray, redo_kinds, kname) -> None:
        """r.repeat = the chunk's exact mask: the device's, re-decided around the host-resolved rows
        (repeats.RepeatTracker); texts and host results follow it."""
        from .repeats import apply_mask, objects_key, text_key
        n, kind, js, al = r.n, r.kind, self.output == "json", self.all
        name_of = lambda i: kname.get(int(kind[i]), "?")   # noqa: E731
        picked = lambda i, x: x[int(r.pick[i]): int(r.pick[i]) + 1] if r.pick is not None and isinstance(x, list) else x   # noqa: E731
        # json_all: a line's key is that of its first text, which the dispatch rules never remove
        list_key = lambda i, x: text_key(name_of(i), x[0]) if isinstance(x, list) and x else None   # noqa: E731
        host_keys = {i: (list_key(i, x) if al else (text_key(name_of(i), x) if isinstance(x, str) else None) if js
                         else objects_key(picked(i, x)))
                     for i, x in r.host.items()}
        redo = [i for i in r.host if redo_kinds and kname.get(int(kind[i])) in redo_kinds
                and r.status[i] == runtime.LS_OK]
        fetched = {}

        def one_text(i):       # the line's published text on its own (route_match="any": the picked message's)
            pkw = self._profile_args(s, [i])
            if al:             # json_all: the line's list
                return self.parser.parse_lines_json_all([self._line(s, i)], dispatch=self.rules, **pkw)[0]
            if not self.match_any:
                return self.parser.parse_lines_json([self._line(s, i)], **pkw)[0]
            x = self.parser.parse_lines_routed([self._line(s, i)], self.routes, route_match="any", **pkw)[0]
            return x[1] if isinstance(x, tuple) else x

        def fetch(i):
            fetched[i] = one_text(i)
            if al:
                return list_key(i, fetched[i])
            return text_key(name_of(i), fetched[i]) if isinstance(fetched[i], str) else None

        if al:
            first = r.first.astype(np.int64)
            has_key = np.diff(first) > 0     # a repeat the device skipped has no range, as it has no text in a json chunk
            blob = r.json

            def dev_key_of(i):
                c = int(first[i])
                o = int(r.off[c])
                return text_key(name_of(i), bytes(blob[o: o + int(r.len[c])]).decode("ascii"))
        elif js:
            has_key = r.len > 0
            blob = r.json

            def dev_key_of(i):
                o = int(r.off[i])
                return text_key(name_of(i), bytes(blob[o: o + int(r.len[i])]).decode("ascii"))
        else:
            has_key, dev_key_of = self._wire_keys(r)
        r.repeat = mask = self.repeats.exact_mask(s.rb, rep, has_key, dev_key_of, host_keys, redo, fetch,
                                                  times=s.times, sources=self._rsrc(r.source), bank=self.bank)
        if not (js or al):
            return

        def drop(i):
            if i in r.host:
                r.host[i] = [] if al else None
            elif al:
                r.len[int(first[i]): int(first[i + 1])] = 0   # every record of the line
            else:
                r.len[i] = 0           # a repeat of a host-resolved line: its text is not published

        def republish(i):              # skipped on the device, but its predecessor was a host row
            r.host[i] = fetched[i] if i in fetched else one_text(i)
        apply_mask(mask, rep, host_keys, drop, republish)

    def _wire_keys(self, r: ChunkResult):
        """wire output: (which lines have results, line -> key) from the chunk's wire sections; the
        sections of a kind are decoded when a key of that kind is first asked for."""
        names = list(r.names)
        tabs = {"MU": self.bank.mu_pids, "MS": self.bank.ms_pids, "MC": self.bank.mc_pids, "MN": self.bank.mn_pids}
        line_kind = {"MU": runtime.LINE_MU, "MS": runtime.LINE_MS, "MC": runtime.LINE_MC, "MN": runtime.LINE_MN}
        has = np.zeros(r.n, bool)
        for j, name in enumerate(names):
            msg = r.sections(j)[0]
            has |= ((msg & 0xFFFF) > 0) & (((msg >> 16) & 0xFF) == runtime.ST_OK) & (r.kind == line_kind[name])
        cache = {}

        def key_of(i):
            name = {v: k for k, v in line_kind.items()}[int(r.kind[i])]
            if name not in cache:
                cache[name] = r.decode(names.index(name))
            desc, rec, heap = cache[name]
            x = rec[int(desc["rec_begin"][i]) + (0 if r.pick is None else int(r.pick[i]))]
            o = int(x["payload_off"])
            return (name, str(tabs[name][int(x["proto"])]), heap[o: o + int(x["payload_len"])].tobytes().decode("latin-1"))
        return has, key_of

    @staticmethod
    def _line(s: _Slot, i: int):
        if s.lines is not None:
            return s.lines[i]
        if isinstance(s.data, _ChunkBytes):
            return s.data.slice(int(s.offsets[i]), int(s.offsets[i + 1]))
        d = s.data.numpy() if hasattr(s.data, "numpy") else s.data   # a pinned torch tensor or numpy
        return d[int(s.offsets[i]): int(s.offsets[i + 1])].tobytes()
