"""Wire-line front end: raw SIGNALduino firmware lines -> DecodedMessage, on the GPU.

Mirrors the reference's parser entry point, ``signalduino.parser.SignalParser``
(signalduino/parser/__init__.py:18-77), and its data types ``RawFrame`` / ``DecodedMessage``
(signalduino/types.py:13-32).  Per line the reference runs, in Python: strip + STX/ETX framing,
Mred=1 decompression, routing by message type, the MU validity regex, ``_parse_to_dict``, the MC
header checks, then ``SDProtocols.demodulate*``.  Here a batch of lines is uploaded once and
  1. ``sdx_parse_lines``   (csrc/sdx_lines.hip) does all of the parsing, one lane per line, writing
                           the demodulators' SoA batch in place (slot layout, ``len_dev``),
  2. ``sdx_select_lines``  builds the per-kind selection lists (MU/MS short or long, MC) on the device,
  3. the MU / MS / MN (and, in mc_mode='fixed', MC) demodulation kernels run over those lists,
and only the result records come back.  The host side assembles the Python objects.

Observable behaviour per line is the reference's: ``parse_line`` returns the same
``DecodedMessage`` list (protocol_id, payload, metadata, raw.line / message_type / rssi /
freq_afc), and lines the reference ignores give ``[]`` (a demodulator exception is caught and
logged by the reference's parsers, so it also gives ``[]``).  Pattern values are the reference's
``float()`` in full: what sdx_parse_lines' one-operation conversion leaves open, sdx_lines_exact
converts correctly rounded (csrc/sdx_strtod.h).  Lines outside the device contract (non-ASCII
characters after decompression, pattern ids of more than 15 digits, more than 16 patterns, an R= /
F= of more than 15 characters, an MC C= / L= beyond int32) are never approximated: ``parse_line``
raises :class:`ContractError` and ``parse_lines`` returns the exception in that line's slot.
There is no CPU fallback.
"""
from __future__ import annotations

import json
import logging
import re
from dataclasses import dataclass, field
from datetime import datetime
from typing import Any, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import runtime
from .packing import ContractError
from .sd_protocols import SDProtocols

_KIND_NAME = {runtime.LINE_MU: "MU", runtime.LINE_MS: "MS", runtime.LINE_MC: "MC", runtime.LINE_MN: "MN"}


@dataclass(slots=True)
class RawFrame:
    """signalduino/types.py:13-21."""

    line: str
    timestamp: datetime = field(default_factory=datetime.utcnow)
    rssi: Optional[float] = None
    freq_afc: Optional[float] = None
    message_type: Optional[str] = None


@dataclass(slots=True)
class DecodedMessage:
    """signalduino/types.py:24-31."""

    protocol_id: str
    payload: str
    raw: RawFrame
    metadata: dict = field(default_factory=dict)


def calc_rssi(raw_rssi: int) -> float:
    """parser/base.py calc_rssi."""
    if raw_rssi >= 128:
        return ((raw_rssi - 256) / 2) - 74
    return (raw_rssi / 2) - 74


def calc_afc(raw_afc: int) -> float:
    """parser/base.py calc_afc."""
    if raw_afc >= 128:
        return (raw_afc - 256) / 2
    return raw_afc / 2


def calc_mn_afc(raw_afc: int) -> float:
    """parser/mn.py:60-68 (the MN frame's A= field)."""
    return round((26000000 / 16384 * raw_afc / 1000), 0)


MN_PATTERN = re.compile(r"^MN;D=(Y?)([0-9A-F]+);(?:R=([0-9]+);)?(?:A=(-?[0-9]{1,3});)?$")  # parser/mn.py:17


def _to_bytes(line: Union[str, bytes]) -> bytes:
    if isinstance(line, (bytes, bytearray, memoryview)):
        return bytes(line)
    try:
        return line.encode("latin-1")  # the transport's decoding (transport.py:123), inverted
    except UnicodeEncodeError as e:
        raise ContractError("characters above U+00FF cannot come from the firmware transport") from e


class LineBatch:
    """Device buffers of one parsed batch (sdx_lines / sdx_lines_out of include/sdx.h)."""

    def __init__(self, eng: "runtime.Engine", data: np.ndarray, offsets: np.ndarray):
        t = eng.torch
        # 16 bytes of padding: the kernel reads whole aligned 8-byte words (include/sdx.h)
        self._alloc(eng, t.from_numpy(np.concatenate([data, np.zeros(16, np.uint8)])).to(eng.dev),
                    t.from_numpy(offsets).to(eng.dev), len(offsets) - 1, int(offsets[-1]))

    @classmethod
    def from_device(cls, eng: "runtime.Engine", bytes_dev, offsets_dev, n: int, total: int) -> "LineBatch":
        """A batch over lines already on the device: ``bytes_dev`` (uint8, 16 readable bytes past
        ``total``) and ``offsets_dev`` (int64[n + 1], offsets[n] = total), e.g. what sdx_split_lines wrote."""
        lb = cls.__new__(cls)
        lb._alloc(eng, bytes_dev, offsets_dev, int(n), int(total))
        return lb

    def _alloc(self, eng: "runtime.Engine", bytes_dev, offsets_dev, n: int, total: int) -> None:
        t = eng.torch
        d = eng.dev
        self.n = n
        self.eng = eng
        self.bytes = bytes_dev
        self.offsets = offsets_dev
        e = lambda k, dt: t.empty(max(k, 1), dtype=dt, device=d)  # noqa: E731
        self.kind, self.status = e(n, t.uint8), e(n, t.uint8)
        self.slot = t.empty(3 * total + 16, dtype=t.uint8, device=d)
        self.doff, self.dlen = e(n, t.int64), e(n, t.int32)
        self.npat, self.pat_id, self.pat_val = e(n, t.uint8), e(10 * n, t.uint8), e(10 * n, t.float64)
        self.cp_slot, self.ms_ok = e(n, t.int8), e(n, t.uint8)
        self.clock, self.mcbitnum, self.mcflags = e(n, t.int32), e(n, t.int32), e(n, t.uint8)
        self.meta, self.plen = e(32 * n, t.uint8), e(n, t.int32)
        self.sel = e(n, t.int32)
        self.counts = t.zeros(8, dtype=t.int32, device=d)
        self.scratch = e(8 * ((n + runtime.SEL_CHUNK - 1) // runtime.SEL_CHUNK), t.int32)
        p = runtime._ptr
        self.c_lines = runtime.SdxLines(p(self.bytes), p(self.offsets), n)
        self.c_out = runtime.SdxLinesOut(p(self.kind), p(self.status), p(self.slot), p(self.doff), p(self.dlen),
                                         p(self.npat), p(self.pat_id), p(self.pat_val), p(self.cp_slot),
                                         p(self.ms_ok), p(self.clock), p(self.mcbitnum), p(self.mcflags),
                                         p(self.meta), p(self.plen))

    def launch(self) -> None:
        """sdx_parse_lines + sdx_select_lines on the engine's current stream (no host sync)."""
        import ctypes
        lib, st = self.eng.lib, self.eng.stream_ptr()
        runtime._check(lib, lib.sdx_parse_lines(ctypes.byref(self.c_lines), ctypes.byref(self.c_out), st))
        runtime._check(lib, lib.sdx_select_lines(ctypes.byref(self.c_out), self.n, runtime._ptr(self.sel),
                                                 runtime._ptr(self.counts), runtime._ptr(self.scratch), st))

    def selections(self):
        """Class sizes (one 32-byte read-back) -> device sub-lists of sel per class."""
        cnt = self.counts.cpu().numpy()[: runtime.SEL_NCLASS]
        start = np.concatenate([[0], np.cumsum(cnt)])
        return [self.sel[int(start[k]): int(start[k + 1])] for k in range(runtime.SEL_NCLASS)], cnt

    def mc_all(self, cnt):
        """Every MC line's index (the short and the long class: adjacent in sel) and their count."""
        a = int(np.sum(cnt[: runtime.SEL_MC]))
        k = int(cnt[runtime.SEL_MC]) + int(cnt[runtime.SEL_MC_LONG])
        return self.sel[a: a + k], k

    def pulse_batch(self):
        return {"data": self.slot, "offsets": self.doff, "npat": self.npat, "pat_id": self.pat_id,
                "pat_val": self.pat_val, "cp_slot": self.cp_slot, "ms_ok": self.ms_ok, "len": self.dlen, "n": self.n}

    def mn_batch(self):
        return {"hex": self.slot, "offsets": self.doff, "len": self.dlen, "n": self.n}

    def general(self, status: np.ndarray, kind_np: np.ndarray, line_kind: int):
        """The SDX_LS_GENERAL lines of one kind through sdx_lines_general + sdx_demod_pulses_general,
        together with the kind's SDX_LS_UNSUPPORTED lines that sdx_lines_exact resolves (P# values that
        need the exact float(): they become SDX_LS_GENERAL rows of the same batch).
        Returns (rows, desc, rec, heap, vals [rows, 16], cp_slot) or None when there are none; status is
        updated in place: resolved rows turn GENERAL, rows the general parse found outside the contract
        turn UNSUPPORTED (both kinds of UNSUPPORTED rows are left out of the returned batch)."""
        import ctypes
        of_kind = kind_np == line_kind
        rows_g = np.nonzero((status == runtime.LS_GENERAL) & of_kind)[0]
        rows_x = np.nonzero((status == runtime.LS_UNSUPPORTED) & of_kind)[0]
        rows = np.concatenate([rows_g, rows_x])
        if not len(rows):
            return None
        t, d, eng = self.eng.torch, self.eng.dev, self.eng
        m, mg = len(rows), len(rows_g)
        sel = t.from_numpy(rows.astype(np.int32)).to(d)
        g = {"offsets": t.empty(m, dtype=t.int64, device=d), "len": t.empty(m, dtype=t.int32, device=d),
             "npat": t.empty(m, dtype=t.uint8, device=d), "pat_ids": t.empty(m * 256, dtype=t.uint8, device=d),
             "pat_val": t.empty(m * 16, dtype=t.float64, device=d), "cp_slot": t.empty(m, dtype=t.int8, device=d),
             "ms_ok": t.empty(m, dtype=t.uint8, device=d)}
        p = runtime._ptr
        width = {"pat_ids": 256, "pat_val": 16}

        def part(a, b):   # rows [a, b) of the batch as an sdx_lines_general_out
            return runtime.SdxLinesGeneralOut(*(p(g[k][a * width.get(k, 1): b * width.get(k, 1)])
                                                for k in ("offsets", "len", "npat", "pat_ids", "pat_val", "cp_slot", "ms_ok")))
        if mg:
            runtime._check(eng.lib, eng.lib.sdx_lines_general(ctypes.byref(self.c_lines), ctypes.byref(self.c_out),
                                                              p(sel[:mg]), mg, ctypes.byref(part(0, mg)), eng.stream_ptr()))
        if m > mg:
            runtime._check(eng.lib, eng.lib.sdx_lines_exact(ctypes.byref(self.c_lines), ctypes.byref(self.c_out),
                                                            p(sel[mg:]), m - mg, ctypes.byref(part(mg, m)), eng.stream_ptr()))
        st = self.status[sel.long()].cpu().numpy()
        status[rows] = st                                   # resolved lines, lines found outside the contract
        keep = np.nonzero(st == runtime.LS_GENERAL)[0]
        if not len(keep):
            return None
        if len(keep) < m:
            kd_ = t.from_numpy(keep).to(d)
            g = {k: v.view(m, -1)[kd_].reshape(-1).contiguous() for k, v in g.items()}
            rows, m = rows[keep], len(keep)
        lens = g["len"].cpu().numpy()
        g.update(data=self.slot, n=m, total=int(lens.sum()), lens_host=lens)
        kd = runtime.KIND_MU if line_kind == runtime.LINE_MU else runtime.KIND_MS
        desc, rec, heap = eng.run_general(kd, g, work_stride=5 * (int(lens.max()) + 512))
        return (rows, desc, rec, heap, g["pat_val"].cpu().numpy().reshape(m, 16),
                g["cp_slot"].cpu().numpy().astype(np.int64))

    def mc_batch(self):
        return {"hex": self.slot, "offsets": self.doff, "clock": self.clock, "mcbitnum": self.mcbitnum,
                "flags": self.mcflags, "len": self.dlen, "n": self.n}


def _check_route_match(route_match, routes) -> None:
    """The ``route_match`` argument of parse_lines_routed / stream: "first" or "any", the latter only with routes."""
    if route_match not in ("first", "any"):
        raise ValueError(f"route_match must be 'first' or 'any', not {route_match!r}")
    if route_match == "any" and routes is None:
        raise ValueError("route_match='any' needs routes")


def _contract(i: int, name) -> ContractError:
    """The slot value of a line whose demodulation hit a device limit (SDX_RAISE_CONTRACT): not a
    reference outcome, so it is reported, never turned into an empty result list."""
    return ContractError(f"line {i} ({name}) exceeds a limit of the device's general path "
                         "(include/sdx.h SDX_GEN_*, payloads > 65535 bytes)")


def _outside_contract(i: int, kind) -> ContractError:
    """The slot value of a line the front end's kernel does not take (SDX_LS_UNSUPPORTED), ``kind`` its line kind."""
    return ContractError(f"line {i} is outside the device contract of the front end "
                         f"(kind {_KIND_NAME.get(int(kind), '?')})")


def pack_lines(lines: Sequence[Union[str, bytes]], copy: bool = True):
    """Concatenate lines into (data uint8, offsets int64[n+1]); per-line ContractError where a line
    cannot be represented (returned in ``bad``; such lines are replaced by an empty line).
    ``copy=False``: data is a read-only view of the joined bytes (one host copy fewer)."""
    if lines and set(map(type, lines)) == {str}:
        # all str (what the transports deliver): one join and one latin-1 encode for the whole batch
        # (a str's latin-1 bytes are as many as its characters); any character above U+00FF sends
        # the batch to the per-line path below, which marks just those lines
        try:
            blob = "".join(lines).encode("latin-1")
        except UnicodeEncodeError:
            blob = None
        if blob is not None:
            offsets = np.zeros(len(lines) + 1, np.int64)
            np.cumsum(np.fromiter(map(len, lines), np.int64, len(lines)), out=offsets[1:])
            data = np.frombuffer(blob, np.uint8)
            return (data.copy() if copy else data), offsets, {}
    bs, bad = [], {}
    for i, ln in enumerate(lines):
        try:
            bs.append(_to_bytes(ln))
        except ContractError as e:
            bad[i] = e
            bs.append(b"")
    lens = np.fromiter((len(b) for b in bs), np.int64, len(bs))
    offsets = np.zeros(len(bs) + 1, np.int64)
    np.cumsum(lens, out=offsets[1:])
    data = np.frombuffer(b"".join(bs), np.uint8)
    return (data.copy() if copy else data), offsets, bad


class _LinesView:
    """The lines of a split byte buffer as a read-only sequence: line i = raw[offsets[i]: offsets[i + 1]]
    (with its terminator), sliced on demand -- no list of a million bytes objects."""

    def __init__(self, raw, offsets: np.ndarray):
        self.raw, self.offsets = raw, offsets

    def __len__(self) -> int:
        return len(self.offsets) - 1

    def __getitem__(self, i: int) -> bytes:
        if not 0 <= i < len(self):
            raise IndexError(i)
        return bytes(self.raw[int(self.offsets[i]): int(self.offsets[i + 1])])


def lines_of(data: bytes, final: bool = True):
    """What the byte-stream entries take as the lines of ``data``: data.split(b"\\n") without its last
    element when that is empty or ``final`` is false -> (lines, tail); the tail is b"" unless final is false."""
    parts = bytes(data).split(b"\n")
    last = parts.pop()
    if final and last:
        parts.append(last)
        last = b""
    return parts, last


class SignalParser:
    """signalduino/parser/__init__.py:18-77 with the whole line -> DecodedMessage path on the GPU."""

    def __init__(self, protocols: Optional[SDProtocols] = None, logger: Optional[logging.Logger] = None,
                 rfmode: Optional[str] = None):
        self.protocols = protocols or SDProtocols()
        self.logger = logger or logging.getLogger(__name__)
        self.protocols.register_log_callback(self._log_adapter)
        self.rfmode = rfmode

    def _log_adapter(self, message: str, level: int):
        if level <= 1:
            self.logger.error(message)
        elif level == 2:
            self.logger.warning(message)
        elif level == 3:
            self.logger.info(message)
        else:
            self.logger.debug(message)

    # ------------------------------------------------------------------------------------------
    def parse_line(self, line: Union[str, bytes]) -> List[DecodedMessage]:
        """SignalParser.parse_line (parser/__init__.py:37-49)."""
        out = self.parse_lines([line])[0]
        if isinstance(out, BaseException):
            raise out
        return out

    @staticmethod
    def _window_args(collapse: bool, times, repeat_window, n: int, sources=None):
        """-> (times as int64[n], W in microseconds), (None, None) without a window; ValueError for a window
        without collapse_repeats or without times, and for times that decrease (repeats.py) -- with
        ``sources`` (repeats.check_sources' array) within a source."""
        if repeat_window is None:
            if times is not None and len(times) != n:
                raise ValueError(f"times: {len(times)} times for {n} lines")
            return None, None
        from .repeats import check_times, window_to_us
        if not collapse:
            raise ValueError("repeat_window needs collapse_repeats=True")
        w = window_to_us(repeat_window)
        return check_times(times, n, sources=sources), w

    @staticmethod
    def _source_args(collapse: bool, sources, n: int, profiles=None):
        """-> the lines' source ids as int32[n], None without ``sources``; ValueError without
        collapse_repeats or ``profiles`` and for ids that are no integers inside [0, 4096) (repeats.py) --
        with ``profiles`` (a profiles.ReceiverProfiles) inside its table's [0, S), and for a table of several
        sources without ids."""
        if sources is None:
            if profiles is not None and profiles.n_sources > 1:
                raise ValueError(f"profiles for {profiles.n_sources} sources need the lines' source ids (sources=)")
            return None
        if not collapse and profiles is None:
            raise ValueError("sources needs collapse_repeats=True or profiles")
        from .repeats import check_sources
        return check_sources(sources, n, None if profiles is None else profiles.n_sources)

    def _mn_elig(self, profiles=None) -> int:
        """sdx_mn_batch.elig: the parser's rfmode, and with ``profiles`` only what some profile enables."""
        elig = self.protocols.mn_eligibility(self.rfmode)
        return elig if profiles is None else elig & profiles.mn_elig(self.protocols._bank)

    def parse_lines(self, lines: Sequence[Union[str, bytes]], collapse_repeats: bool = False, times=None,
                    repeat_window: Optional[float] = None, sources=None,
                    profiles=None, dispatch=None) -> List[Union[List[DecodedMessage], Exception]]:
        """Batch form of parse_line: one upload, one parse launch, one launch per demodulation
        variant, one read-back.  Returns one DecodedMessage list per line (or the ContractError
        for a line outside the device contract).  ``collapse_repeats``: a line that repeats the
        previous result-bearing line's (kind, protocol, payload) gives [] (repeats.py; the mask is
        left in ``last_repeat_mask``).  ``repeat_window`` (seconds) with ``times`` (one arrival time in
        integer microseconds per line, non-decreasing): a run also ends once its last published line
        is more than the window old, as FHEM dispatches (repeats.py).  ``sources`` (one integer id per
        line, the receiver it came from): every source's lines are a stream of their own -- runs, keys and
        the window's anchor per source, the times non-decreasing within a source.  ``profiles`` (a
        profiles.ReceiverProfiles, a Profile or a list of them): every line keeps only the messages
        whose protocol its source's profile enables (``sources``: the ids, also without collapse_repeats; a table
        of one source needs none) -- filtered on the device (sdx_filter_records) before anything is read back.
        ``dispatch`` (a dispatch.DispatchRules, or True for FHEM's defaults): every line's list reduced
        by the dispatch rules -- at most ``max_repeat`` messages of one protocol in a row, a message equal to the one
        before it dropped -- on the device (sdx_dispatch_records), behind the profile pass and in front of
        ``collapse_repeats``; a line's first message always stays."""
        from .dispatch import as_rules
        from .profiles import as_profiles
        dispatch = as_rules(dispatch)
        profiles = as_profiles(profiles)
        sources = self._source_args(collapse_repeats, sources, len(lines), profiles)
        times, w = self._window_args(collapse_repeats, times, repeat_window, len(lines), sources)
        if len(lines) == 0:
            return self._collapsed([], collapse_repeats)
        data, offsets, bad = pack_lines(lines)
        return self._collapsed(self._objects(lines, LineBatch(self.protocols._ensure(), data, offsets), offsets, bad,
                                             len(data), profiles, sources, dispatch), collapse_repeats, times, w,
                               sources if collapse_repeats else None)

    def _collapsed(self, out: list, collapse: bool, times=None, window_us=None, sources=None) -> list:
        """Object output: every payload is on the host already, so the repeats are marked there."""
        if collapse:
            from .repeats import collapse_objects
            self.last_repeat_mask = collapse_objects(out, times, window_us, sources=sources)
        return out

    def _objects(self, lines, lb: LineBatch, offsets: np.ndarray, bad: dict, nbytes: int, profiles=None, sources=None,
                 dispatch=None):
        """parse_lines from the uploaded batch on: ``lines`` indexable (lines[i] = line i's text),
        ``offsets`` the host copy of lb.offsets, ``nbytes`` = offsets[n].  ``profiles`` / ``sources``: the
        launches' results go through sdx_filter_records before the objects are built from them; ``dispatch`` (a
        dispatch.DispatchRules): then through sdx_dispatch_records."""
        n = len(lines)
        eng = self.protocols._ensure()
        bk = self.protocols._bank
        lb.launch()
        sels, cnt = lb.selections()
        res = {}
        pb = lb.pulse_batch()
        if cnt[runtime.SEL_MU_SHORT] or cnt[runtime.SEL_MU_LONG]:
            res["MU"] = eng.run(runtime.KIND_MU, pb, sel_short=sels[runtime.SEL_MU_SHORT],
                                sel_long=sels[runtime.SEL_MU_LONG])
        if cnt[runtime.SEL_MS_SHORT] or cnt[runtime.SEL_MS_LONG]:
            res["MS"] = eng.run(runtime.KIND_MS, pb, sel_short=sels[runtime.SEL_MS_SHORT],
                                sel_long=sels[runtime.SEL_MS_LONG])
        mc_sel, mc_n = lb.mc_all(cnt)
        if self.protocols.mc_mode == "fixed" and mc_n:
            res["MC"] = eng.run(runtime.KIND_MC, lb.mc_batch(), sel_short=mc_sel)
        if cnt[runtime.SEL_MN]:
            # result space: <= (MN protocols) records of <= (preamble + frame) bytes per line
            nmn = int(cnt[runtime.SEL_MN])
            res["MN"] = eng.run(runtime.KIND_MN, lb.mn_batch(), sel_short=sels[runtime.SEL_MN],
                                mn_elig=self._mn_elig(profiles),
                                rec_cap=len(bk.mn_pids) * nmn + 1024, heap_cap=int(4 * nbytes + 64 * nmn + 65536))
        if profiles is not None and res:
            res = eng.filter_fetched(profiles, res, n, sources)
        if dispatch is not None and res:
            res = eng.dispatch_fetched(dispatch, res, n)
        # read-back of the per-line fields the Python objects need
        kind = lb.kind[:n].cpu().numpy()
        status = lb.status[:n].cpu().numpy()
        # SDX_LS_GENERAL lines (multi-digit pattern ids, > 4096 pulses): the general path
        gen = {name: lb.general(status, kind, lk) for name, lk in (("MU", runtime.LINE_MU), ("MS", runtime.LINE_MS))}
        gen_of = {}
        for name, gr in gen.items():
            if gr is not None:
                for j, i in enumerate(gr[0]):
                    gen_of[int(i)] = (name, j)
        plen = lb.plen[:n].cpu().numpy()
        meta = lb.meta[: 32 * n].cpu().numpy().reshape(n, 32)
        need_slot = plen >= 0
        slot = lb.slot.cpu().numpy() if need_slot.any() else None
        ms_clock = None
        if "MS" in res:
            pv = lb.pat_val[: 10 * n].cpu().numpy().reshape(n, 10)
            cps = lb.cp_slot[:n].cpu().numpy().astype(np.int64)
            ok_ms = (kind == runtime.LINE_MS) & (status == runtime.LS_OK)  # cp_slot is written for these
            cps = np.where(ok_ms, np.clip(cps, 0, 9), 0)
            ms_clock = np.abs(pv[np.arange(n), cps])
        # the host assembly reads Python lists / str slices, not numpy rows: one bulk conversion per
        # array instead of a numpy scalar access per field (the per-line objects dominate this path)
        cols = {}
        for k, (desc, rec, heap) in res.items():
            cols[k] = (desc["status"].tolist(), desc["raise_kind"].tolist(), desc["n_rec"].tolist(),
                       desc["rec_begin"].tolist(), rec["proto"].tolist(), rec["payload_off"].tolist(),
                       rec["payload_len"].tolist(), rec["bit_length"].tolist(), heap.tobytes().decode("latin-1"))
        mb = meta.tobytes()
        sb = slot.tobytes() if slot is not None else b""
        hb_mn = res["MN"][2].tobytes() if "MN" in res else b""
        status_l, kind_l, plen_l, off_l = status.tolist(), kind.tolist(), plen.tolist(), offsets.tolist()
        ms_clock_l = ms_clock.tolist() if ms_clock is not None else None
        mu_pids, ms_pids, mc_pids, mu_clock = bk.mu_pids, bk.ms_pids, bk.mc_pids, bk.mu_clock
        ST_OK, ST_RAISED, R_CONTRACT = runtime.ST_OK, runtime.ST_RAISED, runtime.RAISE_CONTRACT
        out: List[Any] = []
        for i in range(n):
            if i in bad:
                out.append(bad[i])
                continue
            st = status_l[i]
            if st == runtime.LS_UNSUPPORTED:
                out.append(_outside_contract(i, kind_l[i]))
                continue
            name = _KIND_NAME.get(kind_l[i])
            if st == runtime.LS_GENERAL:
                gname, j = gen_of[i]
                _, gdesc, grec, gheap, gvals, gcps = gen[gname]
                g = self._general_messages(lines[i], i, plen, offsets, slot, meta, gname, gdesc[j], grec,
                                           gheap.tobytes(), abs(float(gvals[j, max(0, int(gcps[j]))])))
                if profiles is not None and isinstance(g, list):   # the general path's lists are built on the host
                    g = profiles.filter(bk, 0 if sources is None else int(sources[i]), gname, g)
                if dispatch is not None and isinstance(g, list):
                    g = dispatch.reduce(bk, gname, g)
                out.append(g)
                continue
            if st != runtime.LS_OK or name not in res:
                out.append([])
                continue
            d_st, d_rk, d_nr, d_rb, r_p, r_off, r_len, r_bl, hs = cols[name]
            dst = d_st[i]
            if dst == ST_RAISED and d_rk[i] == R_CONTRACT:
                out.append(_contract(i, name))   # a device limit (MC frames > 128 hex: k_mc_general)
                continue
            nr = d_nr[i]
            if dst == ST_RAISED or nr == 0:
                out.append([])  # a demodulator exception is caught by the reference's parsers
                continue
            if dst != ST_OK:
                raise RuntimeError(f"device status {dst} for line {i}")
            if name == "MN":
                out.append(self._mn_messages(lines[i], i, plen, offsets, slot, meta, res[name][0][i], res[name][1],
                                             hb_mn))
                continue
            # RawFrame(line=payload) + _extract_metadata (mu.py:96-108, mc.py:141-155)
            pl = plen_l[i]
            if pl >= 0:
                s0 = 3 * off_l[i]
                payload_line = sb[s0: s0 + pl].decode("latin-1")
            else:
                ln = lines[i]
                payload_line = (ln.decode("latin-1") if isinstance(ln, (bytes, bytearray, memoryview)) else ln).strip()[1:-1]
            fr = RawFrame(line=payload_line, message_type=name)
            m0 = 32 * i
            rl, fl = mb[m0 + 15], mb[m0 + 31]
            rssi_raw = None if rl == 255 else mb[m0: m0 + rl].decode("latin-1")
            if rssi_raw is not None:
                try:
                    fr.rssi = calc_rssi(int(rssi_raw))
                except ValueError:
                    self.logger.warning("Could not parse %s value: %s", "RSSI", rssi_raw)
            if fl != 255:
                afc_raw = mb[m0 + 16: m0 + 16 + fl].decode("latin-1")
                try:
                    fr.freq_afc = calc_afc(int(afc_raw))
                except ValueError:
                    self.logger.warning("Could not parse %s value: %s", "AFC", afc_raw)
            msgs = []
            rb = d_rb[i]
            for r in range(rb, rb + nr):
                p = r_p[r]
                o = r_off[r]
                payload = hs[o: o + r_len[r]]
                if name == "MC":
                    pid = mc_pids[p]
                    md = {"protocol_id": pid, "rssi": None, "freq_afc": None}
                elif name == "MU":
                    pid = mu_pids[p]
                    md = {"bit_length": r_bl[r], "rssi": rssi_raw, "clock": mu_clock[p]}
                else:
                    pid = ms_pids[p]
                    md = {"bit_length": r_bl[r], "rssi": rssi_raw, "clock": ms_clock_l[i]}
                msgs.append(DecodedMessage(protocol_id=str(pid), payload=payload, raw=fr, metadata=md))
            out.append(msgs)
        return out

    def _general_messages(self, line, i, plen, offsets, slot, meta, name, d, rec, hb, ms_clock) -> List[DecodedMessage]:
        """The DecodedMessage list of a general-path line (as the OK lines' records below)."""
        bk = self.protocols._bank
        if d["status"] == runtime.ST_RAISED and int(d["raise_kind"]) == runtime.RAISE_CONTRACT:
            return _contract(i, name)   # a general-path limit (SDX_GEN_*), not a reference outcome
        if d["status"] == runtime.ST_RAISED or int(d["n_rec"]) == 0:
            return []   # a demodulator exception is caught by the reference's parsers
        if d["status"] != runtime.ST_OK:
            raise RuntimeError(f"device status {int(d['status'])} for line {i}")
        fr = self._frame(line, i, plen, offsets, slot, meta, name)
        rssi_raw = self._meta_str(meta[i], 0)
        msgs = []
        for r in rec[int(d["rec_begin"]): int(d["rec_begin"]) + int(d["n_rec"])]:
            p = int(r["proto"])
            off = int(r["payload_off"])
            pid = bk.mu_pids[p] if name == "MU" else bk.ms_pids[p]
            md = {"bit_length": int(r["bit_length"]), "rssi": rssi_raw,
                  "clock": bk.mu_clock[p] if name == "MU" else ms_clock}
            msgs.append(DecodedMessage(protocol_id=str(pid), payload=hb[off: off + int(r["payload_len"])].decode("latin-1"),
                                       raw=fr, metadata=md))
        return msgs

    def _payload(self, line, i, plen, offsets, slot) -> str:
        if plen[i] >= 0:
            s0 = 3 * int(offsets[i])
            return bytes(slot[s0: s0 + int(plen[i])]).decode("latin-1")
        s = line.decode("latin-1") if isinstance(line, (bytes, bytearray, memoryview)) else line
        return s.strip()[1:-1]

    def _mn_messages(self, line, i, plen, offsets, slot, meta, d, rec, hb) -> List[DecodedMessage]:
        """DecodedMessage list of an MN line (parser/mn.py:53-77,175-191): RawFrame(line=payload,
        message_type='MN') without frame rssi/afc; metadata rssi / freq_afc / modulation / rfmode."""
        bk = self.protocols._bank
        fr = RawFrame(line=self._payload(line, i, plen, offsets, slot), message_type="MN")
        r, a = self._meta_str(meta[i], 0), self._meta_str(meta[i], 16)
        rssi = calc_rssi(int(r)) if r else None
        afc = calc_mn_afc(int(a)) if a else None
        msgs = []
        for x in rec[int(d["rec_begin"]): int(d["rec_begin"]) + int(d["n_rec"])]:
            p = int(x["proto"])
            off = int(x["payload_off"])
            msgs.append(DecodedMessage(protocol_id=str(bk.mn_pids[p]),
                                       payload=hb[off: off + int(x["payload_len"])].decode("latin-1"), raw=fr,
                                       metadata={"rssi": rssi, "freq_afc": afc, "modulation": bk.mn_modulation[p],
                                                 "rfmode": bk.mn_rfmode[p]}))
        return msgs

    # ------------------------------------------------------------------------------------------
    def stream(self, chunk_lines: int = 250_000, chunk_bytes: Optional[int] = None, output: str = "json",
               lag: int = 3, collapse_repeats: bool = False, repeat_window: Optional[float] = None,
               repeat_sources: Optional[int] = None, routes=None, drop_unrouted: bool = False,
               route_match: str = "first", profiles=None, rules=None):
        """A pipelined LineStream over this parser (pysignalduino_amd/stream.py): chunks of raw lines
        in, the controller's JSON texts (or the wire form) out, the PCIe copies, parse, demodulation
        and serialisation of successive chunks overlapping; the same per-line results as
        parse_lines_json / parse_lines.  ``repeat_sources``: the stream merges that many receivers, every
        submit names its lines' source ids and repeat suppression runs per source (stream.py).  ``routes``
        (a routes.RouteTable or a list of (name, pattern) pairs) / ``drop_unrouted``: payload routes, as
        parse_lines_routed: ChunkResult.route and items_routed(); None leaves the stream as it is.
        ``route_match="any"`` (with ``routes``): the line's first message that a route wants is the published
        one; ChunkResult.pick holds its index.  ``profiles``: receiver profiles, every
        submit names its lines' source ids as with ``repeat_sources`` (stream.py).  ``output="json_all"``: every
        message of a line, as parse_lines_json_all (ChunkResult.texts_all / items_all), with
        ``rules`` (None, True or a dispatch.DispatchRules) what that call takes as ``dispatch``."""
        from .stream import LineStream
        kw = {} if repeat_window is None else {"repeat_window": repeat_window}
        if rules is not None:
            kw["rules"] = rules
        if repeat_sources is not None:
            kw["repeat_sources"] = repeat_sources
        _check_route_match(route_match, routes)
        if routes is not None:
            kw.update(routes=routes, drop_unrouted=drop_unrouted)
            if route_match != "first":
                kw["route_match"] = route_match
        elif drop_unrouted:
            raise ValueError("drop_unrouted needs routes")
        if profiles is not None:
            kw["profiles"] = profiles
        return LineStream(self, chunk_lines=chunk_lines, chunk_bytes=chunk_bytes, output=output, lag=lag,
                          collapse_repeats=collapse_repeats, **kw)

    def parse_lines_json(self, lines: Sequence[Union[str, bytes]], collapse_repeats: bool = False, times=None,
                         repeat_window: Optional[float] = None, sources=None,
                         profiles=None) -> List[Union[Optional[str], Exception]]:
        """Per line, the MQTT message text the reference controller publishes for it:
        ``MqttPublisher._message_to_json(parse_line(line)[0])`` (signalduino/controller.py:254-257,
        mqtt.py:227-245), or None when the line decodes to nothing -- parse, demodulation and JSON
        serialisation (sdx_serialize_json) all on the device; only the texts come back.
        ``collapse_repeats``: a line that repeats the previous result-bearing line's (kind, protocol,
        payload) gives None -- marked on the device (sdx_mark_repeats) and never serialised; the mask
        is left in ``last_repeat_mask``.  ``repeat_window`` (seconds) with ``times`` (one arrival time in
        integer microseconds per line, non-decreasing; checked before anything is launched): a run also
        ends once its last published line is more than the window old (sdx_mark_repeats_timed).
        ``sources`` (one integer id per line, the receiver it came from; S = the largest id + 1): every
        source's lines are a stream of their own (sdx_mark_repeats_by_source), the times non-decreasing
        within a source.  ``profiles`` (with ``sources``, also without collapse_repeats): receiver profiles as
        parse_lines takes them -- the published message is the first one the line's source enables."""
        from .profiles import as_profiles
        profiles = as_profiles(profiles)
        sources = self._source_args(collapse_repeats, sources, len(lines), profiles)
        times, w = self._window_args(collapse_repeats, times, repeat_window, len(lines), sources)
        if len(lines) == 0:
            if collapse_repeats:
                self.last_repeat_mask = np.zeros(0, np.uint8)
            return []
        data, offsets, bad = pack_lines(lines)
        return self._texts(lines, LineBatch(self.protocols._ensure(), data, offsets), bad, len(data), collapse_repeats,
                           times, w, sources, profiles=profiles)

    def parse_lines_routed(self, lines: Sequence[Union[str, bytes]], routes, drop_unrouted: bool = False,
                           collapse_repeats: bool = False, times=None, repeat_window: Optional[float] = None,
                           sources=None, route_match: str = "first",
                           profiles=None) -> List[Union[None, Tuple[int, str], Exception]]:
        """parse_lines_json with payload routes: per line None, or (route_index, text) -- the
        text parse_lines_json gives, and the index of the first route of ``routes`` (a routes.RouteTable or
        a list of (name, pattern) pairs) whose pattern matches the payload of ``decoded[0]`` by ``re.search``,
        -1 when none does.  Matched on the device (sdx_route_lines) behind the repeat pass, if any, and in
        front of the serialiser; host-resolved lines are matched with RouteTable.match.  ``drop_unrouted``:
        an unrouted line gives None (published = result-bearing, no repeat, routed); routing never changes
        which lines are repeats.  The other arguments, and ContractError slots, as parse_lines_json.  The
        lines' routes are left in ``last_routes`` (int16, -1 also for lines without a result).
        ``route_match="any"``: FHEM's answer for a line that demodulates to several messages --
        the published message is the first one, in the reference's list order, that some route matches
        (``decoded[0]`` when none does): its text, its repeat key and its route, matched on the device over
        every record of the line (sdx_route_records).  ``last_picks`` (uint16) holds that message's index;
        "first" leaves it None.  ``profiles``: as parse_lines_json; the routes see the filtered lists, and
        ``last_picks`` indexes them."""
        from .profiles import as_profiles
        from .routes import as_table
        _check_route_match(route_match, routes)
        table = as_table(routes)
        if table is None:
            raise ValueError("parse_lines_routed needs a route table")
        any_ = route_match == "any"
        profiles = as_profiles(profiles)
        sources = self._source_args(collapse_repeats, sources, len(lines), profiles)
        times, w = self._window_args(collapse_repeats, times, repeat_window, len(lines), sources)
        if len(lines) == 0:
            if collapse_repeats:
                self.last_repeat_mask = np.zeros(0, np.uint8)
            self.last_routes = np.zeros(0, np.int16)
            self.last_picks = np.zeros(0, np.uint16) if any_ else None
            return []
        data, offsets, bad = pack_lines(lines)
        return self._texts(lines, LineBatch(self.protocols._ensure(), data, offsets), bad, len(data), collapse_repeats,
                           times, w, sources, routes=table, drop_unrouted=drop_unrouted, match_any=any_, profiles=profiles)

    # -- what the JSON paths share: one launch set per kind, its outputs left on the device ------------------
    def _json_jobs(self, lb: LineBatch, nbytes: int):
        """-> (per kind with lines: (kind, rec_cap, heap_cap, json_cap, launches), the pulse batch); the batch is
        launched already."""
        bk = self.protocols._bank
        sels, cnt = lb.selections()
        pb = lb.pulse_batch()
        jobs = []
        if cnt[runtime.SEL_MU_SHORT] or cnt[runtime.SEL_MU_LONG]:
            k = int(cnt[runtime.SEL_MU_SHORT] + cnt[runtime.SEL_MU_LONG])
            jobs.append((runtime.KIND_MU, 8 * k + 1024, 200 * k + 65536, 600 * k + 65536,
                         [(pb, sels[runtime.SEL_MU_SHORT], False), (pb, sels[runtime.SEL_MU_LONG], True)]))
        if cnt[runtime.SEL_MS_SHORT] or cnt[runtime.SEL_MS_LONG]:
            k = int(cnt[runtime.SEL_MS_SHORT] + cnt[runtime.SEL_MS_LONG])
            jobs.append((runtime.KIND_MS, 4 * k + 1024, 64 * k + 65536, 300 * k + 65536,
                         [(pb, sels[runtime.SEL_MS_SHORT], False), (pb, sels[runtime.SEL_MS_LONG], True)]))
        mc_sel, k = lb.mc_all(cnt)
        if self.protocols.mc_mode == "fixed" and k:
            jobs.append((runtime.KIND_MC, 4 * k + 1024, 96 * k + 65536, 400 * k + 65536,
                         [(lb.mc_batch(), mc_sel, False)]))
        if cnt[runtime.SEL_MN]:
            k = int(cnt[runtime.SEL_MN])
            jobs.append((runtime.KIND_MN, len(bk.mn_pids) * k + 1024, int(4 * nbytes + 64 * k + 65536),
                         int(6 * nbytes + 400 * k + 65536), [(lb.mn_batch(), sels[runtime.SEL_MN], False)]))
        return jobs, pb

    def _demodulate(self, n: int, kind, launches, rec_cap, heap_cap, elig):
        eng = self.protocols._ensure()
        work = eng.pulses_work_bytes(n) if kind in (runtime.KIND_MU, runtime.KIND_MS) else 0
        out = eng.alloc_out(n, rec_cap, heap_cap, work)  # MU/MS: grouped order + spill room
        for bd, sel, long_v in launches:
            if not sel.numel():
                continue
            if kind == runtime.KIND_MN:
                eng.launch_mn(bd, out, elig=elig, sel=sel)
            elif kind == runtime.KIND_MC:
                eng.launch_mc(bd, out, sel=sel)
            else:
                eng.launch_pulses(kind, bd, out, sel=sel, long_variant=long_v)
        return out

    def _rerun_tile_overflows(self, n: int, pb, kind, out, rec_cap, heap_cap):
        """An MU/MS launch whose cursor[2] is 2: tiles overflowed their on-chip staging and found no
        spill region left (ST_OVF_TILE), which larger outputs cannot cure.  Those messages re-run on
        the long variant into an overlay, as Engine.run does; returns the launch and the overlay as
        one output (merge_overlay), which the repeat pass and the serialiser read like any other."""
        eng = self.protocols._ensure()
        st = out["desc"][: 8 * n].view(-1, 8)[:, 6].cpu().numpy()
        redo = np.nonzero(st == runtime.ST_OVF_TILE)[0].astype(np.int32)
        for _attempt in range(4):
            ov = eng.rerun_overlay(kind, pb, redo, rec_cap, heap_cap)
            c = ov["cursor"].cpu().numpy()
            if c[2] & 2:
                raise RuntimeError("result staging overflow persists (pathological message)")
            if not c[2]:
                return eng.merge_overlay(out, ov, redo)
            rec_cap, heap_cap = 4 * rec_cap, 4 * heap_cap
        raise RuntimeError("result capacity overflow persists")

    def _demodulate_kept(self, n: int, pb, jobs, elig, host_rows: List[int]):
        """Every kind's launch, grown and re-run until nothing but host rows is left over: -> [(kind, out, json_cap)]
        with the outputs on the device; MC frames the device hands over are appended to ``host_rows``."""
        kept = []
        for kind, rec_cap, heap_cap, json_cap, launches in jobs:
            for _attempt in range(4):
                out = self._demodulate(n, kind, launches, rec_cap, heap_cap, elig)
                c1 = out["cursor"].cpu().numpy()
                if kind == runtime.KIND_MC and c1[2] == 2:   # frames of > 128 hex characters: host rows
                    sel = launches[0][1]
                    st = out["desc"][: 8 * n].view(-1, 8)[:, 6][sel.long()].cpu().numpy()
                    host_rows.extend(int(i) for i in sel.cpu().numpy()[st == runtime.ST_OVF_TILE])
                    break
                if kind in (runtime.KIND_MU, runtime.KIND_MS) and c1[2] == 2:   # only tile overflows are left: not a capacity matter
                    out = self._rerun_tile_overflows(n, pb, kind, out, rec_cap, heap_cap)
                    break
                if not c1[2]:
                    break
                rec_cap, heap_cap = 4 * rec_cap, 4 * heap_cap   # bit 0: the outputs overflowed
            else:
                raise RuntimeError("result capacity overflow persists")
            kept.append((kind, out, json_cap))
        return kept

    def _record_passes(self, n: int, kept, lo, profiles=None, sources=None, dispatch=None):
        """_demodulate_kept's outputs through the record passes, right behind the launches: sdx_filter_records
        (``profiles``, ``sources``), then sdx_dispatch_records (``dispatch``).  Every line keeps the records the pass
        keeps, compacted in line order; everything behind reads the rewritten outputs (they share the launches' heaps)."""
        eng = self.protocols._ensure()

        def through(kept, alloc, run):
            bufs = alloc(n, [o for _, o, _ in kept])
            outs = run([eng.json_in(kind, o, lo, n) for kind, o, _ in kept], bufs)
            return [(kind, x, json_cap) for (kind, _, json_cap), x in zip(kept, outs)]

        if kept and profiles is not None:
            kept = through(kept, eng.alloc_profiles, lambda ins, bufs: eng.filter_records(
                profiles, ins, n, bufs, source=None if sources is None else eng.torch.from_numpy(
                    np.ascontiguousarray(sources, np.int32)).to(eng.dev)))
        if kept and dispatch is not None:
            kept = through(kept, eng.alloc_dispatch, lambda ins, bufs: eng.dispatch_records(dispatch, ins, n, bufs))
        return kept

    @staticmethod
    def _pass_kw(rows, profiles=None, sources=None, dispatch=None) -> dict:
        """The profile and dispatch keywords of a parse_lines* call over the lines ``rows`` of this batch."""
        kw = {} if dispatch is None else {"dispatch": dispatch}
        if profiles is not None:
            kw.update(profiles=profiles, sources=None if sources is None else [int(sources[i]) for i in rows])
        return kw

    def _host_rows(self, lines, lb: LineBatch, bad: dict, host_rows: List[int], slots: list, put, **passes):
        """The rows the host resolves: the general-path lines (rare), ``host_rows``, and the unsupported MU/MS lines
        with them -- parse_lines resolves the ones whose P# values need the exact float() (sdx_lines_exact); the
        others come back as ContractError.  ``put(i, g)`` takes line i's parse_lines value (``passes``: its profile
        and dispatch keywords); then ``slots`` gets the ``bad`` values and the ContractErrors.  -> the line kinds."""
        n = len(lines)
        status = lb.status[:n].cpu().numpy()
        kinds = lb.kind[:n].cpu().numpy()
        exact = (status == runtime.LS_UNSUPPORTED) & ((kinds == runtime.LINE_MU) | (kinds == runtime.LINE_MS))
        grows = [int(i) for i in np.nonzero((status == runtime.LS_GENERAL) | exact)[0] if int(i) not in bad] + host_rows
        resolved = set()
        if grows:
            for i, g in zip(grows, self.parse_lines([lines[i] for i in grows], **self._pass_kw(grows, **passes))):
                if exact[i] and not isinstance(g, ContractError):
                    resolved.add(i)   # else still unsupported: reported below, under its index in this batch
                put(i, g)
        for i in range(n):
            if i in bad:
                slots[i] = bad[i]
            elif int(status[i]) == runtime.LS_UNSUPPORTED and i not in resolved:
                slots[i] = _outside_contract(i, kinds[i])
        return kinds

    def _reconcile_repeats(self, slots: list, kinds, rpass, rbufs, rep, has_text, host_keys: dict, times, rsources,
                           empty, first, one) -> None:
        """The device's repeat mask ``rep`` made exact where host-resolved rows stand in a run, and ``slots`` with
        it; the mask is left in last_repeat_mask.  ``empty``: a dropped line's slot value; ``first(x)``: the first
        text of the slot value x, None where it has none; ``one(i)``: line i's slot value computed on its own."""
        import copy
        from .repeats import apply_mask, text_key
        fetched = {}
        key = lambda i, x: None if first(x) is None else text_key(_KIND_NAME[int(kinds[i])], first(x))   # noqa: E731

        def fetch_key(i):   # a flagged line whose run head the host does not know: the batch API
            fetched[i] = one(i)
            return key(i, fetched[i])

        mask = rpass.exact_mask(rbufs, rep, has_text, lambda i: key(i, slots[i]), host_keys, fetch=fetch_key, times=times,
                                sources=rsources)

        def drop(i):         # a host-resolved repeat, or a repeat of a host-resolved line
            slots[i] = copy.copy(empty)

        def republish(i):    # the device skipped it, but its predecessor was a host row
            slots[i] = fetched[i] if i in fetched else one(i)
        apply_mask(mask, rep, host_keys, drop, republish)
        self.last_repeat_mask = mask

    def _texts(self, lines, lb: LineBatch, bad: dict, nbytes: int, collapse: bool = False, times=None,
               window_us: Optional[int] = None, sources=None, routes=None, drop_unrouted: bool = False,
               match_any: bool = False, profiles=None):
        """parse_lines_json from the uploaded batch on (``lines`` and ``nbytes`` as in _objects).  ``routes``
        (a routes.RouteTable; parse_lines_routed): every text becomes (route, text), see there; ``match_any``:
        its route_match="any".  ``profiles`` (a profiles.ReceiverProfiles; ``sources``: the ids, or None for its
        source 0): every kind's launch output goes through sdx_filter_records before anything else reads it."""
        n = len(lines)
        eng = self.protocols._ensure()
        lb.launch()
        lo = {"meta": lb.meta, "pat_val": lb.pat_val, "cp_slot": lb.cp_slot}
        jobs, pb = self._json_jobs(lb, nbytes)
        elig = self._mn_elig(profiles)
        rsources = sources if collapse else None   # the repeat pass's ids: without collapse the ids are the profiles' alone
        texts: List[Any] = [None] * n
        host_rows: List[int] = []   # lines whose text is built from parse_lines' objects (general paths)

        def demodulate(kind, launches, rec_cap, heap_cap):
            return self._demodulate(n, kind, launches, rec_cap, heap_cap, elig)

        def rerun_tile_overflows(kind, out, rec_cap, heap_cap):
            return self._rerun_tile_overflows(n, pb, kind, out, rec_cap, heap_cap)

        def serialize(kind, out, json_cap, skip=None):
            """The launch's texts into a fresh buffer, grown until they fit: (buffers, bytes used)."""
            for _attempt in range(4):
                jo = eng.alloc_json(n, json_cap)
                eng.launch_json(kind, out, lo, n, jo, first_only=True, skip=skip)
                c2 = jo["cursor"].cpu().numpy()
                if not c2[1]:
                    return jo, c2[0]
                json_cap *= 4
            raise RuntimeError("JSON capacity overflow persists")

        pulses = (runtime.KIND_MU, runtime.KIND_MS)

        def take_texts(jo, used):
            lens = jo["len"][:n].cpu().numpy()
            offs = jo["off"][:n].cpu().numpy()
            blob = jo["json"][: int(used)].cpu().numpy().tobytes()
            for i in np.nonzero(lens > 0)[0]:
                texts[int(i)] = blob[int(offs[i]): int(offs[i]) + int(lens[i])].decode("ascii")

        rep = np.zeros(n, np.uint8)   # the device's repeat mask (collapse)
        route = np.full(n, -1, np.int16)   # the lines' routes (routes)
        pick = np.zeros(n, np.uint16)      # the lines' picked records (match_any)
        if collapse:
            from .repeats import RepeatPass, count_sources, objects_key
            rpass = RepeatPass(eng, window_us, None if sources is None else count_sources(sources))
            rbufs = None
        if collapse or routes is not None or profiles is not None:
            # every kind's launch first (their outputs stay on the device), then ONE sdx_mark_repeats over
            # them, then the serialiser with the mask: a repeat is never turned into text
            kept = self._demodulate_kept(n, pb, jobs, elig, host_rows)
            kept = self._record_passes(n, kept, lo, profiles, sources)
            if kept:   # a fresh stream of lines per call; nothing is read back but the mask (and the sources' table)
                ins = [eng.json_in(kind, out, lo, n) for kind, out, _ in kept]
                skip = None
                if match_any:
                    # the match first: it picks every line's published record and writes the views in which a
                    # line owns exactly that record; the repeat pass and the serialiser then run over the views
                    rb = eng.alloc_routes(n, mask=False, skip=not collapse and drop_unrouted, pick=True, views=len(ins))
                    eng.route_records(eng.route_table(routes), ins, n, rb["route"], rb["pick"], rb["views"])
                    ins = [eng.json_in_view(ji, v) for ji, v in zip(ins, rb["views"])]
                    kept = [(kind, dict(out, desc=v), json_cap) for (kind, out, json_cap), v in zip(kept, rb["views"])]
                if collapse:
                    rbufs = rpass.alloc(n, pinned=False)
                    rpass.enqueue(rbufs, ins, n, times=times, sources=rsources)
                    skip = rbufs.mask
                if match_any:
                    if rb["skip"] is not None:   # as below: with collapse the unrouted texts still come back
                        eng.route_skip(ins, n, rb["route"], rb["skip"], drop_unrouted=True)
                        skip = rb["skip"]
                elif routes is not None:
                    # behind the repeat pass, in front of the serialiser.  With collapse the host needs the key
                    # of every line that is no repeat (RepeatTracker), so unrouted texts still come back and are
                    # dropped below; without it the device leaves them out
                    rb = eng.alloc_routes(n, mask=False, skip=not collapse and drop_unrouted)
                    eng.route_lines(eng.route_table(routes), ins, n, rb["route"], None, rb["skip"], drop_unrouted=drop_unrouted)
                    skip = rb["skip"] if rb["skip"] is not None else skip
                for kind, out, json_cap in kept:
                    take_texts(*serialize(kind, out, json_cap, skip=skip))
                if collapse:
                    rep = rbufs.mask[:n].cpu().numpy()
                if routes is not None:
                    route = rb["route"][:n].cpu().numpy()
                if match_any:
                    pick = rb["pick"][:n].cpu().numpy().view(np.uint16)
            jobs = []
        for kind, rec_cap, heap_cap, json_cap, launches in jobs:
            for _attempt in range(4):
                out = demodulate(kind, launches, rec_cap, heap_cap)
                jo = eng.alloc_json(n, json_cap)
                eng.launch_json(kind, out, lo, n, jo, first_only=True)
                c1 = out["cursor"].cpu().numpy()
                c2 = jo["cursor"].cpu().numpy()
                if kind == runtime.KIND_MC and c1[2] == 2 and not c2[1]:
                    # frames of > 128 hex characters were handed over (ST_OVF_TILE): their texts below
                    sel = launches[0][1]
                    st = out["desc"][: 8 * n].view(-1, 8)[:, 6][sel.long()].cpu().numpy()
                    host_rows.extend(int(i) for i in sel.cpu().numpy()[st == runtime.ST_OVF_TILE])
                    break
                if kind in pulses and c1[2] == 2:
                    # only tile overflows are left: not a capacity matter.  The texts again, from the launch
                    # merged with the re-run of those messages
                    jo, used = serialize(kind, rerun_tile_overflows(kind, out, rec_cap, heap_cap), json_cap)
                    c2 = (used, 0)
                    break
                if not c1[2] and not c2[1]:
                    break
                rec_cap, heap_cap, json_cap = 4 * rec_cap, 4 * heap_cap, 4 * json_cap
            else:
                raise RuntimeError("result / JSON capacity overflow persists")
            take_texts(jo, c2[0])
        has_text = np.fromiter((x is not None for x in texts), bool, n) if collapse else None
        host_keys = {}   # collapse: the host-resolved rows' keys (None: no result)

        def put(i, g):   # a host-resolved line: its objects from parse_lines, the text as _message_to_json
            if match_any and isinstance(g, list) and g:   # the published message is the picked one
                pick[i], route[i], _ = routes.pick([m.payload for m in g])
                g = g[int(pick[i]): int(pick[i]) + 1]
            if collapse:
                host_keys[i] = objects_key(g)
            if isinstance(g, BaseException):
                texts[i] = g
            elif g:
                texts[i] = json.dumps({"protocol_id": g[0].protocol_id, "payload": g[0].payload,
                                       "metadata": g[0].metadata}, indent=4)
                if routes is not None and not match_any:   # the same tables, walked on the host
                    route[i] = routes.match(g[0].payload)[0]

        kinds = self._host_rows(lines, lb, bad, host_rows, texts, put, profiles=profiles, sources=sources)
        if collapse:
            def one_text(i):    # the line's published text on its own (match_any: the picked message's)
                pkw = self._pass_kw([i], profiles, sources)
                if not match_any:
                    return self.parse_lines_json([lines[i]], **pkw)[0]
                x = self.parse_lines_routed([lines[i]], routes, route_match="any", **pkw)[0]
                return x[1] if isinstance(x, tuple) else x

            self._reconcile_repeats(texts, kinds, rpass, rbufs, rep, has_text, host_keys, times, rsources, None,
                                    lambda x: x if isinstance(x, str) else None, one_text)
        if routes is not None:
            self.last_routes = route
            self.last_picks = pick if match_any else None
            for i, x in enumerate(texts):
                if isinstance(x, str):
                    texts[i] = None if drop_unrouted and route[i] < 0 else (int(route[i]), x)
        return texts

    # -- every message of a line -------------------------------------------------------
    def parse_lines_json_all(self, lines: Sequence[Union[str, bytes]], dispatch=None, profiles=None, sources=None,
                             collapse_repeats: bool = False, times=None,
                             repeat_window: Optional[float] = None) -> List[Union[List[str], Exception]]:
        """Per line, the MQTT texts of EVERY message it decodes to, in the reference's order:
        ``[MqttPublisher._message_to_json(m) for m in parse_line(line)]``, [] where nothing decodes, the
        ContractError in its slot as elsewhere -- FHEM dispatches every message of a line, where
        parse_lines_json publishes ``decoded[0]`` alone.  The texts are built on the device, one per result
        record (sdx_serialize_json, first_only = 0).  ``dispatch`` (a dispatch.DispatchRules, True for FHEM's
        defaults): every list reduced by the dispatch rules first (sdx_dispatch_records) -- at most ``max_repeat``
        messages of one protocol in a row, a message equal to the one before it dropped unless its protocol
        carries ``dispatchequals``; None: every message.  ``profiles`` / ``sources``: receiver profiles as
        parse_lines_json takes them, in front of the rules (a disabled protocol never runs, so it never counts).
        ``collapse_repeats`` (``times``, ``repeat_window``, ``sources`` as parse_lines_json): a line that repeats
        the previous result-bearing line's first message gives []; the mask is left in ``last_repeat_mask``.  The
        first text of a line's list is always parse_lines_json's text of that line."""
        from .dispatch import as_rules
        from .profiles import as_profiles
        dispatch = as_rules(dispatch)
        profiles = as_profiles(profiles)
        sources = self._source_args(collapse_repeats, sources, len(lines), profiles)
        times, w = self._window_args(collapse_repeats, times, repeat_window, len(lines), sources)
        if len(lines) == 0:
            if collapse_repeats:
                self.last_repeat_mask = np.zeros(0, np.uint8)
            return []
        data, offsets, bad = pack_lines(lines)
        return self._texts_all(lines, LineBatch(self.protocols._ensure(), data, offsets), bad, len(data), dispatch, profiles,
                               sources, collapse_repeats, times, w)

    def parse_bytes_json_all(self, data, final: bool = True, dispatch=None, profiles=None, collapse_repeats: bool = False):
        """parse_lines_json_all over a raw read buffer (see parse_bytes; the same return forms)."""
        from .dispatch import as_rules
        from .profiles import as_profiles
        dispatch = as_rules(dispatch)
        profiles = as_profiles(profiles)
        self._source_args(collapse_repeats, None, 0, profiles)
        lines, lb, tail = self._split_bytes(data, final)
        if collapse_repeats:
            self.last_repeat_mask = np.zeros(0, np.uint8)
        out = (self._texts_all(lines, lb, {}, int(lines.offsets[-1]), dispatch, profiles, None, collapse_repeats)
               if len(lines) else [])
        return out if final else (out, tail)

    def _texts_all(self, lines, lb: LineBatch, bad: dict, nbytes: int, dispatch=None, profiles=None, sources=None,
                   collapse: bool = False, times=None, window_us: Optional[int] = None):
        """parse_lines_json_all from the uploaded batch on (``lines`` and ``nbytes`` as in _objects): every kind's
        launch, the profile pass, the dispatch pass, the repeat pass, then the serialiser over every record of what
        is left -- line g's texts stand at the record indices [rec_begin, rec_begin + n_rec) of its descriptor."""
        n = len(lines)
        eng = self.protocols._ensure()
        lb.launch()
        lo = {"meta": lb.meta, "pat_val": lb.pat_val, "cp_slot": lb.cp_slot}
        jobs, pb = self._json_jobs(lb, nbytes)
        rsources = sources if collapse else None
        out: List[Any] = [[] for _ in range(n)]
        host_rows: List[int] = []   # lines whose texts are built from parse_lines' objects (general paths)
        kept = self._demodulate_kept(n, pb, jobs, self._mn_elig(profiles), host_rows)
        kept = self._record_passes(n, kept, lo, profiles, sources, dispatch)
        ins_of = lambda ks: [eng.json_in(kind, o, lo, n) for kind, o, _ in ks]   # noqa: E731
        rep = np.zeros(n, np.uint8)
        rbufs = None
        if collapse:
            from .repeats import RepeatPass, count_sources, objects_key
            rpass = RepeatPass(eng, window_us, None if sources is None else count_sources(sources))
        if kept:
            skip = None
            if collapse:   # the mask of the lines' first records: a repeat line loses every record's text
                rbufs = rpass.alloc(n, pinned=False)
                rpass.enqueue(rbufs, ins_of(kept), n, times=times, sources=rsources)
                skip = rbufs.mask
            for kind, o, json_cap in kept:
                self._take_texts_all(out, n, kind, o, lo, 2 * json_cap, skip)
            if collapse:
                rep = rbufs.mask[:n].cpu().numpy()
        has_text = np.fromiter((bool(x) for x in out), bool, n) if collapse else None
        host_keys = {}   # collapse: the host-resolved rows' keys (None: no result)
        passes = {"profiles": profiles, "sources": sources, "dispatch": dispatch}

        def put(i, g):   # a host-resolved line: its objects from parse_lines, every message's text on the host
            if collapse:
                host_keys[i] = objects_key(g)
            out[i] = g if isinstance(g, BaseException) else [
                json.dumps({"protocol_id": m.protocol_id, "payload": m.payload, "metadata": m.metadata}, indent=4) for m in g]

        kinds = self._host_rows(lines, lb, bad, host_rows, out, put, **passes)
        if collapse:
            self._reconcile_repeats(out, kinds, rpass, rbufs, rep, has_text, host_keys, times, rsources, [],
                                    lambda x: x[0] if isinstance(x, list) and x else None,
                                    lambda i: self.parse_lines_json_all([lines[i]], **self._pass_kw([i], **passes))[0])
        return out

    def _take_texts_all(self, out: list, n: int, kind, o, lo, json_cap: int, skip) -> None:
        """One kind's texts, one per record (first_only = 0), into a fresh buffer grown until they fit; then per line
        with an OK descriptor the texts of its records, in order, into ``out``."""
        eng = self.protocols._ensure()
        items = max(int(o["rec_cap"]), 1)
        for _attempt in range(5):
            jo = eng.alloc_json(items, json_cap)
            jo["len"].zero_()
            eng.launch_json(kind, o, lo, n, jo, first_only=0, skip=skip)
            c = jo["cursor"].cpu().numpy()
            if not c[1]:
                break
            json_cap *= 4
        else:
            raise RuntimeError("JSON capacity overflow persists")
        desc = o["desc"][: 8 * n].cpu().numpy().view(runtime.DESC_DT)
        rows = np.nonzero((desc["status"] == runtime.ST_OK) & (desc["n_rec"] > 0))[0]
        if not len(rows):
            return
        total = min(int(o["cursor"][0].item()), items)
        lens = jo["len"][:total].cpu().numpy().tolist()
        offs = jo["off"][:total].cpu().numpy().tolist()
        blob = jo["json"][: int(c[0])].cpu().numpy().tobytes().decode("ascii")
        begin, count = desc["rec_begin"][rows].tolist(), desc["n_rec"][rows].tolist()
        for i, b, k in zip(rows.tolist(), begin, count):
            out[i] = [blob[offs[r]: offs[r] + lens[r]] for r in range(b, b + k) if lens[r]]

    # -- byte-stream input ---------------------------------------------------------------------------
    def parse_bytes(self, data, final: bool = True, collapse_repeats: bool = False, profiles=None, dispatch=None):
        """parse_lines over a transport's raw read buffer (bytes-like): the bytes are uploaded and split
        into lines on the device (sdx_split_lines: every '\\n' ends a line, as StreamReader.readline(),
        signalduino/transport.py:113-123).  ``final=True``: bytes after the last '\\n' are the last line
        (readline() at EOF); returns parse_lines' list for those lines.  ``final=False``: returns
        (that list for the terminated lines, the unterminated tail as bytes) -- prepend the tail to the
        next buffer.  There is no ``repeat_window`` here or in parse_bytes_json: one call has no per-line
        arrival times (LineStream.submit_bytes takes one per read buffer).  ``profiles``: receiver profiles as
        parse_lines takes them, for the one receiver the buffer was read from (a table of one source).  ``dispatch``:
        the dispatch rules as parse_lines takes them."""
        from .dispatch import as_rules
        from .profiles import as_profiles
        dispatch = as_rules(dispatch)
        profiles = as_profiles(profiles)
        self._source_args(collapse_repeats, None, 0, profiles)
        lines, lb, tail = self._split_bytes(data, final)
        out = (self._objects(lines, lb, lines.offsets, {}, int(lines.offsets[-1]), profiles, dispatch=dispatch)
               if len(lines) else [])
        out = self._collapsed(out, collapse_repeats)
        return out if final else (out, tail)

    def parse_bytes_json(self, data, final: bool = True, collapse_repeats: bool = False, profiles=None):
        """parse_lines_json over a raw read buffer (see parse_bytes; the same return forms)."""
        from .profiles import as_profiles
        profiles = as_profiles(profiles)
        self._source_args(collapse_repeats, None, 0, profiles)
        lines, lb, tail = self._split_bytes(data, final)
        if collapse_repeats:
            self.last_repeat_mask = np.zeros(0, np.uint8)
        out = self._texts(lines, lb, {}, int(lines.offsets[-1]), collapse_repeats, profiles=profiles) if len(lines) else []
        return out if final else (out, tail)

    def _split_bytes(self, data, final: bool):
        """Upload + sdx_split_lines -> (the lines as a host view, their LineBatch or None, the tail)."""
        raw = data if isinstance(data, (bytes, bytearray)) else bytes(data)
        nb = len(raw)
        if nb >= 1 << 31:
            raise ValueError("parse_bytes takes less than 2^31 bytes per call")
        eng = self.protocols._ensure()
        t, d = eng.torch, eng.dev
        bytes_dev = t.zeros(nb + 16, dtype=t.uint8, device=d)   # 16 zero bytes of read-ahead (include/sdx.h)
        if nb:
            bytes_dev[:nb] = t.from_numpy(np.frombuffer(raw, np.uint8).copy())
        cap = raw.count(b"\n") + 1          # room for every line; the launches are sized by the device's count
        offsets_dev = t.empty(cap + 1, dtype=t.int64, device=d)
        count = t.zeros(2, dtype=t.int64, device=d)
        scratch = t.empty(eng.split_work_ints(nb), dtype=t.int32, device=d)
        eng.split_lines(bytes_dev, nb, final, offsets_dev, cap, count, scratch)
        n, tail_at = (int(x) for x in count.cpu().numpy())
        if n > cap:
            raise RuntimeError(f"sdx_split_lines found {n} lines, the host at most {cap}")
        offsets = offsets_dev[: n + 1].cpu().numpy()
        lines = _LinesView(raw, offsets)
        lb = LineBatch.from_device(eng, bytes_dev, offsets_dev, n, int(offsets[-1])) if n else None
        return lines, lb, bytes(raw[tail_at:])

    @staticmethod
    def _meta_str(m: np.ndarray, base: int) -> Optional[str]:
        ln = int(m[base + 15])
        return None if ln == 255 else bytes(m[base: base + ln]).decode("latin-1")

    def _frame(self, line, i, plen, offsets, slot, meta, name) -> RawFrame:
        """RawFrame(line=payload, message_type) + _extract_metadata (mu.py:96-108, mc.py:141-155)."""
        fr = RawFrame(line=self._payload(line, i, plen, offsets, slot), message_type=name)
        r, f = self._meta_str(meta[i], 0), self._meta_str(meta[i], 16)
        for raw, attr, fn in ((r, "rssi", calc_rssi), (f, "freq_afc", calc_afc)):
            if raw is None:
                continue
            try:
                setattr(fr, attr, fn(int(raw)))
            except ValueError:
                self.logger.warning("Could not parse %s value: %s", "RSSI" if attr == "rssi" else "AFC", raw)
        return fr


class MNParser:
    """signalduino/parser/mn.py:20-191: MN frames -> DecodedMessage, the protocol loop on the GPU.

    ``parse(frame)`` / ``parse_batch(frames)`` take RawFrames whose ``line`` is the payload (as the
    reference's SignalParser hands them over).  MN_PATTERN is matched per frame on the host (the
    batched line path, :class:`SignalParser`, does it on the device), then one ``sdx_demod_mn``
    launch runs the rfmode / length / regexMatch / method loop for every matched frame."""

    def __init__(self, protocols: SDProtocols, logger: Optional[logging.Logger] = None, rfmode: Optional[str] = None):
        self.protocols = protocols
        self.logger = logger or logging.getLogger(__name__)
        self.rfmode = rfmode

    def parse(self, frame: RawFrame) -> List[DecodedMessage]:
        return self.parse_batch([frame])[0]

    def parse_batch(self, frames: Sequence[RawFrame]) -> List[List[DecodedMessage]]:
        rows, hexes, meta = [], [], []
        for k, fr in enumerate(frames):
            if not fr.line.upper().startswith("MN"):        # ensure_message_type (base.py:211-213)
                self.logger.debug("Not an MN message: %s", fr.line[:2])
                continue
            m = MN_PATTERN.match(fr.line)
            if not m:
                self.logger.debug("MN message format mismatch: %s", fr.line)
                continue
            rows.append(k)
            hexes.append(m.group(2))
            meta.append((calc_rssi(int(m.group(3))) if m.group(3) else None,
                         calc_mn_afc(int(m.group(4))) if m.group(4) else None))
        out: List[List[DecodedMessage]] = [[] for _ in frames]
        if not rows:
            return out
        bk = None
        for k, res, (rssi, afc) in zip(rows, self.protocols.mn_parse_batch(hexes, self.rfmode), meta):
            bk = bk or self.protocols._bank
            out[k] = [DecodedMessage(protocol_id=str(pid), payload=payload, raw=frames[k],
                                     metadata={"rssi": rssi, "freq_afc": afc, "modulation": bk.mn_modulation[p],
                                               "rfmode": bk.mn_rfmode[p]}) for pid, payload, p in res]
        return out
