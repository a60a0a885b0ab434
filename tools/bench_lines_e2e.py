#!/usr/bin/env python3
"""End-to-end front-end rate with the PCIe transfers (controller.py:245-264).

The drop-in use (SignalduinoController._parser_task -> SignalParser.parse_line) has raw lines in host
memory and wants decoded results back in host memory.  This tool streams framed firmware lines from
pinned host memory through the product streaming API (``SignalParser.stream``,
pysignalduino_amd/stream.py: H2D, parse + select, demodulation + serialisation, D2H of successive
chunks overlapping on four HIP streams, the host never waiting on a chunk it has just enqueued) and
prints ONE JSON line: value = lines/s end to end (first submit -> last chunk's results landed in
pinned host memory), beside the kernels' own time per chunk, the PCIe bytes each way and the bound
(the stage whose per-chunk time is the largest: H2D, kernels, D2H or the host).  ``--output json``
streams the MQTT texts (what BatchingParserTask publishes) instead of the wire form.  --check
compares chunk 0's results with SignalParser.parse_lines / parse_lines_json on the same lines.

``--bytes`` feeds the same corpus as a transport delivers it: one raw byte string per pass (the lines, each
with the firmware's newline, one after another) in pinned memory, handed to ``LineStream.submit_bytes`` in
pieces of a chunk's share of the bytes (they end mid-line: the tail is carried) -- the lines are found on the
device (sdx_split_lines) and no offsets go up over PCIe.  There --check compares the first --chunk lines' results with the packed mode's.

usage: python tools/bench_lines_e2e.py [--lines 1000000 --chunk 250000 --passes 4 --output wire --bytes --check]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def copy_rates(torch, host_bytes):
    """Pinned H2D and D2H rates of this host link for a chunk-sized buffer (HIP events, 5 copies)."""
    h = torch.from_numpy(host_bytes)
    d = torch.empty(h.numel(), dtype=torch.uint8, device="cuda")
    rates = []
    for src, dst in ((h, d), (d, h)):
        dst.copy_(src, non_blocking=True)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            dst.copy_(src, non_blocking=True)
        e1.record()
        torch.cuda.synchronize()
        rates.append(5 * h.numel() / (e0.elapsed_time(e1) * 1e-3))
    return rates[0], rates[1]


def per_line(results, bank):
    """Per line of the chunks: json -> its text (or the exception's type); wire -> kind, status and the
    (protocol id, payload) list of its records (or of the batch API's objects for the lines it took)."""
    rows = []
    for r in results:
        if r.json is not None:
            rows += [type(t) if isinstance(t, Exception) else t for t in r.texts()]
            continue
        pid = {"MU": bank.mu_pids, "MS": bank.ms_pids, "MC": bank.mc_pids, "MN": bank.mn_pids}
        out = [[int(k), int(s)] for k, s in zip(r.kind.tolist(), r.status.tolist())]
        for j, nm in enumerate(r.names):
            d, rec, heap = r.decode(j)
            hs = heap.tobytes().decode("latin-1")
            for i in np.nonzero(d["n_rec"])[0].tolist():
                b, k = int(d[i]["rec_begin"]), int(d[i]["n_rec"])
                out[i] += [(str(pid[nm][int(x["proto"])]), hs[int(x["payload_off"]): int(x["payload_off"]) + int(x["payload_len"])])
                           for x in rec[b: b + k]]
        for i, h in r.host.items():
            out[i] = out[i][:2] + ([type(h)] if isinstance(h, Exception) else [(m.protocol_id, m.payload) for m in h])
        rows += out
    return rows


def check_bytes(sp, chunk0, head, C, output, lag):
    """--bytes --check: the first C lines' results against the packed mode's on the same lines."""
    b, o = chunk0
    ref = sp.stream(chunk_lines=C, chunk_bytes=b.numel(), output=output, lag=lag)
    ref.submit_packed(b, o)
    bank = sp.protocols._bank
    exp = per_line([r.detach() for r in ref.drain()], bank)
    got = per_line(head, bank)[:C]
    raw = b.numpy()
    bad = sum(e != g for e, g in zip(exp, got)) + abs(len(exp) - len(got))
    k, texts = 0, 0
    for r in head:      # ChunkResult.line(i): the line's bytes, terminator included
        for i in range(0, r.n, 997):
            if k + i < C:
                texts += r.line(i) != raw[o[k + i]: o[k + i + 1]].tobytes()
        k += r.n
    return {"lines": C, "mismatches": int(bad + texts), "against": "submit_packed"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=1_000_000, help="corpus lines (streamed --passes times)")
    ap.add_argument("--chunk", type=int, default=250_000)
    ap.add_argument("--passes", type=int, default=40, help="timed passes over the corpus (40 x 1M lines: ~0.2 s, steadier than 8)")
    ap.add_argument("--lag", type=int, default=3)
    ap.add_argument("--output", default="wire", choices=("wire", "json"))
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--bytes", action="store_true", help="feed raw bytes through submit_bytes (lines split on the device)")
    ap.add_argument("--profile", action="store_true", help="cProfile the timed loop (top 30 by own time, stderr)")
    ap.add_argument("--repeat", type=int, default=1, help="emit each synthetic line R times consecutively (as a stick "
                    "delivers telegrams): --lines / R distinct lines, --lines lines in all")
    ap.add_argument("--collapse", action="store_true", help="stream with collapse_repeats=True (repeats are never serialised)")
    ap.add_argument("--window", type=float, default=None, metavar="SECONDS",
                    help="with --collapse: stream with repeat_window=SECONDS; the lines get synthetic, evenly spaced "
                         "arrival times (SECONDS / 8 apart, so a burst of --repeat 4 stays inside the window; they run "
                         "on over the passes)")
    ap.add_argument("--routes", default=None, metavar="LIST", help="stream with payload routes (DESIGN.md §4l): 'default' "
                    "(routes.DEFAULT_ROUTES) or one regex, which becomes a one-route list")
    ap.add_argument("--drop-unrouted", action="store_true", help="with --routes: unrouted lines are never serialised")
    ap.add_argument("--route-match", default="first", choices=("first", "any"), help="with --routes: 'any' publishes a "
                    "line's first message that a route matches (DESIGN.md §4m)")
    args = ap.parse_args()
    if args.window is not None and not args.collapse:
        ap.error("--window needs --collapse")
    if args.drop_unrouted and args.routes is None:
        ap.error("--drop-unrouted needs --routes")
    if args.route_match != "first" and args.routes is None:
        ap.error("--route-match any needs --routes")
    import torch
    from pysignalduino_amd import frontend, runtime, synth
    from pysignalduino_amd.sd_protocols import SDProtocols
    torch.cuda.set_device(0)
    sp = frontend.SignalParser(SDProtocols(mc_mode="fixed"))
    bk = sp.protocols._ensure().bank
    cache = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"sdx_lines_{args.lines}_45_1-1-1_0.3.npz")
    if os.path.exists(cache):
        z = np.load(cache)
        data, offsets = z["data"], z["offsets"]
    else:
        lines, _ = synth.line_corpus(bk.protocols, args.lines, seed=45, mix=(1, 1, 1), compress_frac=0.3)
        data, offsets, bad = frontend.pack_lines(lines)
        assert not bad
        np.savez(cache, data=data, offsets=offsets)
    if args.repeat > 1:   # the first lines / R corpus lines, each R times in a row (one gather, no Python loop)
        R, m = args.repeat, (len(offsets) - 1) // args.repeat
        idx = np.repeat(np.arange(m), R)
        lens = np.diff(offsets)[idx]
        new_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        src = np.repeat(offsets[:-1][idx] - new_off[:-1], lens) + np.arange(int(new_off[-1]))
        data, offsets = data[src], new_off
    ckw = {"collapse_repeats": True} if args.collapse else {}
    if args.routes is not None:
        from pysignalduino_amd import routes as routesmod
        ckw["routes"] = routesmod.RouteTable(routesmod.DEFAULT_ROUTES if args.routes == "default" else [("only", args.routes)])
        ckw["drop_unrouted"] = args.drop_unrouted
        if args.route_match != "first":
            ckw["route_match"] = args.route_match
    routed = [0, 0, 0]   # --routes: lines routed, JSON bytes copied out, chunks (over all results)
    timed = args.window is not None
    if timed:
        ckw["repeat_window"] = args.window
        spacing_us = int(round(args.window / 8 * 1e6))
    marked = [0, 0]   # --window: repeats marked, lines seen (over all results)
    C = args.chunk
    nck = (len(offsets) - 1) // C
    assert nck >= 2, "need at least two chunks"
    # the chunks in pinned host memory (the lines as the transports deliver them), offsets rebased
    chunks = []
    for k in range(nck):
        o = offsets[k * C: (k + 1) * C + 1].astype(np.int64)
        b = torch.from_numpy(data[o[0]: o[-1]].copy()).pin_memory()
        chunks.append((b, o - o[0]))
    maxb = max(b.numel() for b, _ in chunks)
    if args.bytes:
        # the pass as one byte string: the corpus lines carry the firmware's '\n' (synth.frame), so the
        # string is their concatenation; pieces of equal size, so all but the last end mid-line.  A piece
        # holds about C lines: room for a tenth more, and for the carried line start
        o = offsets[: nck * C + 1].astype(np.int64)
        raw_np = data[: o[-1]]
        assert (raw_np[o[1:] - 1] == 10).all() and int(np.count_nonzero(raw_np == 10)) == nck * C, \
            "every corpus line ends in its only newline"
        raw = torch.from_numpy(raw_np.copy()).pin_memory()
        step = -(-raw.numel() // nck)
        feed = [raw[k * step: (k + 1) * step] for k in range(nck)]
        assert all(p.is_pinned() for p in feed)    # uploaded from where they are, as the packed mode's chunks
        ls = sp.stream(chunk_lines=C + C // 10 + 16, chunk_bytes=step + 65536, output=args.output, lag=args.lag,
                       **ckw)
        submit = ls.submit_bytes
        if timed:   # one time per read buffer: that of the last line it ends
            clock = [0]

            def submit(piece):   # noqa: F811
                clock[0] += C * spacing_us
                return ls.submit_bytes(piece, time=clock[0])
    else:
        feed = chunks
        ls = sp.stream(chunk_lines=C, chunk_bytes=maxb, output=args.output, lag=args.lag, **ckw)
        submit = lambda ch: ls.submit_packed(*ch)   # noqa: E731
        if timed:   # one time per line, evenly spaced, running on from chunk to chunk
            ramp = np.arange(C, dtype=np.int64) * spacing_us
            tbuf = np.empty(C, np.int64)    # one buffer: the stream copies a chunk's times as it takes them
            clock = [0]

            def submit(ch):   # noqa: F811
                np.add(ramp, clock[0], out=tbuf)
                clock[0] += C * spacing_us
                return ls.submit_packed(*ch, times=tbuf)
    # warm-up: one pass through every stage (kernels loaded, buffers touched)
    for ch in feed:
        submit(ch)
    ls.drain()
    ls.kernel_events.clear()
    ls.h2d_bytes = ls.d2h_bytes = 0
    nsteps = nck * args.passes
    first = None
    host_t = 0.0
    torch.cuda.synchronize()
    prof = None
    if args.profile:
        import cProfile
        prof = cProfile.Profile()
        prof.enable()
    t0 = time.perf_counter()
    head = []     # --bytes --check: the results of the first chunks, until they cover C lines
    for k in range(nsteps):
        h0 = time.perf_counter()
        submit(feed[k % nck])
        for r in ls.poll():
            if timed:
                marked[0] += int(np.count_nonzero(r.repeat))
                marked[1] += r.n
            if r.json is not None:
                routed[1] += len(r.json)
                routed[2] += 1
            if args.routes is not None:
                routed[0] += int(np.count_nonzero(r.route >= 0))
            if first is None and args.check:
                first = r.detach()
            if args.bytes and args.check and sum(x.n for x in head) < C:
                head.append(r.detach())
        host_t += time.perf_counter() - h0
    for r in ls.drain():
        if timed:
            marked[0] += int(np.count_nonzero(r.repeat))
            marked[1] += r.n
        if r.json is not None:
            routed[1] += len(r.json)
            routed[2] += 1
        if args.routes is not None:
            routed[0] += int(np.count_nonzero(r.route >= 0))
        if first is None and args.check:
            first = r.detach()
        if args.bytes and args.check and sum(x.n for x in head) < C:
            head.append(r.detach())
    dt = time.perf_counter() - t0
    nsteps = len(ls.kernel_events)     # the chunks queued (--bytes: the stream cuts them)
    if prof is not None:
        import pstats
        prof.disable()
        pstats.Stats(prof, stream=sys.stderr).sort_stats("tottime").print_stats(30)
    total = nck * C * args.passes
    ke = ls.kernel_events
    k_parse = float(np.median([a.elapsed_time(b) * 1e-3 for a, b, _, _ in ke]))
    k_demod = float(np.median([c.elapsed_time(d) * 1e-3 for _, _, c, d in ke]))
    span = [ke[i][0].elapsed_time(ke[i][3]) * 1e-3 for i in range(len(ke))]
    # the device's time per chunk over the whole run: first chunk's parse start -> last chunk's demod
    # end, / chunks (consecutive chunks' demodulations overlap on two streams, so the per-chunk event
    # pairs above include their sharing and do not add up)
    dev_per_chunk = ke[0][0].elapsed_time(ke[-1][3]) * 1e-3 / len(ke)
    per_chunk = dt / nsteps
    h2d_rate, d2h_rate = copy_rates(torch, chunks[0][0].numpy())
    stages = {"kernels (parse + demod + serialise)": min(k_parse + k_demod, dev_per_chunk),
              "H2D": ls.h2d_bytes / nsteps / h2d_rate, "D2H": ls.d2h_bytes / nsteps / d2h_rate,
              "host (submit + poll)": host_t / nsteps}
    res = {
        "metric": "raw firmware lines/sec end to end: pinned host lines -> parse + demodulate + serialise -> results "
                  "in pinned host memory (PCIe both ways, overlapped; SignalParser.stream)",
        "value": total / dt, "unit": "lines/s", "n_gpus": 1, "lines": total, "chunk_lines": C, "lag": args.lag,
        "repeat": args.repeat, "collapse": bool(args.collapse),
        **({"repeat_window_s": args.window, "time_spacing_us": spacing_us, "repeats_marked": marked[0],
            "lines_seen": marked[1]} if timed else {}),
        **({"routes": args.routes, "drop_unrouted": bool(args.drop_unrouted), "route_match": args.route_match,
            "lines_routed": routed[0]}
           if args.routes is not None else {}),
        **({"json_bytes_per_chunk": routed[1] / routed[2]} if routed[2] else {}),
        "output": args.output, "input": "bytes" if args.bytes else "packed", "chunks": nsteps, "ms_per_chunk": 1e3 * per_chunk,
        "kernels_ms_per_chunk": {"parse+select": 1e3 * k_parse, "demod+serialise": 1e3 * k_demod},
        "chunk_span_ms_median": 1e3 * float(np.median(span)),
        "host_ms_per_chunk": 1e3 * host_t / nsteps,
        "hbm_resident_lines_per_s": C / (k_parse + k_demod),
        "device_ms_per_chunk": 1e3 * dev_per_chunk, "device_lines_per_s": C / dev_per_chunk,
        "pcie": {"h2d_bytes_per_line": ls.h2d_bytes / total, "d2h_bytes_per_line": ls.d2h_bytes / total,
                 "h2d_GB_per_s": ls.h2d_bytes / dt / 1e9, "d2h_GB_per_s": ls.d2h_bytes / dt / 1e9},
        "stage_ms_per_chunk": {k: 1e3 * v for k, v in stages.items()},
        "link_GB_per_s": {"h2d": h2d_rate / 1e9, "d2h": d2h_rate / 1e9},
        "data": "synthetic firmware lines (synth.line_corpus: MU/MS/MC 1/3 each, 30 % of MU/MS Mred=1 compressed)",
    }
    res["bound"] = max(stages, key=stages.get)
    if args.check and args.bytes:
        res["check"] = check_bytes(sp, chunks[0], head, C, args.output, args.lag)
        if res["check"]["mismatches"]:
            print(json.dumps(res), flush=True)
            raise SystemExit(f"--check: {res['check']['mismatches']} lines differ from the packed mode's")
    elif args.check:
        b, o = chunks[0]
        b = b.numpy()
        lines = [b[o[i]: o[i + 1]].tobytes() for i in range(C)]
        bad = 0
        if args.output == "json":
            exp = sp.parse_lines_json(lines)
            got = first.texts()
            for i in range(C):
                e, g = exp[i], got[i]
                if isinstance(e, Exception):
                    bad += not isinstance(g, type(e))
                else:
                    bad += e != g
        else:
            exp = sp.parse_lines(lines)
            lk = {runtime.LINE_MU: "MU", runtime.LINE_MS: "MS", runtime.LINE_MC: "MC", runtime.LINE_MN: "MN"}
            names = first.names
            dec = {nm: first.decode(j) for j, nm in enumerate(names)}
            pid = {"MU": bk.mu_pids, "MS": bk.ms_pids, "MC": bk.mc_pids, "MN": bk.mn_pids}
            for i in range(C):
                e = exp[i]
                if i in first.host:
                    g = first.host[i]
                    bad += (type(g) is not type(e)) if isinstance(e, Exception) else \
                        [(m.protocol_id, m.payload) for m in g] != [(m.protocol_id, m.payload) for m in e]
                    continue
                nm = lk.get(int(first.kind[i]))
                if isinstance(e, Exception) or nm is None or nm not in dec or int(first.status[i]) != runtime.LS_OK:
                    bad += (not isinstance(e, Exception)) and bool(e)
                    continue
                d, rc, h = dec[nm]
                dd = d[i]
                got = [(str(pid[nm][int(x["proto"])]),
                        h[int(x["payload_off"]): int(x["payload_off"]) + int(x["payload_len"])].tobytes().decode("latin-1"))
                       for x in rc[int(dd["rec_begin"]): int(dd["rec_begin"]) + int(dd["n_rec"])]]
                bad += got != [(m.protocol_id, m.payload) for m in e]
        res["check"] = {"lines": C, "mismatches": int(bad)}
        if bad:
            print(json.dumps(res), flush=True)
            raise SystemExit(f"--check: {bad} mismatching lines")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
