#!/usr/bin/env python3
"""sdx_split_lines beside sdx_parse_lines / sdx_select_lines on one chunk of the end-to-end corpus
(tools/bench_lines_e2e.py's lines, the first --chunk of them), HBM-resident, one stream, nothing else
on the device: run it under ``rocprofv3 --kernel-trace --stats`` and read k_split_count / k_split_write
against k_parse_lines from the same trace.  Prints one JSON line: the chunk's bytes and lines, the
bytes the two split kernels move, and the event-timed microseconds per repetition of the split alone
and of the parse alone.

usage: rocprofv3 --kernel-trace --stats -d OUT -- python3 tools/prof_split.py [--lines 1000000 --chunk 250000 --reps 20]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=1_000_000, help="corpus lines (bench_lines_e2e.py's cache)")
    ap.add_argument("--chunk", type=int, default=250_000)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch
    from pysignalduino_amd import frontend, synth
    from pysignalduino_amd.sd_protocols import SDProtocols
    torch.cuda.set_device(0)
    sp = frontend.SignalParser(SDProtocols(mc_mode="fixed"))
    eng = sp.protocols._ensure()
    cache = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"sdx_lines_{args.lines}_45_1-1-1_0.3.npz")
    if os.path.exists(cache):
        z = np.load(cache)
        data, offsets = z["data"], z["offsets"]
    else:
        lines, _ = synth.line_corpus(eng.bank.protocols, args.lines, seed=45, mix=(1, 1, 1), compress_frac=0.3)
        data, offsets, bad = frontend.pack_lines(lines)
        assert not bad
        np.savez(cache, data=data, offsets=offsets)
    C = args.chunk
    o = offsets[: C + 1].astype(np.int64)
    raw = data[: o[-1]]
    assert int(np.count_nonzero(raw == 10)) == C and raw[-1] == 10, "every corpus line ends in its only newline"
    nb = len(raw)
    lb = frontend.LineBatch(eng, raw, o)           # the packed upload: bytes + offsets
    split_off = torch.empty(C + 1, dtype=torch.int64, device=eng.dev)
    count = torch.zeros(2, dtype=torch.int64, device=eng.dev)
    scratch = torch.empty(eng.split_work_ints(nb), dtype=torch.int32, device=eng.dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    t_split, t_parse = [], []
    for r in range(args.reps + 3):
        ev[0].record()
        eng.split_lines(lb.bytes, nb, False, split_off, C, count, scratch)
        ev[1].record()
        lb.launch()
        ev[2].record()
        torch.cuda.synchronize()
        if r >= 3:
            t_split.append(ev[0].elapsed_time(ev[1]) * 1e3)
            t_parse.append(ev[1].elapsed_time(ev[2]) * 1e3)
    assert count.cpu().tolist() == [C, nb] and torch.equal(split_off, lb.offsets), "the split's offsets are the packed ones"
    moved = 2 * nb + 8 * (C + 1) + 2 * 4 * eng.split_work_ints(nb)
    print(json.dumps({"chunk_lines": C, "chunk_bytes": nb, "split_bytes_moved": moved,
                      "split_us_events_median": float(np.median(t_split)),
                      "parse_select_us_events_median": float(np.median(t_parse)), "reps": args.reps}), flush=True)


if __name__ == "__main__":
    main()
