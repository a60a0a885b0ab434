#!/usr/bin/env python3
"""What publishing every message of a line costs on the live path, after tools/bench_lines_e2e.py.

One synthetic chunked corpus (synth.line_corpus, bench_lines_e2e.py's) in pinned host memory through three streams
in ONE process, interleaved round by round: the ``json`` stream (decoded[0] per line), ``json_all`` without rules and
``json_all`` with the default dispatch rules.  Prints ONE JSON line: per stream the median lines/s and texts/s over
the rounds with their min / max, and the HIP-event time per chunk of the index pass (sdx_index_records) and of the
dispatch pass (sdx_dispatch_records) on a chunk's launch outputs.

``--against-tree DIR``: is the DEFAULT path where it was?  The ``json`` stream alone, in fresh child processes that
alternate between this tree and DIR, a checkout of the commit to compare with (``git archive`` of it into a folder)
with its own library built there (``python -m pysignalduino_amd.build``): each child imports the Python of its own
tree and loads that tree's libsdx.so, so host code and kernels are both compared.  Reports both medians, their
difference and the run-to-run spread of each.

usage: python tools/bench_stream_all.py [--lines 400000 --chunk 100000 --passes 20 --rounds 5 --against-tree DIR]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def corpus(bank, n):
    from pysignalduino_amd import frontend, synth
    cache = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"sdx_lines_{n}_45_1-1-1_0.3.npz")
    if os.path.exists(cache):
        z = np.load(cache)
        return z["data"], z["offsets"]
    lines, _ = synth.line_corpus(bank.protocols, n, seed=45, mix=(1, 1, 1), compress_frac=0.3)
    data, offsets, bad = frontend.pack_lines(lines)
    assert not bad
    np.savez(cache, data=data, offsets=offsets)
    return data, offsets


def n_texts(r) -> int:
    return int(np.count_nonzero(r.len)) + sum(len(x) if isinstance(x, list) else isinstance(x, str) for x in r.host.values())


def one_pass(ls, chunks, passes):
    """-> (seconds, lines, texts) of ``passes`` passes over the chunks, first submit -> last result landed."""
    import torch
    torch.cuda.synchronize()
    lines = texts = 0
    t0 = time.perf_counter()
    for k in range(passes * len(chunks)):
        ls.submit_packed(*chunks[k % len(chunks)])
        for r in ls.poll():
            lines, texts = lines + r.n, texts + n_texts(r)
    for r in ls.drain():
        lines, texts = lines + r.n, texts + n_texts(r)
    return time.perf_counter() - t0, lines, texts


def event_ms(torch, fn, reps=20):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=400_000)
    ap.add_argument("--chunk", type=int, default=100_000)
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--against-tree", default=None, metavar="DIR")
    ap.add_argument("--child", default=None, metavar="TREE", help=argparse.SUPPRESS)   # the json stream alone, of TREE
    args = ap.parse_args()
    if args.against_tree and not args.child:
        cmd = [sys.executable, os.path.abspath(__file__), "--lines", str(args.lines), "--chunk", str(args.chunk),
               "--passes", str(args.passes), "--rounds", "3", "--child"]
        rates = {"tree": [], "against": []}
        env = dict(os.environ)
        env.pop("SDX_LIB", None)     # every child loads its own tree's library
        for _ in range(args.rounds):
            for name, tree in (("tree", REPO), ("against", os.path.abspath(args.against_tree))):
                run = subprocess.run(cmd + [tree], env=env, cwd=tree, capture_output=True, text=True, timeout=600)
                if run.returncode:
                    raise SystemExit(f"the {name} run failed ({run.returncode}):\n{run.stderr[-2000:]}")
                out = run.stdout
                rates[name].append(json.loads(out.strip().splitlines()[-1])["json"]["lines_per_s"]["median"])
        t, a = np.median(rates["tree"]), np.median(rates["against"])
        spread = lambda v: (max(v) - min(v)) / np.median(v)   # noqa: E731
        print(json.dumps({"metric": "json stream lines/s, this tree against the tree " + args.against_tree, "unit": "lines/s",
                          "tree": stats(rates["tree"]), "against": stats(rates["against"]), "difference_rel": float(t / a - 1),
                          "spread_rel": {"tree": float(spread(rates["tree"])), "against": float(spread(rates["against"]))},
                          "runs_each": args.rounds, "alternating": True}), flush=True)
        return
    sys.path.insert(0, args.child or REPO)
    import torch
    from pysignalduino_amd import frontend, runtime
    assert os.path.dirname(os.path.dirname(os.path.abspath(frontend.__file__))) == os.path.abspath(args.child or REPO)
    from pysignalduino_amd.sd_protocols import SDProtocols
    torch.cuda.set_device(0)
    sp = frontend.SignalParser(SDProtocols(mc_mode="fixed"))
    eng = sp.protocols._ensure()
    data, offsets = corpus(eng.bank, args.lines)
    C = args.chunk
    nck = (len(offsets) - 1) // C
    chunks = []
    for k in range(nck):
        o = offsets[k * C: (k + 1) * C + 1].astype(np.int64)
        chunks.append((torch.from_numpy(data[o[0]: o[-1]].copy()).pin_memory(), o - o[0]))
    maxb = max(b.numel() for b, _ in chunks)
    modes = {"json": dict(output="json")}
    if not args.child:
        modes.update(json_all=dict(output="json_all"), json_all_rules=dict(output="json_all", rules=True))
    streams = {m: sp.stream(chunk_lines=C, chunk_bytes=maxb, **kw) for m, kw in modes.items()}
    for ls in streams.values():      # warm-up: every stage once
        one_pass(ls, chunks, 1)
    rate = {m: ([], []) for m in streams}
    per_line = {}
    for _ in range(args.rounds):
        for m, ls in streams.items():
            dt, lines, texts = one_pass(ls, chunks, args.passes)
            rate[m][0].append(lines / dt)
            rate[m][1].append(texts / dt)
            per_line[m] = texts / lines
    res = {"metric": "stream lines/s and texts/s end to end, the three outputs interleaved in one process", "unit": "lines/s",
           "lines_per_pass": nck * C, "chunk_lines": C, "passes": args.passes, "rounds": args.rounds,
           **{m: {"lines_per_s": stats(rate[m][0]), "texts_per_s": stats(rate[m][1]), "texts_per_line": per_line[m]} for m in streams}}
    if not args.child:
        # the two passes alone, on the launch outputs the rules stream's first slot still holds (a chunk of C lines)
        ls = streams["json_all_rules"]
        s = ls.slots[0]
        lo = {"meta": s.lb.meta, "pat_val": s.lb.pat_val, "cp_slot": s.lb.cp_slot}
        kinds = (("MU", runtime.KIND_MU), ("MS", runtime.KIND_MS), ("MC", runtime.KIND_MC), ("MN", runtime.KIND_MN))
        ins = [eng.json_in(kd, s.outs[nm], lo, C, 2) for nm, kd in kinds if nm in s.outs]
        ins0 = [eng.json_in(kd, s.douts[nm], lo, C, 0) for nm, kd in kinds if nm in s.douts]
        res["pass_ms_per_chunk"] = {"dispatch_records": event_ms(torch, lambda: eng.dispatch_records(ls.drules, ins, C, s.dp)),
                                    "index_records": event_ms(torch, lambda: eng.index_records(ins0, C, s.idx))}
        res["records_per_chunk"] = int(s.idx["first"][C].item())
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
