#!/usr/bin/env python
"""Time the route pass alone on planted launch outputs: sdx_route_lines over one chunk of N
result-bearing lines with routes.DEFAULT_ROUTES, HIP events around ITERS calls, beside sdx_mark_repeats
over the same chunk.  The payloads are the reference-recorded ones of tests/golden/lines_golden.json.gz
(1,267 result-bearing lines), cycled in a seeded random order.

  python tools/bench_route_pass.py --lines 250000

Run it under ``rocprofv3 --kernel-trace --stats`` for the kernel's own time.  Prints one JSON line; a
sample of the routes and masks is checked against ``re.search`` before anything is timed."""
import argparse
import gzip
import json
import os
import re
import sys

import numpy as np

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=250_000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--sample", type=int, default=4000, help="lines checked against re.search")
    args = ap.parse_args()
    import torch
    from pysignalduino_amd import routes, runtime
    from pysignalduino_amd.sd_protocols import SDProtocols
    eng = SDProtocols()._ensure()
    t, n = torch, args.lines
    with gzip.open(os.path.join(REPO, "tests", "golden", "lines_golden.json.gz"), "rt", encoding="utf-8") as fh:
        pays = [c["e2e"][0][1].encode("latin-1") for c in json.load(fh) if c.get("e2e")]
    rng = np.random.default_rng(7)
    pick = rng.integers(0, len(pays), n)
    lens = np.array([len(p) for p in pays])[pick]
    off = np.concatenate([[0], np.cumsum(lens)])
    heap = np.frombuffer(b"".join(pays[i] for i in pick.tolist()), np.uint8)
    desc = np.zeros(n, runtime.DESC_DT)
    desc["rec_begin"], desc["n_rec"], desc["status"] = np.arange(n), 1, runtime.ST_OK
    rec = np.zeros(n, runtime.RES_DT)
    rec["payload_off"], rec["payload_len"], rec["proto"] = off[:-1], lens, 3
    dev = lambda a: t.from_numpy(np.frombuffer(a.tobytes(), np.uint8).copy()).to(eng.dev)   # noqa: E731
    out = {"desc": dev(desc), "rec": dev(rec), "heap": dev(heap), "rec_cap": n,
           "cursor": t.zeros(4, dtype=t.int32, device=eng.dev)}
    ins = [eng.json_in(runtime.KIND_MU, out, {"meta": t.zeros(32 * n, dtype=t.uint8, device=eng.dev)}, n)]
    table = routes.RouteTable(routes.DEFAULT_ROUTES)
    dt = eng.route_table(table)
    b = eng.alloc_routes(n)
    rep, scr = eng.alloc_repeat(n)
    st = eng.alloc_repeat_state()
    eng.route_lines(dt, ins, n, b["route"], b["mask"], b["skip"], drop_unrouted=True)
    t.cuda.synchronize()
    route, mask = b["route"][:n].cpu().numpy(), b["mask"][:n].cpu().numpy().view(np.uint64)
    rx = [re.compile(p) for p in table.patterns]
    for i in rng.integers(0, n, args.sample).tolist():
        s = pays[int(pick[i])].decode("latin-1")
        m = sum(1 << r for r, x in enumerate(rx) if x.search(s))
        if int(mask[i]) != m or int(route[i]) != ((m & -m).bit_length() - 1 if m else -1):
            raise SystemExit(f"line {i} ({s!r}): route {route[i]}, mask {int(mask[i]):#x}, re.search gives {m:#x}")
    calls = {"route_lines_us": lambda: eng.route_lines(dt, ins, n, b["route"], b["mask"], b["skip"], drop_unrouted=True),
             "route_lines_first_match_us": lambda: eng.route_lines(dt, ins, n, b["route"], None, b["skip"], drop_unrouted=True),
             "mark_repeats_us": lambda: eng.mark_repeats(ins, n, rep, scr, st)}
    res = {"lines": n, "routes": len(table), "blob_bytes": len(table.blob), "lds_routes": dt.lds_routes,
           "routed": int((route >= 0).sum()), "distinct_routes": int(len(set(route.tolist()) - {-1})),
           "payload_bytes_mean": float(lens.mean()), "iters": args.iters}
    for name, call in calls.items():
        call()
        e = [t.cuda.Event(enable_timing=True) for _ in range(args.iters + 1)]
        t.cuda.synchronize()
        e[0].record()
        for i in range(args.iters):
            call()
            e[i + 1].record()
        t.cuda.synchronize()
        us = [a.elapsed_time(b_) * 1e3 for a, b_ in zip(e, e[1:])]
        res[name] = float(np.median(us))
        res[name.replace("_us", "_min_max_us")] = [float(min(us)), float(max(us))]
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
