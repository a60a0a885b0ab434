#!/usr/bin/env python
"""Time the route pass alone on planted launch outputs: sdx_route_lines over one chunk of N
result-bearing lines with routes.DEFAULT_ROUTES, HIP events around ITERS calls, beside sdx_mark_repeats
over the same chunk.  The payloads are the reference-recorded ones of tests/golden/lines_golden.json.gz
(1,267 result-bearing lines), cycled in a seeded random order.

  python tools/bench_route_pass.py --lines 250000

``--records`` plants every line's full recorded message list (the golden's records-per-line
mix) as well and times sdx_route_records + sdx_route_skip beside sdx_route_lines in the same run, over that
chunk and over the one where every line has one record (there the new kernel does the same walks).

Run it under ``rocprofv3 --kernel-trace --stats`` for the kernel's own time.  Prints one JSON line; a
sample of the routes and masks (and picks) is checked against ``re.search`` before anything is timed."""
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
    ap.add_argument("--records", action="store_true", help="also time sdx_route_records + sdx_route_skip (route_match='any')")
    args = ap.parse_args()
    import torch
    from pysignalduino_amd import routes, runtime
    from pysignalduino_amd.sd_protocols import SDProtocols
    eng = SDProtocols()._ensure()
    t, n = torch, args.lines
    with gzip.open(os.path.join(REPO, "tests", "golden", "lines_golden.json.gz"), "rt", encoding="utf-8") as fh:
        lists = [[m[1].encode("latin-1") for m in c["e2e"]] for c in json.load(fh) if c.get("e2e")]
    pays = [x[0] for x in lists]
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
    timed = time_calls(t, args.iters)
    calls = {"route_lines_us": lambda: eng.route_lines(dt, ins, n, b["route"], b["mask"], b["skip"], drop_unrouted=True),
             "route_lines_first_match_us": lambda: eng.route_lines(dt, ins, n, b["route"], None, b["skip"], drop_unrouted=True),
             "mark_repeats_us": lambda: eng.mark_repeats(ins, n, rep, scr, st)}
    res = {"lines": n, "routes": len(table), "blob_bytes": len(table.blob), "lds_routes": dt.lds_routes,
           "routed": int((route >= 0).sum()), "distinct_routes": int(len(set(route.tolist()) - {-1})),
           "payload_bytes_mean": float(lens.mean()), "iters": args.iters}
    timed(calls, res)
    if args.records:
        res["records"] = bench_records(eng, t, dt, table, rx, lists, pick, rng, args, timed, ins, b)
    print(json.dumps(res), flush=True)


def time_calls(t, iters):
    def timed(calls, res):
        for name, call in calls.items():
            call()
            e = [t.cuda.Event(enable_timing=True) for _ in range(iters + 1)]
            t.cuda.synchronize()
            e[0].record()
            for i in range(iters):
                call()
                e[i + 1].record()
            t.cuda.synchronize()
            us = [a.elapsed_time(b_) * 1e3 for a, b_ in zip(e, e[1:])]
            res[name] = float(np.median(us))
            res[name.replace("_us", "_min_max_us")] = [float(min(us)), float(max(us))]
    return timed


def bench_records(eng, t, dt, table, rx, lists, pick, rng, args, timed, ins1, b1):
    """The chunk with every line's full record list (same lines, same order) and the one-record chunk ``ins1``:
    sdx_route_records + sdx_route_skip beside sdx_route_lines, interleaved in one run."""
    from pysignalduino_amd import runtime
    n = args.lines
    cnt = np.array([len(x) for x in lists])[pick]
    begin = np.concatenate([[0], np.cumsum(cnt)])
    flat = [p for i in pick.tolist() for p in lists[i]]
    lens = np.array([len(p) for p in flat])
    off = np.concatenate([[0], np.cumsum(lens)])
    desc = np.zeros(n, runtime.DESC_DT)
    desc["rec_begin"], desc["n_rec"], desc["status"] = begin[:-1], cnt, runtime.ST_OK
    rec = np.zeros(len(flat), runtime.RES_DT)
    rec["payload_off"], rec["payload_len"], rec["proto"] = off[:-1], lens, 3
    dev = lambda a: t.from_numpy(np.frombuffer(a.tobytes(), np.uint8).copy()).to(eng.dev)   # noqa: E731
    out = {"desc": dev(desc), "rec": dev(rec), "heap": dev(np.frombuffer(b"".join(flat), np.uint8)), "rec_cap": len(flat),
           "cursor": t.zeros(4, dtype=t.int32, device=eng.dev)}
    insm = [eng.json_in(runtime.KIND_MU, out, {"meta": t.zeros(32 * n, dtype=t.uint8, device=eng.dev)}, n)]
    b = eng.alloc_routes(n, pick=True, views=1)
    eng.route_records(dt, insm, n, b["route"], b["pick"], b["views"], mask=b["mask"])
    t.cuda.synchronize()
    route, mask = b["route"][:n].cpu().numpy(), b["mask"][:n].cpu().numpy().view(np.uint64)
    pk = b["pick"][:n].cpu().numpy().view(np.uint16)
    for i in rng.integers(0, n, args.sample).tolist():
        exp = (0, -1, 0)
        for j, p in enumerate(lists[int(pick[i])]):
            m = sum(1 << r for r, x in enumerate(rx) if x.search(p.decode("latin-1")))
            if m:
                exp = (j, (m & -m).bit_length() - 1, m)
                break
        if (int(pk[i]), int(route[i]), int(mask[i])) != exp:
            raise SystemExit(f"line {i}: pick/route/mask {(int(pk[i]), int(route[i]), hex(int(mask[i])))}, re.search gives {exp}")
    res = {"records": int(len(flat)), "records_per_line_mean": float(cnt.mean()), "records_per_line_max": int(cnt.max()),
           "routed_any": int((route >= 0).sum()), "picked_later": int((pk > 0).sum())}

    def both(ins, mask_):
        eng.route_records(dt, ins, n, b["route"], b["pick"], b["views"], mask=mask_)
        eng.route_skip(ins, n, b["route"], b["skip"], drop_unrouted=True)
    calls = {"one_record_route_lines_us": lambda: eng.route_lines(dt, ins1, n, b1["route"], None, b1["skip"], drop_unrouted=True),
             "one_record_route_records_us": lambda: eng.route_records(dt, ins1, n, b["route"], b["pick"], b["views"]),
             "one_record_route_records_skip_us": lambda: both(ins1, None),
             "one_record_route_lines_mask_us": lambda: eng.route_lines(dt, ins1, n, b1["route"], b1["mask"], b1["skip"],
                                                                       drop_unrouted=True),
             "one_record_route_records_skip_mask_us": lambda: both(ins1, b["mask"]),
             "all_records_route_lines_us": lambda: eng.route_lines(dt, insm, n, b1["route"], None, b1["skip"], drop_unrouted=True),
             "all_records_route_records_us": lambda: eng.route_records(dt, insm, n, b["route"], b["pick"], b["views"]),
             "all_records_route_records_skip_us": lambda: both(insm, None),
             "all_records_route_records_skip_mask_us": lambda: both(insm, b["mask"]),
             "route_skip_us": lambda: eng.route_skip(insm, n, b["route"], b["skip"], drop_unrouted=True)}
    timed(calls, res)
    return res


if __name__ == "__main__":
    main()
