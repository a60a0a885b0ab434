#!/usr/bin/env python
"""Time the receiver-profile pass alone on planted launch outputs: sdx_filter_records (its three
launches) over one chunk of N result-bearing lines, HIP events around ITERS calls, for a table that enables
everything and for one of four profiles that each enable a random half of every kind's classes -- beside
sdx_route_records over the SAME chunk in the same run (it reads the same descriptors and records and then walks
every payload through the route DFAs).  The chunk plants the reference-recorded message lists of
tests/golden/lines_golden.json.gz (1,267 result-bearing MU / MS lines, about 2,600 records, at most 8 a line) with
their real class indices, cycled in a seeded random order; the lines' record ranges stand in a random order in the
record arrays, as a launch's units reserve them.

  python tools/bench_profile_pass.py --lines 250000
  python tools/bench_profile_pass.py --lines 250000 --stream 200000     # + the stream's cost when nothing is removed

``--stream M``: lines/s of a json LineStream over M synthetic lines with ReceiverProfiles([Profile()]) against the
same stream without profiles, in one process, alternating (A B B A A B), three rounds each.

Prints one JSON line; a sample of the filtered lines is checked against the definition before anything is timed."""
import argparse
import gzip
import json
import os
import sys
import time

import numpy as np

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=250_000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--sample", type=int, default=4000, help="lines checked against the definition")
    ap.add_argument("--stream", type=int, default=0, help="also the stream A/B over this many synthetic lines")
    ap.add_argument("--chunk", type=int, default=50_000, help="--stream: lines per chunk")
    args = ap.parse_args()
    import torch
    from pysignalduino_amd import routes, runtime
    from pysignalduino_amd.profiles import Profile, ReceiverProfiles
    from pysignalduino_amd.sd_protocols import SDProtocols
    protocols = SDProtocols()
    eng = protocols._ensure()
    bank = protocols._bank
    t, n = torch, args.lines
    with gzip.open(os.path.join(REPO, "tests", "golden", "lines_golden.json.gz"), "rt", encoding="utf-8") as fh:
        lists = [c["e2e"] for c in json.load(fh) if c.get("e2e")]
    cls = [{str(p): i for i, p in enumerate(x)} for x in (bank.mu_pids, bank.ms_pids)]
    kind_of = np.array([("MU", "MS").index(x[0][3][1]) for x in lists])
    rng = np.random.default_rng(7)
    pick = rng.integers(0, len(lists), n)
    order = rng.permutation(n)
    dev = lambda a: t.from_numpy(np.frombuffer(a.tobytes(), np.uint8).copy()).to(eng.dev)   # noqa: E731
    meta = t.zeros(32 * n, dtype=t.uint8, device=eng.dev)
    outs, ins, host = [], [], []
    for kd in (0, 1):
        desc = np.zeros(n, runtime.DESC_DT)
        mine = order[kind_of[pick[order]] == kd]           # this kind's lines, in the order their ranges stand
        cnt = np.array([len(lists[i]) for i in pick[mine]])
        begin = np.concatenate([[0], np.cumsum(cnt)])
        desc["rec_begin"][mine], desc["n_rec"][mine] = begin[:-1], cnt
        flat = [(m[1].encode("latin-1"), cls[kd][m[0]], g) for g in mine.tolist() for m in lists[pick[g]]]
        lens = np.array([len(p) for p, _, _ in flat])
        off = np.concatenate([[0], np.cumsum(lens)])
        rec = np.zeros(len(flat), runtime.RES_DT)
        rec["payload_off"], rec["payload_len"] = off[:-1], lens
        rec["proto"], rec["msg"] = [c for _, c, _ in flat], [g for _, _, g in flat]
        out = {"desc": dev(desc), "rec": dev(rec), "heap": dev(np.frombuffer(b"".join(p for p, _, _ in flat), np.uint8)),
               "rec_cap": len(rec), "heap_cap": int(off[-1]), "n": n,
               "cursor": t.tensor([len(rec), int(off[-1]), 0, 0], dtype=t.int32, device=eng.dev)}
        outs.append(out)
        host.append((desc, rec))
        ins.append(eng.json_in(kd, out, {"meta": meta}, n))
    src = rng.integers(0, 4, n).astype(np.int32)
    d_src = t.from_numpy(src).to(eng.dev)
    ids = [sorted(set(map(str, x))) for x in (bank.mu_pids, bank.ms_pids)]
    halves = [Profile(whitelist=[p for x in ids for p in rng.choice(x, len(x) // 2, replace=False)]) for _ in range(4)]
    tables = {"all": ReceiverProfiles([Profile()], [0, 0, 0, 0]), "half": ReceiverProfiles(halves, [0, 1, 2, 3])}
    bufs = eng.alloc_profiles(n, outs)
    res = {"lines": n, "records": int(sum(len(r) for _, r in host)), "iters": args.iters,
           "records_per_line_mean": float(sum(len(r) for _, r in host) / n), "records_per_line_max": int(max(len(x) for x in lists))}
    for name, rp in tables.items():                       # the definition on a sample, before anything is timed
        f = eng.filter_records(rp, ins, n, bufs, source=d_src)
        t.cuda.synchronize()
        kept = 0
        for kd in (0, 1):
            d = f[kd]["desc"][: 8 * n].cpu().numpy().view(runtime.DESC_DT)
            total = int(f[kd]["cursor"][0].item())
            r = f[kd]["rec"][: 16 * total].cpu().numpy().view(runtime.RES_DT)
            kept += total
            d0, r0 = host[kd]
            pids = (bank.mu_pids, bank.ms_pids)[kd]
            for g in rng.integers(0, n, args.sample).tolist():
                on = rp.enabled_ids(bank, int(src[g]), kd)
                want = [x for x in r0[int(d0[g]["rec_begin"]): int(d0[g]["rec_begin"]) + int(d0[g]["n_rec"])] if str(pids[int(x["proto"])]) in on]
                got = r[int(d[g]["rec_begin"]): int(d[g]["rec_begin"]) + int(d[g]["n_rec"])]
                if len(want) != len(got) or any(a.tobytes() != b.tobytes() for a, b in zip(want, got)):
                    raise SystemExit(f"{name}: line {g} of kind {kd}: {len(got)} records, the definition gives {len(want)}")
            if total and not (np.diff(r["msg"].astype(np.int64)) >= 0).all():
                raise SystemExit(f"{name}: kind {kd}'s records are not in line order")
        res[name + "_kept_records"] = kept
    table = routes.RouteTable(routes.DEFAULT_ROUTES)
    dt = eng.route_table(table)
    b = eng.alloc_routes(n, mask=False, skip=False, pick=True, views=2)
    dts = {name: eng.profile_table(rp) for name, rp in tables.items()}
    calls = {"filter_all_us": lambda: eng.filter_records(dts["all"], ins, n, bufs, source=d_src),
             "filter_half_us": lambda: eng.filter_records(dts["half"], ins, n, bufs, source=d_src),
             "route_records_us": lambda: eng.route_records(dt, ins, n, b["route"], b["pick"], b["views"]),
             "filter_all_again_us": lambda: eng.filter_records(dts["all"], ins, n, bufs, source=d_src)}
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
    if args.stream:
        res["stream"] = bench_stream(protocols, args.stream, args.chunk)
    print(json.dumps(res), flush=True)


def bench_stream(protocols, m, chunk):
    """lines/s of a json stream with one all-enabled profile (B) against the stream as it is (A): A B B A A B."""
    import torch
    from pysignalduino_amd import synth
    from pysignalduino_amd.frontend import SignalParser
    from pysignalduino_amd.profiles import Profile, ReceiverProfiles
    sp = SignalParser(protocols)
    raw, _ = synth.line_corpus(protocols._bank.protocols, m, seed=91)
    lines = [ln.decode("latin-1") for ln in raw]
    nbytes = 2 * max(sum(len(x) for x in lines[a: a + chunk]) for a in range(0, m, chunk))
    streams = {"A": sp.stream(chunk_lines=chunk, chunk_bytes=nbytes, lag=3),
               "B": sp.stream(chunk_lines=chunk, chunk_bytes=nbytes, lag=3, profiles=ReceiverProfiles([Profile()]))}

    def run(ls):
        torch.cuda.synchronize()
        ls.kernel_events.clear()
        t0 = time.perf_counter()
        texts = host = 0
        for a in range(0, m, chunk):
            ls.submit(lines[a: a + chunk])
            for r in ls.poll():
                texts += int((r.len > 0).sum())
                host += len(r.host)
        for r in ls.drain():
            texts += int((r.len > 0).sum())
            host += len(r.host)
        rate = m / (time.perf_counter() - t0)
        demod = [k[2].elapsed_time(k[3]) * 1e3 for k in ls.kernel_events]     # stage B of every chunk, on the device
        return rate, texts, host, float(np.median(demod))
    for ls in streams.values():       # warm-up: allocations, first launches
        run(ls)
    rates, demod, texts, host = {"A": [], "B": []}, {"A": [], "B": []}, {}, {}
    for k in "ABBAAB":
        r, texts[k], host[k], d = run(streams[k])
        rates[k].append(r)
        demod[k].append(d)
    return {"lines": m, "chunk": chunk, "order": "ABBAAB", "lines_per_s_without": rates["A"], "lines_per_s_all_enabled": rates["B"],
            "ratio_of_medians": float(np.median(rates["B"]) / np.median(rates["A"])), "texts": texts, "host_resolved_lines": host,
            "stage_b_us_per_chunk_without": demod["A"], "stage_b_us_per_chunk_all_enabled": demod["B"]}


if __name__ == "__main__":
    main()
