#!/usr/bin/env python
"""Time the dispatch-rule pass alone on planted launch outputs: sdx_dispatch_records (its three
launches) over one chunk of N result-bearing lines, HIP events around ITERS calls -- alternating, call by call, with
sdx_filter_records over the SAME chunk with everything enabled.  That pass moves the same records through the same
count -> scan -> write idiom without reading a payload, so the difference is what the payload comparisons cost.  The
chunk is §4n's: the reference-recorded message lists of tests/golden/lines_golden.json.gz (1,267 result-bearing
MU / MS lines, 2,526 records, at most 8 a line) with their real class indices, cycled in a seeded random order; the
lines' record ranges stand in a random order in the record arrays, as a launch's units reserve them.

  python tools/bench_dispatch_pass.py --lines 250000

Prints one JSON line; a sample of the reduced lines is checked against the definition (DispatchRules.reduce over
the recorded lists) before anything is timed."""
import argparse
import gzip
import json
import os
import sys

import numpy as np

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=250_000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--sample", type=int, default=4000, help="lines checked against the definition")
    args = ap.parse_args()
    import torch
    from pysignalduino_amd import runtime
    from pysignalduino_amd.dispatch import DispatchRules
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
    rules = {"default": DispatchRules(), "no_rule": DispatchRules(max_repeat=0, drop_equal=False)}
    structs = {k: r.struct(bank) for k, r in rules.items()}
    dbufs = eng.alloc_dispatch(n, outs)
    pbufs = eng.alloc_profiles(n, outs)
    res = {"lines": n, "records": int(sum(len(r) for _, r in host)), "iters": args.iters,
           "payload_bytes": int(sum(o["heap_cap"] for o in outs)),
           "records_per_line_mean": float(sum(len(r) for _, r in host) / n), "records_per_line_max": int(max(len(x) for x in lists))}
    for name, rl in rules.items():                        # the definition on a sample, before anything is timed
        f = eng.dispatch_records(structs[name], ins, n, dbufs)
        t.cuda.synchronize()
        kept = 0
        for kd in (0, 1):
            d = f[kd]["desc"][: 8 * n].cpu().numpy().view(runtime.DESC_DT)
            total = int(f[kd]["cursor"][0].item())
            r = f[kd]["rec"][: 16 * total].cpu().numpy().view(runtime.RES_DT)
            kept += total
            d0, r0 = host[kd]
            for g in rng.integers(0, n, args.sample).tolist():
                if kind_of[pick[g]] != kd:
                    continue
                lst = lists[pick[g]]
                red = rl.reduce(bank, kd, lst)
                keep_idx = [i for i, m in enumerate(lst) if any(m is k for k in red)]
                want = r0[int(d0[g]["rec_begin"]): int(d0[g]["rec_begin"]) + int(d0[g]["n_rec"])][keep_idx]
                got = r[int(d[g]["rec_begin"]): int(d[g]["rec_begin"]) + int(d[g]["n_rec"])]
                if len(want) != len(got) or any(a.tobytes() != b.tobytes() for a, b in zip(want, got)):
                    raise SystemExit(f"{name}: line {g} of kind {kd}: {len(got)} records, the definition gives {len(want)}")
            if total and not (np.diff(r["msg"].astype(np.int64)) >= 0).all():
                raise SystemExit(f"{name}: kind {kd}'s records are not in line order")
        res[name + "_kept_records"] = kept
    table = eng.profile_table(ReceiverProfiles([Profile()]))
    calls = {"dispatch_default_us": lambda: eng.dispatch_records(structs["default"], ins, n, dbufs),
             "filter_all_us": lambda: eng.filter_records(table, ins, n, pbufs),
             "dispatch_no_rule_us": lambda: eng.dispatch_records(structs["no_rule"], ins, n, dbufs)}
    for call in calls.values():
        call()
    us = {name: [] for name in calls}
    ev = lambda: t.cuda.Event(enable_timing=True)   # noqa: E731
    t.cuda.synchronize()
    for _ in range(args.iters):                           # alternating: one call of each per round
        for name, call in calls.items():
            a, b = ev(), ev()
            a.record()
            call()
            b.record()
            us[name].append((a, b))
    t.cuda.synchronize()
    for name, pairs in us.items():
        x = [a.elapsed_time(b) * 1e3 for a, b in pairs]
        res[name] = float(np.median(x))
        res[name.replace("_us", "_min_max_us")] = [float(min(x)), float(max(x))]
    res["dispatch_over_filter"] = res["dispatch_default_us"] / res["filter_all_us"]
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
