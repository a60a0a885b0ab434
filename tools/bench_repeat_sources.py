#!/usr/bin/env python
"""Time sdx_mark_repeats_by_source alone on planted launch outputs, beside sdx_mark_repeats
and sdx_mark_repeats_timed on the same chunk: N result-bearing lines, every key four times in a row within
each source (0.3 s apart, 5 s between bursts), the sources' bursts interleaved line by line (id = line % S).

  python tools/bench_repeat_sources.py --lines 250000 --sources 1,16,4096

The variants alternate inside every iteration (one HIP event pair around each call), so drift hits all of
them alike; the medians are printed as one JSON line.  Every variant's mask is checked against the serial
per-source recurrence before anything is timed.  Run it under ``rocprofv3 --kernel-trace --stats`` for the
per-kernel times."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def recurrence(kid, src, times, w):
    """w None: no window."""
    mask = np.zeros(len(kid), np.uint8)
    carry = {}
    for i, (k, s, t) in enumerate(zip(kid.tolist(), src.tolist(), times.tolist())):
        K, T = carry.get(s, (None, 0))
        if K is not None and k == K and (w is None or t - T <= w):
            mask[i] = 1
        else:
            T = t
        carry[s] = (k, T)
    return mask


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=250_000)
    ap.add_argument("--sources", default="1,16,4096")
    ap.add_argument("--window", type=float, default=2.0)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    import torch
    from pysignalduino_amd import runtime
    from pysignalduino_amd.sd_protocols import SDProtocols
    eng = SDProtocols()._ensure()
    t, n, w = torch, args.lines, int(round(args.window * 1e6))
    dev = lambda a: t.from_numpy(np.frombuffer(a.tobytes(), np.uint8).copy()).to(eng.dev)   # noqa: E731
    i = np.arange(n, dtype=np.int64)

    def chunk(S):
        """-> (the launch's sdx_json_in, key ids, source ids, times) of the chunk as S sources deliver it"""
        kid = i // (4 * S)
        src = (i % S).astype(np.int32)
        times = kid * 5_000_000 + ((i // S) % 4) * 300_000
        desc = np.zeros(n, runtime.DESC_DT)
        desc["rec_begin"], desc["n_rec"], desc["status"] = np.arange(n), 1, runtime.ST_OK
        rec = np.zeros(n, runtime.RES_DT)
        rec["payload_off"], rec["payload_len"], rec["proto"] = np.arange(n) * 12, 12, 3
        heap = np.frombuffer(b"".join(b"%012d" % k for k in kid.tolist()), np.uint8)
        out = {"desc": dev(desc), "rec": dev(rec), "heap": dev(heap), "rec_cap": n,
               "cursor": t.zeros(4, dtype=t.int32, device=eng.dev)}
        ins = [eng.json_in(runtime.KIND_MU, out, {"meta": t.zeros(32 * n, dtype=t.uint8, device=eng.dev)}, n)]
        return ins, out, kid, src, times

    variants, keep = {}, []
    # the parent's two entries on the one-source chunk
    ins, out, kid, src, times = chunk(1)
    keep.append(out)
    shift = int(times[-1] - times[0]) + w + 1      # the same chunk again, later each time: times never decrease
    tdevs = [t.from_numpy(times + k * shift).to(eng.dev) for k in range(args.iters + 2)]
    rep, scr = eng.alloc_repeat(n)
    rep_t, scr_t = eng.alloc_repeat_timed(n)
    st, st_t = eng.alloc_repeat_state(), eng.alloc_repeat_state(timed=True)
    variants["mark_repeats_us"] = (lambda k, ins=ins: eng.mark_repeats(ins, n, rep, scr, st), rep, recurrence(kid, src, times, None))
    variants["mark_repeats_timed_us"] = (lambda k, ins=ins: eng.mark_repeats_timed(ins, n, tdevs[k], w, rep_t, scr_t, st_t),
                                         rep_t, recurrence(kid, src, times, w))
    for S in [int(x) for x in args.sources.split(",")]:
        ins, out, kid, src, times = chunk(S)
        keep.append(out)
        sdev = t.from_numpy(src).to(eng.dev)
        shift = int(times[-1] - times[0]) + w + 1
        td = [t.from_numpy(times + k * shift).to(eng.dev) for k in range(args.iters + 2)]
        for timed in (False, True):
            r, sc = eng.alloc_repeat_sources(n, S)
            state = eng.alloc_repeat_state(sources=S)
            call = (lambda k, ins=ins, sdev=sdev, S=S, td=td, r=r, sc=sc, state=state, timed=timed:
                    eng.mark_repeats_by_source(ins, n, sdev, S, td[k] if timed else None, w if timed else None, r, sc, state))
            variants[f"by_source_S{S}{'_timed' if timed else ''}_us"] = (call, r, recurrence(kid, src, times, w if timed else None))
    # every mask against the recurrence: the first call of a fresh state
    for name, (call, r, exp) in variants.items():
        call(0)
        t.cuda.synchronize()
        got = r[:n].cpu().numpy()
        if not (got == exp).all():
            raise SystemExit(f"{name}: mask differs from the recurrence at {np.flatnonzero(got != exp)[:10].tolist()}")
    samples = {name: [] for name in variants}
    ev = lambda: t.cuda.Event(enable_timing=True)   # noqa: E731
    for k in range(args.iters):
        pairs = []
        for name, (call, _, _) in variants.items():
            a, b = ev(), ev()
            a.record()
            call(k + 1)
            b.record()
            pairs.append((name, a, b))
        t.cuda.synchronize()
        for name, a, b in pairs:
            samples[name].append(a.elapsed_time(b) * 1e3)
    res = {"lines": n, "window_us": w, "iters": args.iters}
    for name, v in samples.items():
        res[name] = round(float(np.median(v)), 1)
        res[name.replace("_us", "_min_us")] = round(float(np.min(v)), 1)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
