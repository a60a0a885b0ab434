#!/usr/bin/env python
"""Time the repeat passes alone on planted launch outputs: sdx_mark_repeats and
sdx_mark_repeats_timed over one chunk of N result-bearing lines, HIP events around ITERS calls each.

  python tools/bench_repeat_pass.py --lines 250000 --shape bursts     # every key 4 times, 5 s between bursts
  python tools/bench_repeat_pass.py --lines 250000 --shape segment    # ONE key, every gap W / 3: the chunk
                                                                      # is one segment, every 4th line published

Run it under ``rocprofv3 --kernel-trace --stats`` for the per-kernel times.  Prints one JSON line; the
masks are checked against the serial recurrence before anything is timed."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def recurrence(kid, times, w):
    mask = np.zeros(len(kid), np.uint8)
    K, T = None, 0
    for i, (k, t) in enumerate(zip(kid.tolist(), times.tolist())):
        if K is not None and k == K and t - T <= w:
            mask[i] = 1
        else:
            T = t
        K = k
    return mask


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=250_000)
    ap.add_argument("--shape", default="bursts", choices=("bursts", "segment"))
    ap.add_argument("--window", type=float, default=2.0)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    import torch
    from pysignalduino_amd import runtime
    from pysignalduino_amd.sd_protocols import SDProtocols
    eng = SDProtocols()._ensure()
    t, n, w = torch, args.lines, int(round(args.window * 1e6))
    if args.shape == "bursts":
        kid = np.arange(n) // 4
        times = (np.arange(n) // 4) * 5_000_000 + (np.arange(n) % 4) * 300_000
    else:
        kid = np.zeros(n, np.int64)
        times = np.arange(n) * (w // 3)
    times = times.astype(np.int64)
    # one MU launch: line i's record i, a 12-byte payload that spells its key
    desc = np.zeros(n, runtime.DESC_DT)
    desc["rec_begin"], desc["n_rec"], desc["status"] = np.arange(n), 1, runtime.ST_OK
    rec = np.zeros(n, runtime.RES_DT)
    rec["payload_off"], rec["payload_len"], rec["proto"] = np.arange(n) * 12, 12, 3
    heap = np.frombuffer(b"".join(b"%012d" % k for k in kid.tolist()), np.uint8)
    dev = lambda a: t.from_numpy(np.frombuffer(a.tobytes(), np.uint8).copy()).to(eng.dev)   # noqa: E731
    out = {"desc": dev(desc), "rec": dev(rec), "heap": dev(heap), "rec_cap": n,
           "cursor": t.zeros(4, dtype=t.int32, device=eng.dev)}
    ins = [eng.json_in(runtime.KIND_MU, out, {"meta": t.zeros(32 * n, dtype=t.uint8, device=eng.dev)}, n)]
    # the timed calls of one stream: the same chunk again, later each time (times never decrease)
    shift = int(times[-1] - times[0]) + w + 1
    tdevs = [t.from_numpy(times + i * shift).to(eng.dev) for i in range(args.iters + 1)]
    rep, scr = eng.alloc_repeat(n)
    rep_t, scr_t = eng.alloc_repeat_timed(n)

    def plain():
        st = eng.alloc_repeat_state()
        return lambda i: eng.mark_repeats(ins, n, rep, scr, st)

    def timed():
        st = eng.alloc_repeat_state(timed=True)
        return lambda i: eng.mark_repeats_timed(ins, n, tdevs[i], w, rep_t, scr_t, st)

    timed()(0)
    t.cuda.synchronize()
    got = rep_t[:n].cpu().numpy()
    exp = recurrence(kid, times, w)
    if not (got == exp).all():
        raise SystemExit(f"mask differs from the recurrence at {np.flatnonzero(got != exp)[:10].tolist()}")
    res = {"lines": n, "shape": args.shape, "window_us": w, "published": int((exp == 0).sum()), "iters": args.iters}
    for name, make in (("mark_repeats_us", plain), ("mark_repeats_timed_us", timed)):
        call = make()
        call(0)     # the first call starts the stream; the timed ones continue it from the carried state
        e = [t.cuda.Event(enable_timing=True) for _ in range(args.iters + 1)]
        t.cuda.synchronize()
        e[0].record()
        for i in range(args.iters):
            call(i + 1)
            e[i + 1].record()
        t.cuda.synchronize()
        res[name] = float(np.median([a.elapsed_time(b) * 1e3 for a, b in zip(e, e[1:])]))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
