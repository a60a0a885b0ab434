"""The output-capacity overflow contract of every kernel that appends results (include/sdx.h sdx_out,
sdx_json_out): a unit (tile, block, wave or message) reserves its space with an atomicAdd on the cursor;
one that does not fit sets cursor[2] bit 0 (JSON: cursor[1]), gives its messages SDX_ST_OVF_OUT with
n_rec = 0 and stores nothing.  Every launch here writes into GUARDED buffers -- larger than the
capacities it declares, pre-filled with 0xA5 -- at capacities taken from a generous launch of the same
batch: exactly the demand (R, H), one less on either side, half on either side, and (0, 0); then again
with a heap base that is 1 and 8 bytes past a 256-byte boundary.  check_contract() is applied to every
launch.  The host loops that consume the flags (Engine.run, run_general, parse_lines_json, LineStream) end
with results equal to the reference from tight starting capacities.

Heap alignment: the tile and MC flushes have a byte-wise branch for a heap base that is not 16-byte
aligned, k_mn's writer has a byte-wise head; the two general kernels (sdx_general.hip: emit(), mc_frame()
through mc_write() / lane_hex()) store every payload byte on its own, so all routes run shifted.

Inputs and references: tests/out_capacity_inputs.py (preconditions: tests/test_out_capacity_inputs.py)."""
import ctypes

import numpy as np
import pytest

import out_capacity_inputs as I
from oracle import json_oracle as J
from oracle import lines_oracle as LO
from oracle import mn_oracle as M
from oracle import sd_oracle as O
from pysignalduino_amd import bank as B
from pysignalduino_amd import runtime, synth

pytestmark = pytest.mark.gpu

GUARD = 0xA5
GUARD_I32 = int(np.frombuffer(bytes([GUARD] * 4), "<i4")[0])
REC_GUARD, BYTE_GUARD = 256, 4096
OK, RAISED, OVF_TILE, OVF_OUT = runtime.ST_OK, runtime.ST_RAISED, runtime.ST_OVF_TILE, runtime.ST_OVF_OUT


@pytest.fixture(scope="module")
def env():
    bk = B.Bank()
    return runtime.Engine(bk, 0), bk


# ---- guarded outputs ---------------------------------------------------------------------------------
def guarded_out(eng, n, rec_cap, heap_cap, work_bytes=0, wire=False, heap_shift=0):
    """An alloc_out-shaped dict whose rec / heap / xrec tensors are larger than the capacities it declares,
    every byte 0xA5; the heap handed over starts heap_shift bytes into its allocation."""
    t, d = eng.torch, eng.dev
    full = lambda nbytes: t.full((nbytes,), GUARD, dtype=t.uint8, device=d)   # noqa: E731
    heap_full = full(heap_shift + heap_cap + BYTE_GUARD)
    out = {"desc": t.zeros(max(n, 1) * runtime.DESC_DT.itemsize, dtype=t.uint8, device=d),
           "rec": full((rec_cap + REC_GUARD) * runtime.RES_DT.itemsize),
           "heap": heap_full[heap_shift:],
           "cursor": t.zeros(4, dtype=t.int32, device=d),
           "work": t.empty(work_bytes, dtype=t.uint8, device=d) if work_bytes else None,
           "wire": t.zeros(max(n, 1), dtype=t.int64, device=d) if wire else None,
           "xrec": full((rec_cap + REC_GUARD) * 4).view(t.int32) if wire else None,
           "rec_cap": rec_cap, "heap_cap": heap_cap, "n": n, "_heap_full": heap_full, "_shift": heap_shift}
    assert (out["heap"].data_ptr() - heap_full.data_ptr()) == heap_shift and heap_full.data_ptr() % 256 == 0
    return out


def check_guards(out, untouched=False):
    """Every byte past the declared capacities (and in front of a shifted heap) is still 0xA5;
    untouched: so is every byte of rec, heap and xrec."""
    rc, hc, sh = out["rec_cap"], out["heap_cap"], out["_shift"]
    rec = out["rec"].cpu().numpy()
    heap = out["_heap_full"].cpu().numpy()
    assert (rec[(0 if untouched else rc) * runtime.RES_DT.itemsize:] == GUARD).all(), "store past rec_cap"
    assert (heap[:sh] == GUARD).all(), "store in front of heap_dev"
    assert (heap[sh + (0 if untouched else hc):] == GUARD).all(), "store past heap_cap"
    if out.get("xrec") is not None:
        xr = out["xrec"].cpu().numpy()
        assert (xr[(0 if untouched else rc):] == GUARD_I32).all(), "store past xrec's rec_cap"


# ---- the contract ------------------------------------------------------------------------------------
def check_messages(desc, rec, heap, ref, pid_of, rec_cap=None, heap_cap=None, allow=(OK, RAISED, OVF_OUT)):
    """Rules 1 and 2.  Returns (OK messages with results, SDX_ST_OVF_OUT messages, SDX_ST_OVF_TILE messages)."""
    assert len(desc) == len(ref)
    rec_cap = len(rec) if rec_cap is None else min(rec_cap, len(rec))
    heap_cap = len(heap) if heap_cap is None else heap_cap
    hb = heap.tobytes()
    st, rk, rb, nr = (desc[f].tolist() for f in ("status", "raise_kind", "rec_begin", "n_rec"))
    r_off, r_len, r_p, r_bl, r_msg = (rec[f].tolist() for f in ("payload_off", "payload_len", "proto", "bit_length", "msg"))
    ranges, n_res, n_out, n_tile = [], 0, 0, 0
    for i, e in enumerate(ref):
        s = st[i]
        assert s in allow, (i, s)
        if not isinstance(e, list):   # the reference raises: RAISED with its kind, whatever the capacity
            assert s == RAISED and rk[i] == e, (i, s, rk[i], e)
            continue
        assert s != RAISED, (i, rk[i], e)
        if s != OK:
            assert nr[i] == 0, (i, s, nr[i])
            n_out += s == OVF_OUT
            n_tile += s == OVF_TILE
            continue
        b, k = rb[i], nr[i]
        assert k == len(e), (i, k, len(e))   # never OK with fewer (or other) records than the reference
        if not k:
            continue
        assert b + k <= rec_cap, (i, b, k, rec_cap)
        ranges.append((b, b + k))
        n_res += 1
        for q, x in zip(range(b, b + k), e):
            assert r_off[q] + r_len[q] <= heap_cap, (i, q, r_off[q], r_len[q], heap_cap)
            got = (pid_of(r_p[q]), hb[r_off[q]: r_off[q] + r_len[q]], r_bl[q] if x[2] is not None else None)
            assert got == x and r_msg[q] == i, (i, q, got, x, r_msg[q])
    ranges.sort()
    assert all(a[1] <= b[0] for a, b in zip(ranges, ranges[1:])), "record ranges of two messages overlap"
    return n_res, n_out, n_tile


def wire_view(out, desc):
    """Per OK message (wire_dev word, its records' xrec entries); None for the others, whose word must be 0."""
    w = out["wire"][: len(desc)].cpu().numpy()
    xr = out["xrec"].cpu().numpy()
    view = []
    for i, d in enumerate(desc):
        if d["status"] != OK:
            assert w[i] == 0, (i, int(d["status"]), int(w[i]))
            view.append(None)
        else:
            view.append((int(w[i]), tuple(xr[int(d["rec_begin"]): int(d["rec_begin"]) + int(d["n_rec"])].tolist())))
    return view


def check_contract(eng, out, ref, pid_of, gen_wire=None, allow_tile=False, untouched=False):
    """Applied after every launch: rules 1-6 of the module docstring's contract."""
    desc, rec, heap = eng.fetch(out)
    cur = out["cursor"].cpu().numpy().astype(np.uint32)
    allow = (OK, RAISED, OVF_OUT) + ((OVF_TILE,) if allow_tile else ())
    n_res, n_out, n_tile = check_messages(desc, rec, heap, ref, pid_of, out["rec_cap"], out["heap_cap"], allow)
    assert bool(cur[2] & 1) == (n_out > 0), (int(cur[2]), n_out)
    # the cursors count what THIS launch's units asked for, placed or not: everything fits when both
    # totals are within the capacities, and otherwise the reserver that ends last does not
    demand_fits = int(cur[0]) <= out["rec_cap"] and int(cur[1]) <= out["heap_cap"]
    assert (n_out == 0) == demand_fits, (n_out, cur[:2].tolist(), out["rec_cap"], out["heap_cap"])
    if not allow_tile:
        assert not cur[2] & 2, int(cur[2])
    check_guards(out, untouched)
    if out.get("wire") is not None:
        view = wire_view(out, desc)
        if gen_wire is not None:
            bad = [i for i, (a, b) in enumerate(zip(view, gen_wire)) if a is not None and a != b]
            assert not bad, ("wire / xrec differ from the generous launch", bad[:5])
    return n_res, n_out, cur


# ---- routes -------------------------------------------------------------------------------------------
class Route:
    """One kernel / route over one batch: launch(out), its reference, how a record's proto maps to the
    reference's protocol, and the product path (run(rec_cap, heap_cap) -> host desc, rec, heap)."""

    def __init__(self, n, ref, pid_of, launch, run=None, work=0, wire=False):
        self.n, self.ref, self.pid_of, self.launch, self.run, self.work, self.wire = n, ref, pid_of, launch, run, work, wire
        self.gen = None   # the generous launch: (R, H, its wire view)
        self.heap_varies, self.last_heap = False, 0


def _pids(lst):
    return lambda p: str(lst[p])


def _pulse_route(eng, bk, kind, pb, ref, **kw):
    k = runtime.KIND_MU if kind == "MU" else runtime.KIND_MS
    bd = eng.to_device_pulses(pb)
    mrec = kw.pop("mrec", None)

    def launch(out):
        keep = eng.use_mrec
        if mrec is not None:
            eng.use_mrec = mrec
        try:
            eng.launch_pulses(k, bd, out, **kw)
        finally:
            eng.use_mrec = keep
    return Route(pb.n, ref, _pids(bk.mu_pids if kind == "MU" else bk.ms_pids), launch,
                 run=lambda rc, hc: eng.run(k, bd, rec_cap=rc, heap_cap=hc),
                 work=0 if kw.get("long_variant") else eng.pulses_work_bytes(pb.n), wire=True)


def _general_route(eng, bk, kind):
    msgs, gen, ref = I.general_pulses(kind)
    k = runtime.KIND_MU if kind == "MU" else runtime.KIND_MS
    gd = eng.to_device_general(gen.arrays())
    n, lens = gd["n"], np.asarray(gd["lengths"])
    max_len = int(lens.max(initial=0))
    t = eng.torch
    wb = int(eng.lib.sdx_general_work_bytes(eng.handle, k, int(gd["total"]), n, max_len, 0))
    work = t.empty(max(wb, 1), dtype=t.uint8, device=eng.dev)
    sel = t.from_numpy(np.argsort(-lens, kind="stable").astype(np.int32)).to(eng.dev)
    p = runtime._ptr

    def launch(out):
        o = eng._out_struct(out)
        o.work_dev, o.work_cap = p(work), int(work.numel())
        b = runtime.SdxGeneralBatch(p(gd["data"]), p(gd["offsets"]), p(gd["npat"]), p(gd["pat_ids"]), p(gd["pat_val"]),
                                    p(gd["cp_slot"]), p(gd["ms_ok"]), p(sel), n, n, None, 0, max_len, 0)
        runtime._check(eng.lib, eng.lib.sdx_demod_pulses_general(eng.handle, k, ctypes.byref(b), ctypes.byref(o),
                                                                 eng.stream_ptr()))
    return Route(n, ref, _pids(bk.mu_pids if kind == "MU" else bk.ms_pids), launch,
                 run=lambda rc, hc: eng.run_general(k, gd, rec_cap=rc, heap_cap=hc))


def _mn_route(eng, bk, mode):
    frames, parser, method = I.mn_both()
    bd = eng.to_device_mn([f[0] for f in frames])
    if mode == "parser":
        elig = sum(1 << k for k, rf in enumerate(bk.mn_rfmode) if rf)   # parser/mn.py:83-93 without an rfmode
        assert bin(elig).count("1") >= 3
        kw, ref, pid_of = {"elig": elig}, parser, _pids(bk.mn_pids)
        run = lambda rc, hc: eng.run(runtime.KIND_MN, bd, rec_cap=rc, heap_cap=hc, mn_elig=elig)   # noqa: E731
    else:
        k = B.MN_METHODS[I.MN_METHOD]
        kw, ref, pid_of = {"method": k}, method, (lambda p: p)
        run = lambda rc, hc: eng.run(runtime.KIND_MN, bd, rec_cap=rc, heap_cap=hc, mn_method=k)    # noqa: E731
    return Route(len(frames), ref, pid_of, lambda out: eng.launch_mn(bd, out, **kw), run=run)


def _mc_route(eng, bk, general):
    frames, mb, ref = I.mc_general() if general else I.mc_both()
    bd = eng.to_device_mc(mb)
    if general:
        sel = eng.torch.arange(mb.n, dtype=eng.torch.int32, device=eng.dev)
        launch = lambda out: eng.launch_mc_general(bd, out, sel, bd["max_hex"])   # noqa: E731
    else:
        launch = lambda out: eng.launch_mc(bd, out)   # noqa: E731
    return Route(mb.n, ref, _pids(bk.mc_pids), launch, wire=not general,
                 run=lambda rc, hc: eng.run(runtime.KIND_MC, bd, rec_cap=rc, heap_cap=hc))


ROUTES = {
    "mu_short": lambda e, b: _pulse_route(e, b, "MU", *I.mu_short(), group=False),
    "mu_grouped": lambda e, b: _pulse_route(e, b, "MU", *I.mu_grouped(), mrec=False),
    "mu_grouped_mrec": lambda e, b: _pulse_route(e, b, "MU", *I.mu_grouped(), mrec=True),
    "mu_long": lambda e, b: _pulse_route(e, b, "MU", *I.mu_long(), long_variant=True),
    "ms_tile128": lambda e, b: _pulse_route(e, b, "MS", *I.ms_classes(), group=False),
    "ms_tile64": lambda e, b: _pulse_route(e, b, "MS", *I.ms_classes(), group=False),
    "mc": lambda e, b: _mc_route(e, b, False),
    "mc_general": lambda e, b: _mc_route(e, b, True),
    "general_mu": lambda e, b: _general_route(e, b, "MU"),
    "general_ms": lambda e, b: _general_route(e, b, "MS"),
    "mn_parser": lambda e, b: _mn_route(e, b, "parser"),
    "mn_method": lambda e, b: _mn_route(e, b, "method"),
}
_routes = {}


def generous_caps(n):
    return 64 * n + 4096, 4096 * n + 65536


@pytest.fixture
def route(name, env, monkeypatch):
    """The route named by the test's `name` parameter, with the demand (R, H) of a generous launch."""
    if name.startswith("ms_tile"):
        monkeypatch.setenv("SDX_MS_TILE", name[len("ms_tile"):])
    eng, bk = env
    if name not in _routes:
        r = _routes[name] = ROUTES[name](eng, bk)
        rc, hc = generous_caps(r.n)
        cursors = []
        for _ in range(2):   # twice: a deterministic batch order makes the totals deterministic
            out = guarded_out(eng, r.n, rc, hc, r.work, r.wire)
            r.launch(out)
            n_res, n_out, cur = check_contract(eng, out, r.ref, r.pid_of)
            assert n_out == 0 and n_res == sum(1 for e in r.ref if isinstance(e, list) and e)
            cursors.append((int(cur[0]), int(cur[1]), int(cur[3])))
        # a tile that spills splits its payloads between LDS and its spill region by the order in which
        # its waves stage them, and reserves both parts rounded up: the heap total of a launch with
        # spilling tiles varies from run to run (seen: 413440 and 414272 bytes for mu_grouped), the
        # record total does not.  Every other launch's totals are deterministic.
        r.heap_varies = cursors[0][2] > 0
        assert cursors[0][0] == cursors[1][0] and (r.heap_varies or cursors[0][1] == cursors[1][1]), cursors
        R, H = cursors[0][:2]
        assert R == sum(len(e) for e in r.ref if isinstance(e, list)) and H >= I.demand(r.ref)[1].sum()
        r.gen = (R, H, wire_view(out, eng.fetch(out)[0]) if r.wire else None)
    return _routes[name]


def launch_at(eng, r, rec_cap, heap_cap, shift=0, untouched=False):
    out = guarded_out(eng, r.n, rec_cap, heap_cap, r.work, r.wire, shift)
    r.launch(out)
    n_res, n_out, cur = check_contract(eng, out, r.ref, r.pid_of, gen_wire=r.gen[2], untouched=untouched)
    r.last_heap = int(cur[1])   # what this launch's units asked for
    return n_res, n_out


CASES = ["exact", "rec-1", "heap-1", "rec/2", "heap/2", "zero"]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("name", list(ROUTES))
def test_capacity_boundaries(env, route, name, case):
    eng, _ = env
    R, H, _ = route.gen
    with_results = sum(1 for e in route.ref if isinstance(e, list) and e)
    # (a launch with spilling tiles may ask for a few bytes more or less heap than the generous one did,
    # see the route fixture: the heap boundary is then judged against this launch's own total, which
    # check_contract does for every launch)
    if case == "exact":       # exactly the demand: no overflow, everything equal to the reference
        got = launch_at(eng, route, R, H)
        assert got == (with_results, 0) or (route.heap_varies and route.last_heap > H), got
    elif case in ("rec-1", "heap-1"):   # the reservations sum to more than the capacity: the last reserver overflows
        n_res, n_out = launch_at(eng, route, R - (case == "rec-1"), H - (case == "heap-1"))
        assert n_out >= 1 or (case == "heap-1" and route.heap_varies and route.last_heap < H)
    elif case in ("rec/2", "heap/2"):   # the first reserver still fits (test_out_capacity_inputs): some of each
        n_res, n_out = launch_at(eng, route, R // 2 if case == "rec/2" else R, H // 2 if case == "heap/2" else H)
        assert n_out >= 1 and n_res >= 1, (n_res, n_out)
    else:                     # nothing fits: every result-bearing message overflows, nothing is stored
        n_res, n_out = launch_at(eng, route, 0, 0, untouched=True)
        assert n_res == 0 and n_out >= with_results


@pytest.mark.parametrize("shift", [1, 8])
@pytest.mark.parametrize("name", ["mu_short", "ms_tile128", "ms_tile64", "mc", "mn_parser", "mn_method", "mc_general",
                                  "general_mu", "general_ms"])
def test_unaligned_heap_base(env, route, name, shift):
    """heap_dev 1 and 8 bytes past a 256-byte boundary: the same results and intact guards (in front of
    the heap too), at the exact demand and at half the records."""
    eng, _ = env
    R, H, _ = route.gen
    with_results = sum(1 for e in route.ref if isinstance(e, list) and e)
    assert launch_at(eng, route, R, H, shift) == (with_results, 0)
    n_res, n_out = launch_at(eng, route, R // 2, H, shift)
    assert n_out >= 1 and n_res >= 1


@pytest.mark.parametrize("name", list(ROUTES))
def test_product_path_from_half_the_capacity(env, route, name):
    """Engine.run / run_general started with half the demand: the re-runs end with every message equal to
    the reference and no overflow status left."""
    R, H, _ = route.gen
    desc, rec, heap = route.run(max(1, R // 2), max(1, H // 2))
    n_res, n_out, n_tile = check_messages(desc, rec, heap, route.ref, route.pid_of, allow=(OK, RAISED))
    assert n_res == sum(1 for e in route.ref if isinstance(e, list) and e)


# ---- the fused step -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def step_parts(env):
    """MU, MS and MC batches of <= 600 messages, their separate generous launches (canonical form, wire
    views) and demands."""
    from pysignalduino_amd import dist
    eng, bk = env
    mu, mu_ref = I.mu_short()
    ms, ms_ref = I.ms_classes()
    _, mc, mc_ref = I.mc_step()
    bds = {"MU": eng.to_device_pulses(mu), "MS": eng.to_device_pulses(ms), "MC": eng.to_device_mc(mc)}
    assert 0 < bds["MC"]["max_hex"] <= runtime.MC_SHORT_HEX   # MC runs inside the fused kernel
    parts = {}
    for k, ref, pids in (("MU", mu_ref, bk.mu_pids), ("MS", ms_ref, bk.ms_pids), ("MC", mc_ref, bk.mc_pids)):
        n = bds[k]["n"]
        out = guarded_out(eng, n, *generous_caps(n), eng.pulses_work_bytes(n) if k != "MC" else 0, True)
        if k == "MC":
            eng.launch_mc(bds[k], out)
        else:
            eng.launch_pulses(runtime.KIND_MU if k == "MU" else runtime.KIND_MS, bds[k], out, group=False)
        n_res, n_out, cur = check_contract(eng, out, ref, _pids(pids))
        assert n_out == 0
        f = eng.fetch(out)
        parts[k] = {"bd": bds[k], "n": n, "ref": ref, "pid_of": _pids(pids), "R": int(cur[0]), "H": int(cur[1]),
                    "canon": [x.tobytes() for x in dist.canonical(*f)], "wire": wire_view(out, f[0])}
    return parts


@pytest.mark.parametrize("tight", ["none", "MU", "MS", "MC", "all"])
def test_fused_step_parts_overflow_on_their_own(env, step_parts, tight):
    """sdx_demod_step with each part in its own guarded out: a tight part (half its records) overflows by
    the contract and changes no byte of the other parts' canonical outputs, which equal the separate
    launches'."""
    from pysignalduino_amd import dist
    eng, _ = env
    outs = {}
    for k, p in step_parts.items():
        rc, hc = (p["R"] // 2, p["H"]) if tight in (k, "all") else generous_caps(p["n"])
        outs[k] = guarded_out(eng, p["n"], rc, hc, eng.pulses_work_bytes(p["n"]) if k != "MC" else 0, True)
    eng.launch_step(mu=(step_parts["MU"]["bd"], outs["MU"], None, None), ms=(step_parts["MS"]["bd"], outs["MS"], None, None),
                    mc=(step_parts["MC"]["bd"], outs["MC"], None))
    for k, p in step_parts.items():
        n_res, n_out, _ = check_contract(eng, outs[k], p["ref"], p["pid_of"], gen_wire=p["wire"])
        if tight in (k, "all"):
            assert n_out >= 1 and n_res >= 1, (k, n_res, n_out)
        else:
            assert n_out == 0
            assert [x.tobytes() for x in dist.canonical(*eng.fetch(outs[k]))] == p["canon"], k


# ---- the serialiser -----------------------------------------------------------------------------------
def _line_inputs(kind):
    """(lines, per line the reference's texts, one per result in order) of <= 512 lines of one kind."""
    ob = O.OracleBank()
    if kind in ("MU", "MS"):
        pb = (I.mu_short() if kind == "MU" else I.ms_classes())[0]
        lines = [synth.frame(synth.pulse_payload(pb, i)) for i in range(256 if kind == "MU" else 300)]
        texts = []
        for ln in lines:
            r = LO.parse_line(ln)
            assert r["status"] == LO.OK
            try:
                res = O.demod(ob, dict(r["msg"]), kind)
            except Exception:  # noqa: BLE001  (the parsers catch a demodulator exception: no result)
                res = []
            texts.append([J.message_to_json(x["protocol_id"], x["payload"], x["meta"]) for x in res])
    elif kind == "MC":
        frames, mb, _ = I.mc_both()
        rows = list(range(384)) + list(range(1024, 1152))   # both launches of sdx_demod_mc
        lines = [synth.frame(synth.mc_payload(mb, i)) for i in rows]
        texts = []
        for i in rows:
            h, c, L, _, _ = frames[i]
            try:
                res = O.demod_mc_fixed(ob, h, c, L, "MC", None)
            except Exception:  # noqa: BLE001
                res = []
            texts.append([J.message_to_json(x["protocol_id"], x["payload"],
                                            {"protocol_id": x["protocol_id"], "rssi": None, "freq_afc": None}) for x in res])
    else:
        frames = I.mn_both()[0][:512]
        lines = [synth.frame(synth.mn_payload(*f)) for f in frames]
        texts = []
        for ln in lines:
            r = LO.parse_line(ln)
            res = M.mn_parse(ob, r["data"].decode(), M.rssi_of(r["R"]), M.afc_of(r["F"]), None) if r["status"] == LO.OK else []
            texts.append([J.message_to_json(*x) for x in res])
    return lines, texts


@pytest.fixture(scope="module")
def json_launches(env):
    return line_launches(env)


def line_launches(env):
    """Per kind: the parsed line batch and a generous demodulation launch of its lines (as
    parse_lines_json makes them), with the reference's texts."""
    from pysignalduino_amd.frontend import LineBatch, pack_lines
    eng, bk = env
    cache = {}

    def get(kind):
        if kind in cache:
            return cache[kind]
        lines, texts = _line_inputs(kind)
        n = len(lines)
        data, offsets, bad = pack_lines(lines)
        assert not bad
        lb = LineBatch(eng, data, offsets)
        lb.launch()
        sels, cnt = lb.selections()
        k = {"MU": runtime.KIND_MU, "MS": runtime.KIND_MS, "MC": runtime.KIND_MC, "MN": runtime.KIND_MN}[kind]
        out = eng.alloc_out(n, *generous_caps(n), eng.pulses_work_bytes(n) if kind in ("MU", "MS") else 0)
        if kind == "MN":
            eng.launch_mn(lb.mn_batch(), out, elig=sum(1 << j for j, rf in enumerate(bk.mn_rfmode) if rf),
                          sel=sels[runtime.SEL_MN])
        elif kind == "MC":
            sel, m = lb.mc_all(cnt)
            assert int(cnt[runtime.SEL_MC]) >= 100 and int(cnt[runtime.SEL_MC_LONG]) >= 100   # both launches
            eng.launch_mc(lb.mc_batch(), out, sel=sel)
        else:
            short = sels[runtime.SEL_MU_SHORT if kind == "MU" else runtime.SEL_MS_SHORT]
            assert short.numel() > n // 2
            eng.launch_pulses(k, lb.pulse_batch(), out, sel=short)
        desc, rec, _ = eng.fetch(out)
        assert int(out["cursor"][2].item()) == 0
        assert [int(d["n_rec"]) if d["status"] == OK else 0 for d in desc] == [len(x) for x in texts]
        cache[kind] = (k, lb, out, desc, rec, texts)
        return cache[kind]
    return get


def guarded_json(eng, items, cap):
    t, d = eng.torch, eng.dev
    return {"json": t.full((cap + BYTE_GUARD,), GUARD, dtype=t.uint8, device=d),
            "off": t.full((max(items, 1),), GUARD_I32, dtype=t.int32, device=d),
            "len": t.full((max(items, 1),), GUARD_I32, dtype=t.int32, device=d),
            "cursor": t.zeros(2, dtype=t.int32, device=d), "cap": cap, "items": items}


def run_json(eng, launch, mode, skip, cap, expected):
    """One serialiser launch into guarded buffers; `expected`: per item its text or None.  Checks the
    texts, their placement, the overflow flag and the guards; returns (cursor[0], missing texts)."""
    k, lb, out, desc, rec, _ = launch
    n = lb.n
    lo = {"meta": lb.meta, "pat_val": lb.pat_val, "cp_slot": lb.cp_slot}
    jo = guarded_json(eng, len(expected), cap)
    out = dict(out, rec_cap=len(expected)) if mode == 0 else out   # rec_max: the record-indexed outputs' size
    eng.launch_json(k, out, lo, n, jo, first_only=mode, skip=skip)
    eng.torch.cuda.current_stream(eng.dev).synchronize()
    cur = jo["cursor"].cpu().numpy().astype(np.uint32)
    off, ln = jo["off"].cpu().numpy(), jo["len"].cpu().numpy()
    blob = jo["json"].cpu().numpy()
    assert (blob[cap:] == GUARD).all(), "store past json_cap"
    missing = 0
    for i, e in enumerate(expected):
        if e is None:
            if mode == 2:   # sparse: a line without a text is not written at all
                assert off[i] == GUARD_I32 and ln[i] == GUARD_I32, (i, int(off[i]), int(ln[i]))
            else:
                assert ln[i] == 0, (i, int(ln[i]))
            continue
        if ln[i] == 0:
            missing += 1
            continue
        assert 0 <= off[i] and off[i] + ln[i] <= cap, (i, int(off[i]), int(ln[i]), cap)
        assert blob[off[i]: off[i] + ln[i]].tobytes().decode("ascii") == e, i
    assert bool(cur[1]) == (missing > 0), (int(cur[1]), missing)
    return int(cur[0]), missing


@pytest.mark.parametrize("mode", [1, 2, 0])
@pytest.mark.parametrize("skipped", [False, True])
@pytest.mark.parametrize("kind", ["MU", "MS", "MC", "MN"])
def test_json_capacity_boundaries(env, json_launches, kind, skipped, mode):
    eng, _ = env
    launch = json_launches(kind)
    k, lb, out, desc, rec, texts = launch
    n = lb.n
    mask = np.zeros(n, np.uint8)
    if skipped:
        mask[::3] = 1   # sdx_serialize_json_skip: every third line gets no text
    skip = eng.torch.from_numpy(mask).to(eng.dev) if skipped else None
    if mode == 0:   # one text per record, indexed like rec_dev
        owner = {}
        for i, d in enumerate(desc):
            if d["status"] == OK:
                for j in range(int(d["n_rec"])):
                    owner[int(d["rec_begin"]) + j] = (i, j)
        assert sorted(owner) == list(range(len(rec)))
        expected = [None if mask[owner[g][0]] else texts[owner[g][0]][owner[g][1]] for g in range(len(rec))]
    else:
        expected = [t[0] if t and not mask[i] else None for i, t in enumerate(texts)]
    total = sum(len(e) for e in expected if e is not None)
    assert total > 0
    Jn, missing = run_json(eng, launch, mode, skip, total + 65536, expected)
    assert Jn == total and missing == 0
    assert run_json(eng, launch, mode, skip, Jn, expected) == (Jn, 0)            # exactly the demand
    assert run_json(eng, launch, mode, skip, Jn - 1, expected)[1] >= 1           # the last reserver overflows
    half = run_json(eng, launch, mode, skip, Jn // 2, expected)[1]
    assert 1 <= half < sum(e is not None for e in expected)                      # the first reserver fits
    assert run_json(eng, launch, mode, skip, 0, expected)[1] == sum(e is not None for e in expected)


# ---- host loops that consume the flags ------------------------------------------------------------------
@pytest.fixture(scope="module")
def parser():
    from pysignalduino_amd.frontend import SignalParser
    from pysignalduino_amd.sd_protocols import SDProtocols
    return SignalParser(SDProtocols())


@pytest.fixture(scope="module")
def heavy_cases():
    cache = {}

    def get(min_rec):
        if min_rec not in cache:
            lines = I.heavy(min_rec)[0]
            cache[min_rec] = (lines, I.heavy_texts(lines))
        return cache[min_rec]
    return get


def _collapsed(texts):
    """The texts with the repeats of the previous result-bearing line's (protocol, payload) dropped."""
    import json
    out, last = [], None
    for t in texts:
        if t is None:
            out.append(None)
            continue
        d = json.loads(t)
        key = (d["protocol_id"], d["payload"])
        out.append(None if key == last else t)
        last = key
    return out


def _counting(monkeypatch, eng):
    """eng.alloc_out as a counting pass-through: the (rec_cap, workspace bytes) of every call."""
    calls, real = [], eng.alloc_out

    def alloc_out(n, rec_cap, heap_cap, work_bytes=0, wire=False):
        calls.append((rec_cap, work_bytes))
        return real(n, rec_cap, heap_cap, work_bytes, wire)
    monkeypatch.setattr(eng, "alloc_out", alloc_out)
    return calls


@pytest.mark.parametrize("collapse", [False, True])
@pytest.mark.parametrize("min_rec", [16, 8])
def test_parse_lines_json_retries_past_a_capacity_overflow(parser, heavy_cases, monkeypatch, min_rec, collapse):
    """Lines that all carry >= min_rec MU results ask for more than the first attempt's 8k + 1024 records;
    the call ends with the reference's texts.  min_rec 16: 14 tiles, every spilling tile finds a region,
    the launch overflows its outputs (cursor[2] = 1) and is repeated with four times the capacities.
    min_rec 8: more tiles spill than the workspace has regions; those tiles report SDX_ST_OVF_TILE and
    reserve nothing, so the others fit and cursor[2] is 2 -- growing the capacities cannot cure that
    (before the fix: four attempts, then RuntimeError "capacity overflow persists"); those messages re-run
    on the long variant into an overlay."""
    lines, exp = heavy_cases(min_rec)
    eng = parser.protocols._ensure()
    calls = _counting(monkeypatch, eng)
    got = parser.parse_lines_json(lines, collapse_repeats=collapse)
    want = _collapsed(exp) if collapse else exp
    bad = [i for i, (g, e) in enumerate(zip(got, want)) if g != e]
    assert not bad, (len(bad), bad[:5], got[bad[0]], want[bad[0]])
    assert sum(e is not None for e in exp) == len(lines)
    # the first attempt did overflow: more than one MU allocation (every line is an MU line)
    assert len(calls) > 1 and calls[0][0] == 8 * len(lines) + 1024 and calls[0][1] > 0, calls
    if min_rec == 16:
        assert calls[1] == (4 * calls[0][0], calls[0][1]), calls       # the same launch, grown
    else:
        assert calls[1][1] == 0 and len(calls) == 2, calls             # the overlay of the long variant's re-run


@pytest.mark.parametrize("min_rec", [16, 8])
def test_line_stream_hands_an_overflowed_chunk_to_the_batch_api(parser, heavy_cases, min_rec):
    """One chunk of all the heavy lines: the slot's MU capacity (8 C + 4096 records) is below their
    demand, so the chunk's MU lines go through the batch API (r.host) and come back with the reference's
    texts."""
    lines, exp = heavy_cases(min_rec)
    ls = parser.stream(chunk_lines=len(lines), chunk_bytes=sum(len(ln) for ln in lines))
    ls.submit(lines)
    res = ls.drain()
    assert len(res) == 1 and res[0].n == len(lines)
    r = res[0]
    assert set(r.host) == set(range(len(lines)))   # every line is an MU line: all of them were redone
    got = r.texts()
    bad = [i for i, (g, e) in enumerate(zip(got, exp)) if g != e]
    assert not bad, (len(bad), bad[:5])
