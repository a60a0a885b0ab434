"""The json_all stream end to end: the recorded lines of tests/golden/lines_golden.json.gz through
``sp.stream(output="json_all")`` in chunks of 1000 and of 257 lines.

Every line's list must equal both the one-shot call's (parse_lines_json_all with the same arguments) and the
reference-recorded "e2e" lists pushed through DispatchRules.reduce and oracle/json_oracle.message_to_json, with a
ContractError exactly where the plain parse_lines call has one (test_dispatch_e2e.py's ``setup`` and ``compare``).
So that the host fallback cannot hide a failure: no chunk reports an overflow, the batch API resolves at most 5 % of
the lines, and with the default rules the device-resolved lines alone show at least 100 changed lists."""
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import sd_oracle as O

from test_dispatch_e2e import BLACK, KINDS, compare, setup, sp, texts_of  # noqa: F401  (fixtures)
from test_profiles_host import restate_filter

pytestmark = pytest.mark.gpu


def run_stream(sp, lines, chunk_lines, times=None, sources=None, output="json_all", **kw):   # noqa: F811
    """The lines through a stream in chunks of ``chunk_lines``, polls in between -> per line its result, the chunk
    results."""
    chunks = [slice(a, min(a + chunk_lines, len(lines))) for a in range(0, len(lines), chunk_lines)]
    nbytes = max(sum(len(x) for x in lines[c]) for c in chunks) + 4096
    ls = sp.stream(chunk_lines=chunk_lines, chunk_bytes=nbytes, output=output, lag=3, **kw)
    got = []
    for j, c in enumerate(chunks):
        skw = {}
        if times is not None:
            skw["times"] = times[c]
        if sources is not None:
            skw["sources"] = sources[c]
        assert ls.submit(lines[c], **skw) == j
        if j % 2:
            got += [r.detach() for r in ls.poll()]
    got += [r.detach() for r in ls.drain()]
    assert [r.id for r in got] == list(range(len(chunks)))
    return [x for r in got for x in (r.texts_all() if output == "json_all" else r.texts())], got


def fallback_stays_small(s, res):
    """No overflow anywhere, and the batch API resolved at most 5 % of the lines (test_stream.py's bound)."""
    assert not any(r.overflow for r in res)
    assert sum(len(r.host) for r in res) <= 0.05 * len(s.lines)
    for r in res:
        first = r.first.astype(np.int64)
        assert first[0] == 0 and (np.diff(first) >= 0).all() and first[-1] == len(r.off) == len(r.len)


def on_host(res):
    return {a + i for a, r in zip(np.cumsum([0] + [r.n for r in res[:-1]]).tolist(), res) for i in r.host}


@pytest.fixture(scope="module")
def rule_sets(setup, sp):   # noqa: F811
    """name -> (the stream's ``rules``, the one-shot call's lists, the reference's lists reduced on the host)."""
    from pysignalduino_amd.dispatch import DispatchRules
    s = setup
    cap1 = DispatchRules(max_repeat=1, keep_equal=())
    red1 = [cap1.reduce(s.bank, e[0][3][1], e) if e else [] for e in s.e2e]
    return {"none": (None, sp.parse_lines_json_all(s.lines), [texts_of(e) for e in s.e2e]),
            "default": (True, sp.parse_lines_json_all(s.lines, dispatch=True), [texts_of(e) for e in s.red]),
            "cap1": (cap1, sp.parse_lines_json_all(s.lines, dispatch=cap1), [texts_of(e) for e in red1])}


@pytest.mark.parametrize("chunk_lines", [1000, 257])
@pytest.mark.parametrize("name", ["none", "default", "cap1"])
def test_every_message_of_every_line(setup, sp, rule_sets, name, chunk_lines):   # noqa: F811
    s = setup
    rules, one_shot, exp = rule_sets[name]
    got, res = run_stream(sp, s.lines, chunk_lines, **({} if rules is None else {"rules": rules}))
    compare(s, got, exp)
    compare(s, got, [[] if c else x for x, c in zip(one_shot, s.ce)])
    fallback_stays_small(s, res)
    if name != "cap1":      # what a json stream loses: the lines that publish two or more messages
        assert sum(len(x) >= 2 for x, c in zip(got, s.ce) if not c) > (300 if name == "none" else 250)
    if name == "default":   # the rules act on the lines the DEVICE resolves, too
        host = on_host(res)
        every = rule_sets["none"][2]
        assert sum(got[i] != every[i] for i in range(len(got)) if i not in host and not s.ce[i]) >= 100


def test_first_text_is_the_json_streams_text(setup, sp, rule_sets):   # noqa: F811
    s = setup
    one, _ = run_stream(sp, s.lines, 1000, output="json")
    assert [isinstance(x, s.ContractError) for x in one] == s.ce
    for name in ("none", "default"):
        got, _ = run_stream(sp, s.lines, 1000, **({} if name == "none" else {"rules": True}))
        assert [x for x, c in zip(one, s.ce) if not c] == [(x[0] if x else None) for x, c in zip(got, s.ce) if not c]


def test_profiles_in_front_of_the_rules(setup, sp):   # noqa: F811
    """test_dispatch_e2e.py's four receivers (line g % 4) with four profiles."""
    from pysignalduino_amd.profiles import Profile, ReceiverProfiles
    s = setup
    P = O.OracleBank().p
    ids = sorted({m[0] for e in s.e2e for m in e}, key=float)
    kws = [dict(whitelist=ids[::2]), dict(blacklist=BLACK), dict(skip_development=True), dict()]
    src = np.arange(len(s.lines), dtype=np.int32) % 4
    filt = [restate_filter(P, KINDS.index(e[0][3][1]), e, **kws[int(k)]) if e else [] for e, k in zip(s.e2e, src)]
    exp = [s.rules.reduce(s.bank, f[0][3][1], f) if f else [] for f in filt]
    rp = ReceiverProfiles([Profile(**kw) for kw in kws], [0, 1, 2, 3])
    got, res = run_stream(sp, s.lines, 257, sources=src, profiles=rp, rules=True)
    compare(s, got, [texts_of(x) for x in exp])
    one_shot = sp.parse_lines_json_all(s.lines, dispatch=True, profiles=rp, sources=src)
    compare(s, got, [[] if c else x for x, c in zip(one_shot, s.ce)])
    fallback_stays_small(s, res)
    got, res = run_stream(sp, s.lines, 1000, sources=src, profiles=rp)                 # the profiles alone
    compare(s, got, [texts_of(x) for x in filt])


def doubled(s, k=2):
    """Every decoding line k times in a row -> (the original line of every line, the lines, their reduced lists as objects)."""
    idx = [i for i in range(len(s.lines)) for _ in range(k if s.e2e[i] else 1)]
    objs = [[] if s.ce[i] else [SimpleNamespace(protocol_id=m[0], payload=m[1], raw=SimpleNamespace(message_type=m[3][1]))
                               for m in s.red[i]] for i in idx]
    return idx, [s.lines[i] for i in idx], objs


def test_collapse_repeats_with_pairs_across_chunk_ends(setup, sp):   # noqa: F811
    """Every decoding line twice, 257 lines a chunk: pairs straddle chunk ends, the run is carried on the device.  The
    mask is repeats.collapse_objects on the reduced lists; a repeat line gives []."""
    from pysignalduino_amd import repeats
    s = setup
    idx, lines, objs = doubled(s)
    exp_mask = repeats.collapse_objects(objs).tolist()
    assert sum(exp_mask) > 1000 and any(exp_mask[a] for a in range(257, len(lines), 257))
    got, res = run_stream(sp, lines, 257, collapse_repeats=True, rules=True)
    assert np.concatenate([r.repeat for r in res]).tolist() == exp_mask
    assert [isinstance(g, s.ContractError) for g in got] == [s.ce[i] for i in idx]
    exp = [[] if m else texts_of(s.red[i]) for i, m in zip(idx, exp_mask)]
    bad = [(j, lines[j][:60]) for j, i in enumerate(idx) if not s.ce[i] and got[j] != exp[j]]
    assert not bad, (len(bad), bad[:3])
    assert not any(r.overflow for r in res) and sum(len(r.host) for r in res) <= 0.05 * len(lines)


def test_repeat_window_with_times(setup, sp):   # noqa: F811
    """Every decoding line three times, 0.4 s between lines, a window of 0.6 s: the second line is a repeat, the third
    stands 0.8 s behind the published one and is published again.  Expected: repeats.collapse_objects with the times,
    and the one-shot call."""
    from pysignalduino_amd import repeats
    s = setup
    idx, lines, objs = doubled(s, 3)
    times = np.arange(len(lines), dtype=np.int64) * 400_000
    exp_mask = repeats.collapse_objects(objs, times, 600_000, [None, 0, None]).tolist()
    plain = repeats.collapse_objects(doubled(s, 3)[2]).tolist()
    assert sum(exp_mask) > 1000 and sum(plain) > sum(exp_mask) + 1000      # the window does end runs here
    got, res = run_stream(sp, lines, 257, times=times, collapse_repeats=True, repeat_window=0.6, rules=True)
    assert np.concatenate([r.repeat for r in res]).tolist() == exp_mask
    exp = [[] if m else texts_of(s.red[i]) for i, m in zip(idx, exp_mask)]
    assert not [j for j, i in enumerate(idx) if not s.ce[i] and got[j] != exp[j]]
    one_shot = sp.parse_lines_json_all(lines, dispatch=True, collapse_repeats=True, times=times, repeat_window=0.6)
    assert sp.last_repeat_mask.tolist() == exp_mask
    assert not [j for j, i in enumerate(idx) if not s.ce[i] and got[j] != one_shot[j]]


def test_submit_bytes(setup, sp):   # noqa: F811
    s = setup
    one = [i for i in range(len(s.lines)) if s.lines[i].endswith("\n") and s.lines[i].count("\n") == 1]
    assert len(one) > 3000
    data = "".join(s.lines[i] for i in one).encode("latin-1")
    sub = SimpleNamespace(lines=[s.lines[i] for i in one], ce=[s.ce[i] for i in one], ContractError=s.ContractError)
    ls = sp.stream(chunk_lines=257, chunk_bytes=1 << 20, output="json_all", rules=True)
    ids = []
    for a in range(0, len(data), 100_000):                                 # read buffers that end inside lines
        ids += ls.submit_bytes(data[a: a + 100_000], final=a + 100_000 >= len(data))
    res = [r.detach() for r in ls.drain()]
    assert [r.id for r in res] == ids and sum(r.n for r in res) == len(one)
    compare(sub, [x for r in res for x in r.texts_all()], [texts_of(s.red[i]) for i in one])
    assert not any(r.overflow for r in res) and sum(len(r.host) for r in res) <= 0.05 * len(one)
    assert [ln for r in res for ln in r.lines()] == [x.encode("latin-1") for x in sub.lines]


def test_arguments(setup, sp):   # noqa: F811
    from pysignalduino_amd.routes import DEFAULT_ROUTES
    for kw in (dict(rules=True), dict(output="json", rules=True), dict(output="wire", rules=True),
               dict(output="json_all", routes=DEFAULT_ROUTES), dict(output="json_all", routes=DEFAULT_ROUTES, drop_unrouted=True),
               dict(output="json_all", routes=DEFAULT_ROUTES, route_match="any"), dict(output="json_all", rules="yes")):
        with pytest.raises(ValueError):
            sp.stream(chunk_lines=64, **kw)
    with pytest.raises(TypeError):
        sp.stream(chunk_lines=64, dispatch=True)
    ls = sp.stream(chunk_lines=64, output="json_all")
    ls.submit(setup.lines[:10])
    r = ls.drain()[0]
    with pytest.raises(ValueError):
        r.texts()
    with pytest.raises(ValueError):
        r.items()
    assert [i for i, _ in r.items_all()] == [i for i, x in enumerate(r.texts_all()) if isinstance(x, Exception) or x]
