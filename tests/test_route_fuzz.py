"""k_route and k_route_rec (csrc/sdx_route.hip) on generated route tables and arbitrary bytes: tables of 1, 7 and
64 routes from tests/regex_corpus.py, one with 16-bit transitions, one that overflows the kernel's LDS, dozens of
byte classes; payloads over every byte value but the newline, at lengths 0 to 5 (the head4 register), up to
80, and 300.

Expected values come only from ``re.search`` over the payloads this test plants (``restate`` of test_routes.py,
``restate_pick`` of test_route_records_host.py); the planting and the comparisons are those tests' ``Planted`` /
``run`` / ``check`` and ``Plant`` / ``check``.  The compiler is used to choose tables (what it refuses is not
routed), never to say what a payload's route is."""
import random
import re
import struct
import warnings

import pytest

from pysignalduino_amd import regex_dfa, routes

import regex_corpus
import test_route_records as RR
import test_routes as TR
from test_routes import eng  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

LDS_BYTES = 20480       # SDX_ROUTE_LDS_BYTES (csrc/sdx_route_layout.h)
CHUNKS = (1, 64, 65, 257)
N_PAYLOADS = sum(CHUNKS)


def lds_routes_of(blob):
    """sdx_route_lds_routes restated: the routes whose tables end inside the kernel's LDS budget."""
    _, _, n_routes, n_class, width, _, _, _ = struct.unpack_from(routes.HDR_FMT, blob, 0)
    for r in range(n_routes):
        ns, _, _, t_off = struct.unpack_from(routes.DFA_FMT, blob, routes.DFA_OFF + 16 * r)
        if ((t_off + ns * n_class * width + 3) & ~3) - routes.CLS_OFF > LDS_BYTES:
            return r
    return n_routes


def draw(gen, n, probes, max_states=256):
    """n patterns of ``gen`` that re and the compiler take, that do not match the empty string and match at most
    2 % of ``probes`` (random text): a route that takes everything would leave nothing unrouted.  A group under
    an unbounded quantifier is left out: ``re``, the reference here, backtracks exponentially on 300 characters."""
    out = []
    while len(out) < n:
        pat = gen.pattern()
        if re.search(r"\)(?:[*+]|\{\d*,\})", pat.text):
            continue
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            try:
                rx = re.compile(pat.text)
            except re.error:
                continue
        if rx.search("") or sum(1 for s in probes if rx.search(s)) > len(probes) // 50:
            continue
        try:
            regex_dfa.compile_pattern(pat.text, max_states=max_states)
        except (NotImplementedError, ValueError):
            continue
        out.append(pat)
    return out


class Case:
    """A table and N_PAYLOADS planted results (kind, payload, trailer) with their routes by ``re`` alone."""

    def __init__(self, name, seed, n_full, n_payload, window=None):
        rng = random.Random(seed)
        full = regex_corpus.Generator(seed + 1, "full", stacked_rate=0.0, depth=1)
        pay = regex_corpus.Generator(seed + 2, "payload")
        probes = [full.random_text(rng.randint(1, 80)) for _ in range(100)] + [pay.payload_text() for _ in range(100)]
        pats = draw(full, n_full, probes) + draw(pay, n_payload, probes)
        rng.shuffle(pats)
        if window:      # an unanchored window of 2^(k+1) states and more: 16-bit transitions; not the first route
            wide = regex_corpus.Generator(seed + 3, "payload", window=(window, window))
            while True:
                p = wide.pattern()
                if re.search(r"\.\{%d\}" % window, p.text) and "|" not in p.text:
                    break
            pats.insert(1, p)
        self.name, self.pats = name, pats
        self.table = routes.RouteTable([("r%d" % i, p.text) for i, p in enumerate(pats)])
        self.n_class = struct.unpack_from(routes.HDR_FMT, self.table.blob, 0)[3]
        gens = {"full": full, "payload": pay}
        texts = []
        for ln in (0, 1, 2, 3, 4, 5):                       # the lengths around the head4 register, any bytes
            texts += [full.random_text(ln) for _ in range(3)]
        texts += [full.random_text(300) for _ in range(3)]
        near = []
        k = 0
        while len(texts) + 2 * len(near) < N_PAYLOADS - 60:     # strings built from the table's own patterns
            p = pats[k % len(pats)]
            near.append(gens[p.mode].near(p))
            k += 1
        while len(texts) + 2 * len(near) < N_PAYLOADS:
            texts.append(full.random_text(rng.randint(6, 80), high=rng.random() < 0.6 or None))
        # behind each payload stands what would change a verdict if it were read: a near string is planted whole in
        # front of the start of another one, and once more cut one character short in front of that character
        items = [(t, near[rng.randrange(len(near))] + "A0F") for t in texts + near]
        items += [(t[:-1], t[-1:] + "A0F") if t else (t, "A0F") for t in near]
        rng.shuffle(items)
        assert len(items) == N_PAYLOADS
        self.items = [(i % 4, t.encode("latin-1"), tr.encode("latin-1")) for i, (t, tr) in enumerate(items)]
        self.exp = [TR.restate(self.table.patterns, it[1]) for it in self.items]

    def conditions(self):
        """The properties of the payloads that keep the comparison from being vacuous, by ``re`` alone."""
        n = len(self.items)
        pays = [it[1] for it in self.items]
        assert all(b"\n" not in p for p in pays)
        assert {len(p) for p in pays} >= {0, 1, 2, 3, 4, 5, 300} and sum(5 < len(p) <= 80 for p in pays) >= 60
        assert sum(any(b >= 128 for b in p) for p in pays) >= n // 4
        seen = set().union(*pays)
        assert len(seen) >= 250 and 10 not in seen                         # every byte value but the newline
        routed = sum(r >= 0 for r, _ in self.exp)
        assert 0.1 * n <= routed <= 0.9 * n, routed
        # one byte too far: the verdict with the trailer's first byte appended differs for many a payload
        one_more = sum(TR.restate(self.table.patterns, it[1] + it[2][:1]) != e for it, e in zip(self.items, self.exp))
        assert one_more >= n // 20, one_more
        for ln in (3, 4, 5):        # head4 and the first byte behind it decide verdicts, both ways
            v = {r >= 0 for (r, _), p in zip(self.exp, pays) if len(p) == ln}
            assert v == {True, False} or len(self.table) == 1, (ln, v)
        return routed


@pytest.fixture(scope="module")
def cases():
    cache = {}
    spec = {"one": (11, 0, 1, None), "seven": (12, 7, 0, None), "sixtyfour": (13, 40, 24, None),
            "wide": (14, 3, 3, 8), "classes": (15, 20, 4, None)}

    def get(name):
        if name not in cache:
            cache[name] = Case(name, *spec[name])
        return cache[name]
    return get


def test_the_tables_have_the_shapes_the_kernels_branch_on(eng, cases):   # noqa: F811
    one, seven, big, wide, classes = (cases(k) for k in ("one", "seven", "sixtyfour", "wide", "classes"))
    assert (len(one.table), len(seven.table), len(big.table)) == (1, 7, 64)
    assert wide.table.blob[16] == 2 and all(c.table.blob[16] == 1 for c in (one, seven, big, classes))
    assert 0 < lds_routes_of(big.table.blob) < 64 and 0 < lds_routes_of(wide.table.blob) < len(wide.table)
    assert lds_routes_of(seven.table.blob) == 7
    assert classes.n_class >= 24 and big.n_class >= 24
    for c in (one, seven, big, wide, classes):
        assert eng.route_table(c.table).lds_routes == lds_routes_of(c.table.blob)
        c.conditions()
    hit = set()
    for _, m in big.exp:
        hit |= {r for r in range(64) if m >> r & 1}
    assert len(hit) >= 40, len(hit)
    firsts = {r for r, _ in big.exp}
    assert any(r >= lds_routes_of(big.table.blob) for r in firsts)      # a route decided in global memory


@pytest.mark.parametrize("name", ["one", "seven", "sixtyfour", "wide", "classes"])
def test_route_lines_on_generated_tables(eng, cases, name):   # noqa: F811
    """sdx_route_lines in chunks of 1, 64, 65 and 257 lines over all four kinds: route and mask equal the
    definition, and the route alone when no mask is given (``check`` of test_routes.py)."""
    c = cases(name)
    at = 0
    for n in CHUNKS:
        items = c.items[at: at + n]
        assert TR.check(eng, c.table, items) == c.exp[at: at + n]
        assert n == 1 or {it[0] for it in items} == {0, 1, 2, 3}
        at += n
    assert at == len(c.items)


@pytest.mark.parametrize("name", ["one", "seven", "sixtyfour", "wide", "classes"])
def test_route_records_on_generated_tables(eng, cases, name):   # noqa: F811
    """sdx_route_records over the same payloads as lines of 1 to 5 records: pick, route and mask are those of
    the first record in list order that any route matches (``check`` of test_route_records.py)."""
    c = cases(name)
    rng = random.Random(len(c.table))
    at = 0
    picks, unrouted = set(), 0
    for n in CHUNKS:
        idx = [[rng.randrange(len(c.items)) for _ in range(rng.randint(1, 5))] for _ in range(n)]
        lines = [[((at + i) % 4, [(1 + j, c.items[x][1], c.items[x][2]) for j, x in enumerate(ix)])] for i, ix in enumerate(idx)]
        assert n == 1 or {len(ix) for ix in idx} == {1, 2, 3, 4, 5}
        _, exp = RR.check(eng, c.table, lines)
        # the definition once more, from the routes by re alone that this module computed for every payload
        assert exp == [next(((j,) + c.exp[x] for j, x in enumerate(ix) if c.exp[x][0] >= 0), (0, -1, 0)) for ix in idx]
        picks |= {e[0] for e in exp if e[1] >= 0}
        unrouted += sum(e[1] < 0 for e in exp)
        at += n
    assert picks >= {0, 1, 2} and unrouted >= 10
