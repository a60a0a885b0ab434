"""regex_dfa.py against Python's ``re`` (CPU): generated patterns (tests/regex_corpus.py) on strings over every
byte value but the newline, the class escapes on every code point, and the patterns ``re.compile`` refuses.

The definition is ``re.search(pattern, text)`` on ``str``, the text being the payload's latin-1 decoding
(routes.py; ``restate`` of test_routes.py).  ``$`` before a trailing newline is the documented difference
(regex_dfa.py) and stays out of the inputs: no string holds a newline."""
import re
import warnings

import pytest

from pysignalduino_amd import regex_dfa

import regex_corpus

MAX_STATES = 300        # keeps the pure-Python subset construction fast; beyond it compile_pattern raises ValueError
N_PATTERNS = {"full": 2400, "payload": 400}
REFUSED_BY_RE = [r"a**", r"a++a", r"a*+a", r"a?+a", r"a{2}{3}", r"a{1,2}{2}", r"a{3,2}", r"[\w-z]", r"[z-a]", r"^*a",
                 r"$?7", r"(?:a{2})?+a", r"a+?*", r"a{2}+", r"{2}a", r"b|{1,2}", r"(?:*a)", r"[a-\d]", r"[\D-x]",
                 r"^{2}", r"$+", r"a{2,1}?", r"(a", r"a)", r"[a", "a\\"]
NOT_LATIN_1 = ["€", "[€]", "[a-€]", "[a-\\€]", "\\€", "[\\€]"]    # re takes them; a payload is bytes


def re_compile(pattern):
    """re.compile, or None where it refuses.  A warning (a nested set, say) would be a generator mistake."""
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        try:
            return re.compile(pattern)
        except re.error:
            return None


def dfa_compile(patterns):
    """compile_bank_dfas, or None where the compiler refuses (syntax: NotImplementedError; a limit: ValueError)."""
    try:
        return regex_dfa.compile_bank_dfas(patterns, max_states=MAX_STATES)
    except (NotImplementedError, ValueError):
        return None


@pytest.fixture(scope="module", params=["full", "payload"])
def corpus(request):
    """-> (mode, [(Pattern, compiled re or None, its strings)]), generated once."""
    mode = request.param
    gen = regex_corpus.Generator(seed=20 if mode == "full" else 21, mode=mode)
    out = []
    for _ in range(N_PATTERNS[mode]):
        pat = gen.pattern()
        out.append((pat, re_compile(pat.text), gen.strings(pat)))
    return mode, out


def test_generated_patterns_equal_re_search(corpus):
    """Every generated pattern both sides accept, alone and in tables of 8 over shared byte classes:
    dfa_search == bool(re.search) on every one of its strings.  The conditions below keep that from being
    vacuous; they are properties of the generator and of ``re`` alone, apart from the refusal rate."""
    mode, cases = corpus
    both, refused = [], 0
    for pat, rx, strings in cases:
        assert all("\n" not in s and max(map(ord, s), default=0) < 256 for s in strings)
        one = dfa_compile([pat.text])
        if rx is None:
            assert one is None, "re.compile refuses %r, compile_pattern takes it" % pat.text
            continue
        if one is None:
            refused += 1
            continue
        both.append((pat, rx, strings, [bool(rx.search(s)) for s in strings]))
        cls_of, _, (dfa,) = one
        got = [regex_dfa.dfa_search(dfa, cls_of, s.encode("latin-1")) for s in strings]
        bad = [(pat.text, s, e) for s, e, g in zip(strings, both[-1][3], got) if e != g]
        assert not bad, bad[:3]
    accepted_by_re = sum(rx is not None for _, rx, _ in cases)
    # at most 15 % of the patterns re takes are refused by compile_pattern (limits and unsupported syntax)
    assert refused <= 0.15 * accepted_by_re, (refused, accepted_by_re)
    assert len(both) >= (200 if mode == "full" else 100), len(both)
    # at least half of the compiled patterns see a match and a non-match
    mixed = sum(any(e) and not all(e) for _, _, _, e in both)
    assert mixed >= 0.5 * len(both), (mixed, len(both))
    # at least a fifth of all strings hold a byte >= 0x80: of the full corpus only -- the payload corpus is
    # preambles and hex digits by construction, and its strings are not counted towards the share
    if mode == "full":
        strings = [s for _, _, ss, _ in both for s in ss]
        high = sum(any(ord(c) >= 128 for c in s) for s in strings)
        assert high >= 0.2 * len(strings), (high, len(strings))
        assert sum(rx is None for _, rx, _ in cases) >= 3       # the stacked quantifiers did occur
    # tables of 8: the shared byte classes; every table's strings go to every pattern of the table
    for a in range(0, len(both) - 7, 8):
        group = both[a: a + 8]
        table = dfa_compile([g[0].text for g in group])
        assert table is not None
        cls_of, n_class, dfas = table
        assert len(dfas) == 8 and max(cls_of) == n_class - 1
        strings = [s for g in group for s in g[2][:10]]
        for (pat, rx, _, _), dfa in zip(group, dfas):
            bad = [(pat.text, s) for s in strings
                   if regex_dfa.dfa_search(dfa, cls_of, s.encode("latin-1")) != bool(rx.search(s))]
            assert not bad, bad[:3]


ONE_CHAR = [chr(c) for c in range(256) if c != 10]


@pytest.mark.parametrize("form", ["\\%s", "[\\%s]", "[^\\%s]", "[\\%sx-]", "^[^\\%s#]$"])
@pytest.mark.parametrize("esc", list("dwsDWS"))
def test_class_escapes_on_every_code_point(esc, form):
    pattern = form % esc
    rx = re.compile(pattern)
    cls_of, _, (dfa,) = regex_dfa.compile_bank_dfas([pattern])
    bad = [(pattern, hex(ord(c))) for c in ONE_CHAR
           if regex_dfa.dfa_search(dfa, cls_of, c.encode("latin-1")) != bool(rx.search(c))]
    assert not bad, bad[:8]


def test_issue_table_of_class_escapes():
    for pattern, text, want in ((r"\w", "\xe9", True), (r"^\S$", "\xa0", False), (r"\s", "\x1f", True)):
        assert bool(re.search(pattern, text)) == want
        cls_of, _, (dfa,) = regex_dfa.compile_bank_dfas([pattern])
        assert regex_dfa.dfa_search(dfa, cls_of, text.encode("latin-1")) == want, (pattern, text)


@pytest.mark.parametrize("pattern", REFUSED_BY_RE)
def test_what_re_refuses_is_refused(pattern):
    """The same rule under every Python: x++, x*+ and x?+ are refused even where ``re`` reads them as
    possessive (3.11 on), so the list is not filtered by the running ``re``."""
    with pytest.raises((NotImplementedError, ValueError)):
        regex_dfa.compile_pattern(pattern)
    with pytest.raises((NotImplementedError, ValueError)):
        regex_dfa.compile_bank_dfas(["^P", pattern])


@pytest.mark.parametrize("pattern", NOT_LATIN_1)
def test_code_points_above_255_are_refused(pattern):
    """Nowhere truncated silently: not as a literal, not in a class, not as a range's upper end."""
    assert re_compile(pattern) is not None
    with pytest.raises(NotImplementedError):
        regex_dfa.compile_pattern(pattern)


def test_the_refused_list_is_refused_by_this_re():
    """Documents the list: apart from the possessive forms of newer Pythons, re.compile refuses each."""
    possessive = {r"a++a", r"a*+a", r"a?+a", r"(?:a{2})?+a", r"a{2}+", r"$+"}
    for pattern in REFUSED_BY_RE:
        if re_compile(pattern) is not None:
            assert pattern in possessive, pattern


def test_neighbours_of_the_refusals_still_compile():
    """What looks like a refused form and is not: lazy quantifiers, a literal brace, a quantified group that
    holds an anchor or a quantifier, a class escape beside a trailing dash."""
    for pattern, hit, miss in ((r"a*?b", "ab", "a"), (r"a??b", "b", "a"), (r"a{2}?b", "aab", "ab"), (r"a{2,3}?$", "aaa", "a"),
                               (r"a{x", "a{x", "ax"), (r"a{", "a{", "a"), (r"x{,a}", "x{,a}", "x"), (r"(?:a*)*b", "b", "a"),
                               (r"(a+)+$", "aaa", "ab"), (r"(?:^)*a", "a", "b"), (r"(^a)?b", "ab", "a"), (r"(?:a$)?b", "b", "a"),
                               (r"[\w-]+$", "a-\xe9", "a #"), (r"[\d-]x", "-x", "ax"), (r"a{,2}b", "aab", "a")):
        assert re.search(pattern, hit) and not re.search(pattern, miss)
        cls_of, _, (dfa,) = regex_dfa.compile_bank_dfas([pattern])
        assert regex_dfa.dfa_search(dfa, cls_of, hit.encode("latin-1")), (pattern, hit)
        assert not regex_dfa.dfa_search(dfa, cls_of, miss.encode("latin-1")), (pattern, miss)
