"""Seeded generator of regular expressions and of strings to try them on (a helper, not a test).

The patterns stay inside the syntax pysignalduino_amd/regex_dfa.py lists: literals (escaped punctuation, one
latin-1 letter), ``.``, ``\\d \\w \\s \\D \\W \\S``, classes (ranges, negation, escapes, a leading ``]``, a trailing
``-``), ``(...)`` and ``(?:...)``, ``|`` with empty branches, ``* + ? {m} {m,} {m,n} {,n}`` and their lazy forms,
``^`` and ``$`` anywhere.  At a small rate a quantifier is stacked on a quantified item or its bounds are
reversed: what ``re.compile`` refuses the compiler has to refuse too.

Nothing here imports the code under test or ``re``: a pattern is a tree that is rendered to text and, for its
strings, sampled -- a branch picked, a count picked inside the bounds, a character picked from each set -- so
that matches occur without asking any engine.  No string holds a newline (``$`` before a trailing newline is
the documented difference, regex_dfa.py).

``mode="payload"`` restricts both to what a decoded telegram looks like: a preamble (``P7#``, ``W33#``, ``u40#``,
bare letters), hex digits, ``#``; counted hex classes, windows (``A.{6}B``), alternations of digit pairs."""
import random

HEX = "0123456789ABCDEF"
LITERALS = "abAB01#xZ_ "
ESCAPED = ".*+?()[]{}|^$\\-"           # punctuation written with a backslash
LATIN = "\xe9"
CLASS_SAMPLES = {"d": "0598", "w": "aZ_5\xe9\xb5", "s": " \t\xa0\x1f\x85", "D": "a# \xff", "W": "# \xa0-\x1c", "S": "a#\xe9_0"}
PREAMBLES = ["P7#", "P12#", "P61#", "P56#", "W33#", "W113x#", "u40#", "u9#", "i", "s", "TX", "Ys", "K", "E0"]
ALL_BUT_NL = [chr(c) for c in range(256) if c != 10]


# ---- rendering and sampling a tree -------------------------------------------------------------------
def render(node):
    t = node[0]
    if t == "lit":
        return node[1]
    if t == "any":
        return "."
    if t == "esc":
        return "\\" + node[1]
    if t == "cls":
        _, neg, lead, items, dash = node
        body = "".join(it[1] if it[0] == "c" else it[1] + "-" + it[2] if it[0] == "r" else "\\" + it[1] for it in items)
        return "[" + ("^" if neg else "") + ("]" if lead else "") + body + ("-" if dash else "") + "]"
    if t == "grp":
        return ("(" if node[1] else "(?:") + render(node[2]) + ")"
    if t == "alt":
        return "|".join(render(b) for b in node[1])
    if t == "seq":
        return "".join(render(x) for x in node[1])
    if t == "rep":
        return render(node[1]) + node[2]
    if t == "bol":
        return "^"
    if t == "eol":
        return "$"
    raise AssertionError(t)


def sample(node, rng):
    """A string the node is likely to match (anchors contribute nothing; a negated class guesses)."""
    t = node[0]
    if t == "lit":
        return node[2]
    if t == "any":
        return rng.choice(ALL_BUT_NL)
    if t == "esc":
        return rng.choice(CLASS_SAMPLES[node[1]])
    if t == "cls":
        _, neg, lead, items, dash = node
        if neg:
            return rng.choice("q%GÿÀ7 ")
        pool = (["]"] if lead else []) + (["-"] if dash else [])
        for it in items:
            pool.append(it[2] if it[0] == "c" else chr(rng.randint(ord(it[3]), ord(it[4]))) if it[0] == "r"
                        else rng.choice(CLASS_SAMPLES[it[1]]))
        return rng.choice(pool)
    if t == "grp":
        return sample(node[2], rng)
    if t == "alt":
        return sample(rng.choice(node[1]), rng)
    if t == "seq":
        return "".join(sample(x, rng) for x in node[1])
    if t == "rep":
        _, sub, _, m, n = node
        hi = m + 2 if n is None else min(n, m + 2)
        return "".join(sample(sub, rng) for _ in range(rng.randint(min(m, hi), hi)))
    return ""


class Pattern:
    def __init__(self, tree, mode):
        self.tree, self.mode, self.text = tree, mode, render(tree)

    def __repr__(self):
        return "Pattern(%r)" % self.text


# ---- the generator ---------------------------------------------------------------------------------------
class Generator:
    """``Generator(seed, mode).pattern()`` -> Pattern; ``strings(pattern, n)`` -> n str.  mode: "full" or "payload"."""

    def __init__(self, seed, mode="full", stacked_rate=0.03, window=(2, 6), depth=2):
        """stacked_rate: how often a quantifier is one re.compile refuses; window: the k of payload mode's
        ``X.{k}Y`` (its DFA has about 2^(k+1) states); depth: how deep groups nest in full mode."""
        assert mode in ("full", "payload")
        self.rng = random.Random(seed)
        self.mode = mode
        self.stacked_rate = stacked_rate
        self.window = window
        self.depth = depth

    # -- full mode
    def _literal(self):
        r = self.rng
        x = r.random()
        if x < 0.70:
            c = r.choice(LITERALS)
            return ("lit", c, c)
        if x < 0.90:
            c = r.choice(ESCAPED)
            return ("lit", "\\" + c, c)
        return ("lit", LATIN, LATIN)

    def _class(self):
        r = self.rng
        items = []
        for _ in range(r.randint(0 if r.random() < 0.2 else 1, 4)):
            x = r.random()
            if x < 0.40:
                c = r.choice("abAB019#xZ_" + LATIN)
                items.append(("c", c, c))
            elif x < 0.50:
                c = r.choice("]-^\\")
                items.append(("c", "\\" + c, c))
            elif x < 0.80:
                lo, hi = sorted(r.sample("09AFZaf" + LATIN + "\xff", 2))
                items.append(("r", lo, hi, lo, hi))
            else:
                items.append(("e", r.choice("dwsDWS")))
        lead = r.random() < 0.15 or not items
        dash = r.random() < 0.15
        return ("cls", r.random() < 0.3, lead, items, dash)

    def _quantifier(self):
        """(text, m, n) with n None for no upper bound."""
        r = self.rng
        x = r.random()
        if x < 0.12:
            q = ("*", 0, None)
        elif x < 0.37:
            q = ("+", 1, None)
        elif x < 0.50:
            q = ("?", 0, 1)
        else:        # mostly not nullable: a pattern that matches the empty string matches every string
            m = r.choice([0, 1, 1, 2, 2, 3])
            n = m + r.randint(0, 2)
            q = r.choice([("{%d}" % m, m, m), ("{%d,}" % m, m, None), ("{%d,%d}" % (m, n), m, n), ("{%d,%d}" % (m, n), m, n),
                          ("{%d}" % m, m, m), ("{,%d}" % n, 0, n)])
        if r.random() < 0.25:
            q = (q[0] + "?",) + q[1:]
        return q

    def _item(self, depth):
        r = self.rng
        x = r.random()
        if x < 0.07:
            return ("bol",)
        if x < 0.14:
            return ("eol",)
        if x < 0.50:
            atom = self._literal()
        elif x < 0.58:
            atom = ("any",)
        elif x < 0.68:
            atom = ("esc", r.choice("dwsDWS"))
        elif x < 0.83 or depth <= 0:
            atom = self._class()
        else:
            atom = ("grp", r.random() < 0.4, self._alt(depth - 1))
        if r.random() < 0.4:
            text, m, n = self._quantifier()
            if r.random() < self.stacked_rate:       # what re.compile refuses: x**, x{2}{3}, x?+, x{3,2}
                if r.random() < 0.3:
                    return ("rep", atom, "{%d,%d}" % (m + 1 + r.randint(0, 2), m), m, m)
                return ("rep", ("rep", atom, text, m, n), r.choice(["*", "+", "{2}", "{1,2}"]), 1, 1)
            return ("rep", atom, text, m, n)
        return atom

    def _seq(self, depth):
        r = self.rng
        k = 0 if r.random() < 0.05 else r.randint(1, 4)
        return ("seq", [self._item(depth) for _ in range(k)])

    def _alt(self, depth):
        r = self.rng
        k = 1 if r.random() < 0.7 else r.randint(2, 3)
        return ("alt", [self._seq(depth) for _ in range(k)])

    # -- payload mode
    def _hexclass(self):
        r = self.rng
        return r.choice([("cls", False, False, [("r", "0", "9", "0", "9"), ("r", "A", "F", "A", "F")], False),
                         ("cls", False, False, [("r", "A", "F", "A", "F")], False),
                         ("cls", False, False, [("r", "0", "9", "0", "9")], False),
                         ("cls", True, False, [("r", "0", "7", "0", "7")], False),
                         ("esc", "d"), ("any",)])

    def _hexlit(self, k):
        return [("lit", c, c) for c in (self.rng.choice(HEX) for _ in range(k))]

    def _payload_pattern(self):
        r = self.rng
        items = []
        anchored = r.random() < 0.55
        if anchored:
            items.append(("bol",))
            items += [("lit", c, c) for c in r.choice(PREAMBLES)]
        for _ in range(r.randint(1, 3)):
            x = r.random()
            if x < 0.35:        # a counted body
                m = r.randint(1, 8)
                n = m + r.randint(0, 6)
                q = r.choice([("{%d}" % m, m, m), ("{%d,%d}" % (m, n), m, n), ("{%d,}" % m, m, None), ("+", 1, None), ("*", 0, None)])
                items.append(("rep", self._hexclass(), *q))
            elif x < 0.55:      # literal digits
                items += self._hexlit(r.randint(1, 2))
            elif x < 0.75 and not anchored:     # a window: X.{k}Y
                k = r.randint(*self.window)
                items += self._hexlit(1) + [("rep", ("any",), "{%d}" % k, k, k)] + self._hexlit(1)
            elif x < 0.90:      # an alternation of digit pairs
                alts = ("alt", [("seq", self._hexlit(2)) for _ in range(r.randint(2, 3))])
                m = r.randint(1, 2)
                n = m + r.randint(0, 2)
                items.append(("rep", ("grp", False, alts), "{%d,%d}" % (m, n), m, n))
            else:
                items.append(self._hexclass())
        if r.random() < 0.4:
            items.append(("eol",))
        return ("alt", [("seq", items)])

    def pattern(self):
        return Pattern(self._payload_pattern() if self.mode == "payload" else self._alt(self.depth), self.mode)

    # -- strings
    def random_text(self, n, high=None):
        """n characters over every byte value but the newline; high=False: below 0x80 only."""
        r = self.rng
        pool = ALL_BUT_NL if high is None else [c for c in ALL_BUT_NL if (ord(c) >= 128) == high]
        return "".join(r.choice(pool) for _ in range(n))

    def payload_text(self):
        r = self.rng
        return r.choice(PREAMBLES + ["", "75"]) + "".join(r.choice(HEX) for _ in range(r.randint(0, 26)))

    def near(self, pat):
        """A sampled string as it is, inside junk, or with one character changed or dropped."""
        r = self.rng
        s = sample(pat.tree, r)
        junk = (lambda: self.random_text(r.randint(1, 3))) if self.mode == "full" else (lambda: r.choice(HEX + "#P"))
        x = r.random()
        if x < 0.30:
            return s
        if x < 0.45:
            return junk() + s
        if x < 0.60:
            return s + junk()
        if x < 0.70:
            return junk() + s + junk()
        if not s:
            return junk()
        j = r.randrange(len(s))
        return s[:j] + (junk() if x < 0.85 else "") + s[j + 1:]

    def strings(self, pat, n=24):
        """The empty string, random strings, and strings built from the pattern's own sets."""
        r = self.rng
        out = [""]
        for k in range(n - 1):
            if k % 3 == 0:
                out.append(self.random_text(r.randint(1, 12)) if self.mode == "full" else self.payload_text())
            else:
                out.append(self.near(pat))
        return out
