"""The string corpus of the exact float() tests (tests/test_strtod_host.py on the CPU,
tests/test_float_exact.py on the GPU): deterministic, about 5,000 ASCII strings.  The expected value
of every string is Python's own float(s), computed by the tests; nothing is recorded here."""
import functools
import math
import random
import struct
from fractions import Fraction

SYNTAX_BAD = ["", " ", "1__0", "_1", "1_", "1_e5", "1._5", "1e_5", "1e", "1e+", ".", "+.", "+-1", "0x10", "1e5.0",
              "infinit", "in", "1.5\x1c", "\x1c1.5", "1 .5"]
SYNTAX_OK = ["1e1_0", "1_0.0_1e0_1", "1.e5", "+.5e1", " 1.5\n", "\x0b1.5\x0c", "nan", "-NaN", "+iNfInItY"]


def exact_decimal(fr: Fraction) -> str:
    """The exact decimal expansion of a non-negative dyadic fraction, as 'iii.fff' or 'iii'."""
    assert fr >= 0
    den = fr.denominator
    k = den.bit_length() - 1
    assert den == 1 << k, "a dyadic fraction"
    if k == 0:
        return str(fr.numerator)
    digits = str(fr.numerator * 5 ** k).rjust(k + 1, "0")   # fr = numerator * 5^k / 10^k
    ip, fp = digits[:-k], digits[-k:].rstrip("0")
    return ip + ("." + fp if fp else "")


def _next_up(x: float) -> Fraction:
    """The double after x as a Fraction, or 2^1024 after the largest double."""
    y = math.nextafter(x, math.inf)
    return Fraction(2) ** 1024 if math.isinf(y) else Fraction(y)


def _lower_last(s: str) -> str:
    """s with its last digit lowered by one (an integer that ends in 0 borrows; a fraction never ends in 0)."""
    if s[-1] == "0":
        assert "." not in s
        return str(int(s) - 1)
    return s[:-1] + str(int(s[-1]) - 1)


def _with_point(s: str) -> str:
    return s if "." in s else s + "."


def midpoint_doubles(rng: random.Random):
    xs = [5e-324, 2.2250738585072009e-308, float(2 ** 53), 1.7976931348623157e308, 1.0, 0.5, 3.0]
    assert xs[1] == struct.unpack("<d", struct.pack("<Q", (1 << 52) - 1))[0]   # the largest subnormal
    for _ in range(220):   # normals over the whole exponent range
        xs.append(struct.unpack("<d", struct.pack("<Q", (rng.randrange(1, 2047) << 52) | rng.getrandbits(52)))[0])
    for _ in range(80):    # subnormals
        xs.append(struct.unpack("<d", struct.pack("<Q", rng.randrange(1, 1 << 52)))[0])
    for k in (1, 2, 3, 1 << 51, (1 << 52) - 2):   # the smallest subnormals: the 750+ digit midpoints
        xs.append(struct.unpack("<d", struct.pack("<Q", k))[0])
    return xs


def midpoint_strings(rng: random.Random):
    out = []
    for x in midpoint_doubles(rng):
        mid = exact_decimal((Fraction(x) + _next_up(x)) / 2)
        out.append(mid)
        for k in (0, 300):
            out.append(_with_point(mid) + "0" * k + "1")
        out.append(_lower_last(mid))
    out.append(exact_decimal(Fraction(5e-324) / 2))   # half of the smallest subnormal -> 0.0
    out.append("-" + exact_decimal(Fraction(5e-324) / 2))
    return out


@functools.lru_cache(maxsize=None)
def corpus():
    """The whole corpus as a tuple of str (ASCII only)."""
    rng = random.Random(20261019)
    out = list(midpoint_strings(rng))
    # the families of tests/golden/lines_float_golden.json.gz
    out += ["9007199254740993", "9007199254740993.0", "9007199254740995", "9007199254740993.0" + "0" * 700 + "1",
            "-249.1234567890123456789"]
    for n in (1, 2, 5, 17, 444, 1446, 99999):
        for sg in ("", "-", "+"):
            out += [f"{sg}{n}e400", f"{sg}{n}e-400"]
    # boundaries
    out += ["1.7976931348623157e308", "1.7976931348623158e308", "1e309", "4.9e-324", "2.4703282292062327e-324",
            "2.4703282292062328e-324", "2.2250738585072011e-308", "2.2250738585072012e-308",
            "2.2250738585072014e-308"]
    # exponent bookkeeping
    out += ["1e99999999999999999999", "-1e-99999999999999999999", "0e99999999999999999999",
            "1e9223372036854775807", "1e-9223372036854775808", "1e18446744073709551616",
            "0." + "0" * 400 + "1e401", "1" + "0" * 400 + "e-400",
            "0." + "0" * 3000 + "1e3001", "1" + "0" * 3000 + "e-3000",
            "0" * 500 + "1." + "0" * 500, "." + "0" * 340 + "1", "1" + "0" * 310]
    # long digit strings
    for nd in (20, 21, 100, 767, 768, 769, 800, 2000):
        for _ in range(30):
            sig = str(rng.randrange(1, 10)) + "".join(rng.choice("0123456789") for _ in range(nd - 1))
            cut = rng.randrange(0, nd + 1)
            s = sig[:cut] + "." + sig[cut:] if rng.random() < 0.7 else sig
            e = rng.randrange(-350, 321) - (cut if "." in s else nd) * (rng.random() < 0.5)
            out.append(("-" if rng.random() < 0.3 else "") + s + f"e{e}")
    # repr of random doubles with 1-30 random digits appended to the significand
    for _ in range(2000):
        x = struct.unpack("<d", struct.pack("<Q", rng.getrandbits(64)))[0]
        if x != x or math.isinf(x):
            x = rng.random()
        r = repr(x)
        mant, _, ex = r.partition("e")
        if "." not in mant:
            mant += "."
        mant += "".join(rng.choice("0123456789") for _ in range(rng.randrange(1, 31)))
        out.append(mant + ("e" + ex if ex else ""))
    # short significands over the whole exponent range, the subnormal and overflow edges included
    for _ in range(500):
        nd = rng.randrange(1, 26)
        sig = "".join(rng.choice("0123456789") for _ in range(nd))
        out.append(("-" if rng.random() < 0.3 else "") + sig[:1] + "." + sig[1:] + f"e{rng.randrange(-345, 311)}")
    # syntax
    out += SYNTAX_BAD + SYNTAX_OK
    out += ["inf", "-inf", "Infinity", "-INFINITY", "+nan", "1.", ".5", "-.5e-3", "1E5", "1e+05", "1e-05", "00012",
            "-0", "-0.0", "0e5", "-0e-5", "1_000_000", "1.5e", "1.5e+", "e5", ".e5", "1..5", "--1", "1e5e5", "nan1",
            "infinityx", "\t\r 7 \f\v", "7\x00", "1,5", "1_.5", "1e1__0", "12a"]
    # strings inside the one-operation fast path: the answers of the present front end
    out += [str(v) for v in range(-32768, 32768, 131)] + ["-1446.5", "1446.25", "-32768", "32767", "123456789012345678",
                                                          "9007199254740991", "1e22", "1e-22", "123.456e-20"]
    out += [f"{rng.randrange(-99999, 100000)}.{rng.randrange(0, 1000):03d}" for _ in range(200)]
    assert all(ord(c) < 128 for s in out for c in s)
    return tuple(out)


def float_bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def expected(s: str):
    """(class, bits) of Python's float(s): (0, 0) where it raises ValueError."""
    try:
        return 1, float_bits(float(s))
    except ValueError:
        return 0, 0
