"""The value corpus of the repr(float) tests (tests/test_dtoa_host.py on the CPU,
tests/test_repr_device.py on the GPU): binary64 values by class, seeded, about 40k values."""
import json
import math
import random
import struct

SEED = 20260


def bits_of(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def of_bits(b: int) -> float:
    return struct.unpack("<d", struct.pack("<Q", b & (2 ** 64 - 1)))[0]


def neighbours(x: float):
    return [math.nextafter(x, -math.inf), x, math.nextafter(x, math.inf)]


def ndigits(x: float) -> int:
    """significant digits of repr(x), x finite and non-zero"""
    m = repr(abs(x)).split("e")[0].replace(".", "").lstrip("0")
    return len(m.rstrip("0")) or 1


SPECIAL = [0.0, -0.0, math.inf, -math.inf, math.nan]
DECPT = [9999999999999998.0, 1e16, 0.0001, 9.999999999999999e-05, 1e-05]
EXTREMES = [5e-324, of_bits(0x000FFFFFFFFFFFFF), 2.2250738585072014e-308, 1.7976931348623157e+308]


def classes():
    """name -> list of floats"""
    rng = random.Random(SEED)
    c = {}
    c["special"] = list(SPECIAL)
    c["pow2"] = [math.ldexp(1.0, e) for e in range(-1074, 1024)]
    c["pow2_below"] = [math.nextafter(v, 0.0) for v in c["pow2"][1:]]
    c["pow10"] = [w for e in range(-323, 309) for w in neighbours(float("1e%d" % e))]
    c["decpt"] = [w for v in DECPT for w in neighbours(v)]
    c["extremes"] = [w for v in EXTREMES for w in neighbours(v) if not math.isinf(w)]
    ints = list(range(0, 300)) + [rng.randrange(2 ** k, 2 ** (k + 1)) for k in range(8, 53) for _ in range(20)]
    ints += [2 ** 53 - 2, 2 ** 53 - 1, 2 ** 53, 2 ** 53 + 2, 2 ** 53 + 4, 2 ** 54 + 4, 2 ** 63, 2 ** 64, 10 ** 15 - 1,
             10 ** 15, 10 ** 16 - 2, 10 ** 16, 10 ** 16 + 2, 10 ** 17, 10 ** 22, 10 ** 23]
    c["ints"] = [float(i) for i in ints]
    c["halves_quarters"] = [i / 4.0 for i in range(-200, 2000)] + [rng.randrange(1, 100000) / 4.0 for _ in range(600)]
    for nd in (1, 2, 3, 8, 15, 16, 17):   # decimal literals of nd digits at random exponents
        vals = []
        while len(vals) < 1200:
            m = rng.randrange(10 ** (nd - 1), 10 ** nd)
            if m % 10 == 0:
                continue
            v = float("%de%d" % (m, rng.randrange(-325, 309 - nd)))
            if v == 0.0 or math.isinf(v) or ndigits(v) != nd:
                continue
            vals.append(v if rng.random() < 0.7 else -v)
        c["digits%d" % nd] = vals
    c["clockish"] = [rng.randrange(100, 3000) + rng.choice([0.1, 0.25, 0.0625, 0.123456789, 0.3, 0.7]) for _ in range(500)]
    rnd = [of_bits(rng.getrandbits(64)) for _ in range(20000)]
    c["random_bits"] = rnd
    c["random_subnormal"] = [of_bits(rng.getrandbits(52) | (rng.getrandbits(1) << 63)) for _ in range(1000)]
    c["random_mid"] = [rng.uniform(-1, 1) * 10.0 ** rng.randrange(-8, 24) for _ in range(3000)]
    return c


_CACHE = {}


def corpus():
    """the whole corpus as a list of floats (the same list every call)"""
    if "c" not in _CACHE:
        _CACHE["c"] = [v for vals in classes().values() for v in vals]
    return _CACHE["c"]


def expected(x: float, json_form: bool) -> str:
    return json.dumps(x) if json_form else repr(x)
