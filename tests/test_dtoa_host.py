"""csrc/sdx_dtoa.h on the host: the header the device kernels compile, built into a stand-alone
program (tests/dtoa_driver.cpp) with AddressSanitizer + UndefinedBehaviorSanitizer and run over the
whole corpus of tests/repr_corpus.py.  Every text must be Python's repr() / json.dumps() byte for byte,
float(text) must give the value back, and the program must end clean.  The table of powers of ten is
regenerated and compared, and the generator's exactness checks run.  CPU only."""
import importlib.util
import math
import os
import subprocess

import pytest

import repr_corpus as RC

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
DRIVER = os.path.join(HERE, "dtoa_driver.cpp")
CSRC = os.path.join(REPO, "pysignalduino_amd", "csrc")
HEADER = os.path.join(CSRC, "sdx_dtoa.h")
TABLE = os.path.join(CSRC, "sdx_dtoa_pow10.h")


def _gen():
    spec = importlib.util.spec_from_file_location("gen_dtoa_pow10", os.path.join(REPO, "tools", "gen_dtoa_pow10.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert os.path.exists(HEADER), "pysignalduino_amd/csrc/sdx_dtoa.h is missing"
    out = str(tmp_path_factory.mktemp("dtoa") / "dtoa_san")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", DRIVER, "-o", out], check=True)
    return out


def _run(exe, values):
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    text = "".join("%016x\n" % RC.bits_of(v) for v in values)
    r = subprocess.run([exe], input=text, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, \
        f"rc={r.returncode}\n{r.stderr[-4000:]}"
    rows = r.stdout.split("\n")[:-1]
    assert len(rows) == len(values)
    return [tuple(row.split(" ")) for row in rows]


def test_table_is_what_the_generator_writes():
    with open(TABLE) as fh:
        assert fh.read() == _gen().render()


def test_generator_exactness_checks():
    """the shift-multiply logarithms, the range of h and of the table index, and the distance of every
    scaled value from the integers that lets 128 bits decide round-to-odd (check()'s docstring)"""
    r = _gen().check()
    assert r["min_distance_log2"] >= -68 and r["pairs"] > 600


def test_corpus_has_the_required_classes():
    cl = RC.classes()
    c = RC.corpus()
    assert 30000 <= len(c) <= 60000
    bits = {RC.bits_of(v) for v in c}
    for v in (0.0, -0.0, math.inf, -math.inf):
        assert RC.bits_of(v) in bits
    assert any(math.isnan(v) for v in c)
    for e in range(-1074, 1024):
        p = math.ldexp(1.0, e)
        assert RC.bits_of(p) in bits
        if e > -1074:
            assert RC.bits_of(math.nextafter(p, 0.0)) in bits
    for e in range(-323, 309):
        p = float("1e%d" % e)
        for w in RC.neighbours(p):
            assert RC.bits_of(w) in bits, (e, w)
    for v, t in ((9999999999999998.0, "9999999999999998.0"), (1e16, "1e+16"), (0.0001, "0.0001"),
                 (9.999999999999999e-05, "9.999999999999999e-05"), (1e-05, "1e-05"), (5e-324, "5e-324"),
                 (2.2250738585072014e-308, "2.2250738585072014e-308"), (1.7976931348623157e+308, "1.7976931348623157e+308"),
                 (RC.of_bits(0x000FFFFFFFFFFFFF), "2.225073858507201e-308")):
        assert RC.bits_of(v) in bits and repr(v) == t
    for i in (2 ** 53 - 1, 2 ** 53, 2 ** 53 + 2, 255, 256):
        assert RC.bits_of(float(i)) in bits
    for nd in (1, 15, 16, 17):
        vals = cl["digits%d" % nd]
        assert len(vals) >= 1000 and all(RC.ndigits(v) == nd for v in vals)
    assert RC.bits_of(377.25) in bits and RC.bits_of(0.5) in bits and RC.bits_of(-12.75) in bits
    assert len(cl["random_bits"]) == 20000
    assert c is RC.corpus() and [RC.bits_of(v) for v in RC.classes()["random_bits"][:50]] == \
        [RC.bits_of(v) for v in cl["random_bits"][:50]]                      # seeded


def test_header_equals_repr_and_json_under_asan_ubsan(exe):
    c = RC.corpus()
    got = _run(exe, c)
    bad = [(RC.bits_of(v), g, repr(v)) for v, g in zip(c, got)
           if g != (RC.expected(v, False), RC.expected(v, True))]
    assert not bad, f"{len(bad)} of {len(c)} differ from repr()/json.dumps(): {bad[:5]}"
    # second, independent condition: the text reads back as the value; and it fits the promise
    for v, (r, j) in zip(c, got):
        assert len(r) <= 24 and len(j) <= 24
        if math.isfinite(v):
            assert RC.bits_of(float(r)) == RC.bits_of(v) and RC.bits_of(float(j)) == RC.bits_of(v), (v, r, j)
