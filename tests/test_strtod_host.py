"""csrc/sdx_strtod.h on the host: the header the device kernels compile, built into a stand-alone
program (tests/strtod_driver.cpp) with AddressSanitizer + UndefinedBehaviorSanitizer and run over
the whole corpus of tests/float_corpus.py.  Every answer must be Python's float() bit for bit and
the program must end clean.  CPU only."""
import os
import subprocess

import pytest

import float_corpus as FC

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
DRIVER = os.path.join(HERE, "strtod_driver.cpp")
HEADER = os.path.join(REPO, "pysignalduino_amd", "csrc", "sdx_strtod.h")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert os.path.exists(HEADER), "pysignalduino_amd/csrc/sdx_strtod.h is missing"
    out = str(tmp_path_factory.mktemp("strtod") / "strtod_san")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", DRIVER, "-o", out], check=True)
    return out


def _run(exe, strings):
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    text = "".join(s.encode("latin-1").hex() + "\n" for s in strings)
    r = subprocess.run([exe], input=text, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, \
        f"rc={r.returncode}\n{r.stderr[-4000:]}"
    rows = r.stdout.split("\n")[:-1]
    assert len(rows) == len(strings)
    return [(int(a), int(b, 16)) for a, b in (row.split() for row in rows)]


def test_corpus_has_the_required_cases():
    c = FC.corpus()
    assert 4500 <= len(c) <= 6000
    assert sum(len(s.replace(".", "").lstrip("0")) >= 768 for s in c) >= 50      # the 768-digit cases
    half_min = FC.exact_decimal(FC.Fraction(5e-324) / 2)
    assert half_min in c and float(half_min) == 0.0 and float(half_min + "0" * 300 + "1") == 5e-324
    top = FC.exact_decimal((FC.Fraction(1.7976931348623157e308) + FC.Fraction(2) ** 1024) / 2)
    assert top in c and float(top) == float("inf") and float(FC._lower_last(top)) == 1.7976931348623157e308
    for s in FC.SYNTAX_BAD:
        assert FC.expected(s)[0] == 0, s
    for s in FC.SYNTAX_OK:
        assert FC.expected(s)[0] == 1, s
    assert float("-444e-400") == 0.0 and FC.float_bits(float("-444e-400")) == 1 << 63
    assert float("0." + "0" * 400 + "1e401") == 1.0 and float("1" + "0" * 3000 + "e-3000") == 1.0
    assert float("2.4703282292062327e-324") == 0.0 and float("2.4703282292062328e-324") == 5e-324


def test_header_equals_float_under_asan_ubsan(exe):
    c = FC.corpus()
    got = _run(exe, c)
    bad = [(s[:60], len(s), g, FC.expected(s)) for s, g in zip(c, got) if g != FC.expected(s)]
    assert not bad, f"{len(bad)} of {len(c)} differ from float(): {bad[:5]}"


def test_high_byte_is_class_2(exe):
    assert _run(exe, ["1.5\xe9", "\xa01.5", "1.5"]) == [(2, 0), (2, 0), (1, FC.float_bits(1.5))]
