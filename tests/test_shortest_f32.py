"""CPU test of Rust's `{}` for an f32 (oarfish_amd/csrc/oem_shortest_f32.h): the header's pure functions -- the ones
the kernels of oem_count_matrix_text.hip call -- are compiled into a stand-alone host program with the address and
undefined-behaviour sanitizers on (tests/native/shortest_f32_main.cpp) and held to `writers.rust_display(x, f32=True)`,
the formatting of the existing `.count.mtx` writer.  The program gives each text a heap block of exactly the measured
length, so a printer that writes one byte more than it measured is a sanitizer report.  Its `--sweep` mode checks,
without any reference, that every text reads back as the same bits, is shortest, and respects the header's bound."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oarfish_amd.writers import rust_display

from .shortest_f32_common import (as_f32, em_counts, eighths, exponent_grid, integers, powers_of_ten_neighbours,
                                   random_bit_patterns, specials_and_negatives, subnormal_ladder)

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "shortest_f32_main.cpp")
EXE = os.path.join(HERE, "native", "shortest_f32_main")
CSRC = os.path.join(HERE, "..", "oarfish_amd", "csrc")
HDRS = [os.path.join(CSRC, "oem_shortest_f32.h"), os.path.join(CSRC, "oem_text_format.h")]
SWEEP_STRIDE = 997                                    # prime: 2 145 532 of the 2 139 095 039 positive finite patterns


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-o", EXE, SRC])
    return EXE


def check_bits(exe, bits):
    """Every pattern's text is rust_display's, and the measured length is the text's."""
    bits = np.asarray(bits, dtype=np.uint32)
    r = subprocess.run([exe], input="".join(f"{int(b):x}\n" for b in bits), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout.split("\n")
    assert out[-1] == "" and len(out) == len(bits) + 1
    for b, x, ln in zip(bits, as_f32(bits), out[:-1]):
        text, n = ln.rsplit(" ", 1)
        assert text == rust_display(x, f32=True), (hex(int(b)), text)
        assert int(n) == len(text), (hex(int(b)), text, n)


def check_values(exe, values):
    check_bits(exe, np.asarray(values, dtype=np.float32).view(np.uint32))


def test_every_exponent(exe):
    grid = exponent_grid()
    assert len(grid) == 255 * 6 - 1
    check_bits(exe, grid)


def test_subnormals(exe):
    bits = subnormal_ladder()
    assert len(bits) == 23 + 1000
    check_bits(exe, bits)


def test_around_the_powers_of_ten(exe):
    bits = powers_of_ten_neighbours()
    assert len(bits) > 5 * 80
    check_bits(exe, bits)


def test_integers_and_eighths(exe):
    assert len(integers()) == 70_000 and len(eighths()) == 4096
    check_values(exe, integers())
    check_values(exe, eighths())


def test_counts_of_the_em(exe):
    x = em_counts()
    assert len(x) == 100_000 and x.min() > 1e-6 and x.max() < 5e4
    check_values(exe, x)


def test_random_bit_patterns(exe):
    bits = random_bit_patterns()
    assert len(bits) == 100_000
    check_bits(exe, bits)


def test_specials_and_negatives(exe):
    bits = specials_and_negatives()
    assert len(bits) == 14
    check_bits(exe, bits)
    r = subprocess.run([exe], input="".join(f"{b:x}\n" for b in bits[:7]), capture_output=True, text=True)
    assert r.stdout.split("\n")[:7] == ["0 1", "-0 2", "inf 3", "-inf 4", "NaN 3", "NaN 3", "NaN 3"]
    # large values are their shortest digits and zeros, never the exact integer
    r = subprocess.run([exe], input="7149f2ca\n", capture_output=True, text=True)      # 1e30f32
    assert r.stdout == "1" + "0" * 30 + " 31\n"


def test_self_checks_over_a_strided_sweep(exe):
    """strtof reads every text back; at most 9 digits; one digit fewer never reads back; the longest text is the
    header's bound (and, with this compiler's <charconv>, the digits are std::to_chars')."""
    r = subprocess.run([exe, "--sweep", str(SWEEP_STRIDE)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    f = r.stdout.split()
    assert f[0] == "checked" and int(f[1]) > 2_000_000, r.stdout
    # the bound the header states, less the sign: the kernels size their LDS stage by it
    hdr = open(HDRS[0]).read()
    assert "constexpr uint32_t kShortestF32MaxLen = 1 + 2 + 45;" in hdr and int(f[3]) == 47


def test_table_is_the_generated_one():
    gen = os.path.join(HERE, "..", "scripts", "gen_shortest_f32_table.py")
    assert subprocess.run([sys.executable, gen, "--check"]).returncode == 0
