"""CPU test of the `.prob` file's number formatting (oarfish_amd/csrc/oem_text_format.h): the header's pure functions
-- the ones the device kernels of oem_assignment_text.hip call -- are compiled into a stand-alone host program with the
address and undefined-behaviour sanitizers on, and held to Python's `f"{x:.{d}f}"` (correctly rounded on the exact
binary value, ties to even: what Rust's `{:.d}` and glibc's `%.*f` print) at the ties and around them, and to `str` for
the unsigned decimals.  Every printer's measured length must be the length it emits: the program gives each printer a
buffer of exactly the measured size, so one byte more is a sanitizer report."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "text_format_main.cpp")
EXE = os.path.join(HERE, "native", "text_format_main")
HDR = os.path.join(HERE, "..", "oarfish_amd", "csrc", "oem_text_format.h")
DECIMALS = range(3, 10)


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-o", EXE, SRC])
    return EXE


def run(exe, requests):
    r = subprocess.run([exe], input="".join(requests), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout.split("\n")
    assert out[-1] == "" and len(out) == len(requests) + 1
    return [tuple(ln.rsplit(" ", 1)) for ln in out[:-1]]


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def check_floats(exe, values):
    cases = [(float(x), d) for x in values for d in DECIMALS]
    got = run(exe, [f"f {bits(x):x} {d}\n" for x, d in cases])
    for (x, d), (text, n) in zip(cases, got):
        assert text == f"{x:.{d}f}", (x.hex(), d, text)
        assert int(n) == len(text), (x.hex(), d, text, n)


def around(x):
    return [float(np.nextafter(x, -np.inf)), x, float(np.nextafter(x, np.inf))]


def test_ties_and_their_neighbours(exe):
    vals = []
    for k in range(0, 13):                               # 2^-k: an exact tie at d = k - 1 decimals (0.5 -> d = 0 only; 0.125 at
        vals += around(2.0 ** -k)                        # d = 2; 2^-4 .. 2^-10 tie inside 3 .. 9), both neighbours never tie
    for t in (0.5, 0.125, 0.0625, 0.375, 0.3125, 0.6875, 0.9375, 0.0009765625, 0.0029296875, 0.5625, 0.4375,
              0.001953125, 0.005859375, 2.5 * 2.0 ** -10, 1.5 * 2.0 ** -9):
        vals += around(t)                                # odd and even neighbours: ties go both ways
    for d in DECIMALS:                                   # decimal "ties" that are none in binary: 0.0005, 0.00000005 ...
        vals += around(5.0 * 10.0 ** -(d + 1)) + around(15.0 * 10.0 ** -(d + 1)) + around(1.0 - 5.0 * 10.0 ** -(d + 1))
    check_floats(exe, vals)
    # the ties really are ties, and go to even in both directions
    got = dict(zip(("0.0625", "0.1875", "0.4375", "0.5625"),
                   run(exe, [f"f {bits(x):x} 3\n" for x in (0.0625, 0.1875, 0.4375, 0.5625)])))
    assert [g[0] for g in got.values()] == ["0.062", "0.188", "0.438", "0.562"]


def test_edges(exe):
    vals = [1.0, float(np.nextafter(1.0, 0.0)), 0.0, -0.0, 5e-324, 1e-300, 2.2250738585072014e-308, -0.25, -1e-12,
            9.0, float(np.nextafter(9.0, 0.0)), 9.9995, 9.99949999, 10.0, 99.9999999995, 2.0 ** 20 - 2.0 ** -33,
            1048575.9999999995]
    vals += around(1e-9) + around(1e-6) + around(1e-3) + around(1e-12)
    check_floats(exe, vals)
    assert run(exe, [f"f {bits(float(np.nextafter(1.0, 0.0))):x} 3\n"])[0] == ("1.000", "5")
    assert run(exe, [f"f {bits(-0.0):x} 3\n"])[0] == ("-0.000", "6")
    for d in DECIMALS:                                   # Rust prints NaN as `NaN`, whatever its sign or payload
        for nan_bits in (0x7ff8000000000000, 0xfff8000000000000, 0x7ff0000000000001):
            assert run(exe, [f"f {nan_bits:x} {d}\n"])[0] == ("NaN", "3")


def test_random_doubles(exe):
    rng = np.random.default_rng(20240601)
    small = np.concatenate([rng.random(10_000), 10.0 ** -rng.uniform(0, 12, 10_000)])   # uniform, and log-uniform down to 1e-12
    assert small.min() >= 0.0 and small.max() <= 1.0 and len(small) == 20_000
    check_floats(exe, small)
    check_floats(exe, np.concatenate([2.0 ** rng.uniform(0, 20, 1_000), rng.uniform(1.0, 2.0 ** 20, 1_000)]))


def test_unsigned_decimals_at_every_power_of_ten(exe):
    for kind, top in (("u", 2 ** 32 - 1), ("U", 2 ** 64 - 1)):
        vals = {0, top, top - 1}
        p = 1
        while p <= top:
            vals |= {v for v in (p - 1, p, p + 1) if 0 <= v <= top}
            p *= 10
        vals = sorted(vals)
        assert len(vals) >= (30 if kind == "u" else 60)
        got = run(exe, [f"{kind} {v}\n" for v in vals])
        for v, (text, n) in zip(vals, got):
            assert text == str(v) and int(n) == len(text), (kind, v, text, n)


def test_decimals_follow_the_reference():
    """writers.prob_display_decimals is what the device call uses for d (write_function.rs:218-224)."""
    from oarfish_amd.writers import prob_display_decimals
    assert [prob_display_decimals(t) for t in (1e-6, 1e-3, 0.2, 1e-12, 0.0, -1.0, math.inf, math.nan)] == [6, 3, 3, 9, 9, 9, 9, 9]
