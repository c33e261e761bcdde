"""Value sets shared by tests/test_shortest_f64.py (the host build of oem_shortest_f64.h) and
tests/test_quant_text_gpu.py (its device build): both builds see literally the same arrays."""
import numpy as np

LONGEST = 0x8000000000000001          # -5e-324: `-0.`, 323 zeros, `5` -- the 327 bytes of kShortestF64MaxLen


def as_f64(bits) -> np.ndarray:
    return np.asarray(bits, dtype=np.uint64).view(np.float64)


def bits_of(values) -> np.ndarray:
    return np.asarray(values, dtype=np.float64).view(np.uint64)


def edge_bits() -> np.ndarray:
    """Finite bit patterns: every power of two and every power of ten in range, each with its two neighbours; the
    subnormal edge (5e-324, the largest subnormal, the smallest normal); DBL_MAX; 2^53 - 1, 2^53, 2^53 + 2 and what
    9007199254740993 reads as; 0.1 + 0.2; 1e21, 1e22, 1e23; both zeros; and the negative of every tenth of them."""
    top = 0x7FF0000000000000
    bits = []
    for e in range(-1074, 1024):
        b = int(bits_of([np.ldexp(1.0, e)])[0])
        bits += [b - 1, b, b + 1]
    for k in range(-323, 309):
        b = int(bits_of([float(f"1e{k}")])[0])
        bits += [b - 1, b, b + 1]
    bits += [1, 0x000FFFFFFFFFFFFF, 0x0010000000000000, top - 1]
    bits += [int(b) for b in bits_of([2.0 ** 53 - 1, 2.0 ** 53, 2.0 ** 53 + 2, float("9007199254740993"), 0.1 + 0.2,
                                      1e21, 1e22, 1e23, 1.0, 0.1, 0.5, 123.456])]
    bits = [b for b in bits if 0 < b < top]
    bits += [b | (1 << 63) for b in bits[::10]]
    bits += [0, 1 << 63, LONGEST]
    return np.array(bits, dtype=np.uint64)


def seeded_bits() -> np.ndarray:
    """10^5 finite bit patterns: 50 000 random ones, then counts as an EM leaves them -- 40 000 log-uniform in
    (1e-12, 5e6), the integers 1 .. 5000 and the eighths 1/8 .. 625."""
    rng = np.random.default_rng(20250119)
    raw = rng.integers(0, 1 << 64, 60_000, dtype=np.uint64)
    raw = raw[(raw & np.uint64(0x7FF0000000000000)) != np.uint64(0x7FF0000000000000)][:50_000]
    em = np.concatenate([np.exp(rng.uniform(np.log(1e-12), np.log(5e6), 40_000)), np.arange(1, 5001, dtype=np.float64),
                         np.arange(1, 5001) / 8.0])
    return np.concatenate([raw, bits_of(em)])
