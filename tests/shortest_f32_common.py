"""Value sets shared by tests/test_shortest_f32.py (the host build of oem_shortest_f32.h) and
tests/test_count_matrix_text_gpu.py (its device build): both builds see literally the same arrays."""
import numpy as np

GRID_MANTISSAS = (0, 1, 2, 0x400000, 0x7FFFFE, 0x7FFFFF)


def exponent_grid() -> np.ndarray:
    """Bit patterns: every binary exponent 0 .. 254 x GRID_MANTISSAS, without +0 (1 529 values)."""
    bits = [(e << 23) | m for e in range(255) for m in GRID_MANTISSAS]
    return np.array([b for b in bits if b], dtype=np.uint32)


def as_f32(bits) -> np.ndarray:
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def bits_of_f32(values) -> np.ndarray:
    """The patterns of the values rounded to f32."""
    return np.asarray(values, dtype=np.float32).view(np.uint32)


def subnormal_ladder() -> np.ndarray:
    """Bit patterns: every power of two below FLT_MIN, and the 1000 least subnormals."""
    return np.array([1 << k for k in range(23)] + list(range(1, 1001)), dtype=np.uint32)


def powers_of_ten_neighbours() -> np.ndarray:
    """Bit patterns: what 1e-45 .. 1e38 read as, each with its two neighbours on either side (positive and finite)."""
    bits = []
    for k in range(-45, 39):
        b = int(np.array([float(f"1e{k}")], dtype=np.float64).astype(np.float32).view(np.uint32)[0])
        bits += [v for v in range(b - 2, b + 3) if 0 < v < 0x7F800000]
    return np.array(bits, dtype=np.uint32)


def integers() -> np.ndarray:
    """Values: 1 .. 70 000."""
    return np.arange(1, 70_001)


def eighths() -> np.ndarray:
    """Values: 1/8 .. 512 in steps of 1/8."""
    return np.arange(1, 4097) / 8.0


def em_counts() -> np.ndarray:
    """Values (f64, to be rounded to f32): 100 000 log-uniform counts in (1e-6, 5e4), as an EM leaves them."""
    rng = np.random.default_rng(20250117)
    return np.exp(rng.uniform(np.log(1e-6), np.log(5e4), 100_000))


def random_bit_patterns() -> np.ndarray:
    """100 000 random bit patterns, NaNs and infinities as drawn."""
    rng = np.random.default_rng(20250118)
    return rng.integers(0, 1 << 32, 100_000, dtype=np.uint64).astype(np.uint32)


SPECIALS = (0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001)


def specials_and_negatives() -> list:
    """Bit patterns: the zeros, the infinities, three NaNs (SPECIALS), then seven negatives."""
    return list(SPECIALS) + [0x80000000 | int(b) for b in (0x3F800000, 0x3DCCCCCD, 0x00000001, 0x7F7FFFFF, 0x4B800000,
                                                           0x00800000, 0x501502F9)]
