"""Value sets shared by tests/test_shortest_f32.py (the host build of oem_shortest_f32.h) and
tests/test_count_matrix_text_gpu.py (its device build)."""
import numpy as np

GRID_MANTISSAS = (0, 1, 2, 0x400000, 0x7FFFFE, 0x7FFFFF)


def exponent_grid() -> np.ndarray:
    """Bit patterns: every binary exponent 0 .. 254 x GRID_MANTISSAS, without +0 (1 529 values)."""
    bits = [(e << 23) | m for e in range(255) for m in GRID_MANTISSAS]
    return np.array([b for b in bits if b], dtype=np.uint32)


def as_f32(bits) -> np.ndarray:
    return np.asarray(bits, dtype=np.uint32).view(np.float32)
