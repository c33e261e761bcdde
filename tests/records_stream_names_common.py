"""What the two tiers of the names-session tests share (tests/test_records_stream_names.py,
tests/test_records_stream_names_gpu.py): the 16-record input and its cuttings."""
import numpy as np

from oarfish_amd import _lib
from oarfish_amd.builder import ALN_RECORD

T = 3
U = _lib.REC_UNMAPPED
# reads of sizes 1, 3, 1, 2 and 4; unmapped records first, last, between two reads and inside a read; one unmapped
# record with an empty name (6), one with the name of the read it sits in (4), one inside a read under another name (12)
INPUT16 = [(U, b"zz"), (0, b"r1"), (0, b"read2"), (0, b"read2"), (U, b"read2"), (0, b"read2"), (U, b""), (0, b"r3"),
           (0, b"ACGTACGTAC"), (0, b"ACGTACGTAC"), (0, b"r5"), (0, b"r5"), (U, b"other"), (0, b"r5"), (0, b"r5"), (U, b"tail")]
SIZES16, HEADS16 = [1, 3, 1, 2, 4], [1, 2, 7, 8, 10]


def cuttings16():
    """every single cut (17), every pair of distinct cuts (136), one record per batch"""
    n = len(INPUT16)
    out = [(a,) for a in range(n + 1)]
    out += [(a, b) for a in range(n + 1) for b in range(a + 1, n + 1)]
    out.append(tuple(range(1, n)))
    return out


def records16():
    n = len(INPUT16)
    rec = np.zeros(n, dtype=ALN_RECORD)
    for i, (flags, _) in enumerate(INPUT16):
        if flags & U:
            rec[i] = (0xFFFFFFFF, 0, 0, 0, 0, 0, U, 0)
        else:   # a plain full-length alignment the default filters keep; two per read at most share a transcript
            rec[i] = (i % T, 10, 1500, 1400, 1000 - i, 1500, _lib.REC_HAS_SCORE, 0)
    names = [nm for _, nm in INPUT16]
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum([len(nm) for nm in names], out=off[1:])
    return rec, (np.frombuffer(b"".join(names), dtype=np.uint8), off)
