"""What the two tiers of the sorting-names-session tests share (tests/test_records_stream_sort.py,
tests/test_records_stream_sort_gpu.py): the 16-record input of the names-session tests, permuted and with secondary
flags, and the sort rule of oarfish_amd/csrc/oem_collate.h in plain Python."""
import numpy as np

from tests.records_stream_names_common import INPUT16, U, records16

# the names-session input in this order: every read's records are scattered, and the secondaries of r5 (11, 13, 14), of
# read2 (5 before 3) and of ACGTACGTAC (9) come before or between their primaries (10, 2, 8)
PERM16 = [11, 6, 2, 15, 9, 0, 13, 5, 8, 1, 14, 3, 12, 7, 10, 4]
SECONDARY16 = {3, 5, 9, 11, 13, 14}          # by the record's index in INPUT16: every record of a read but its first


def sort_records16():
    """(records, (blob, offsets), secondary) of the permuted input"""
    rec, (blob, off) = records16()
    names = [INPUT16[p][1] for p in PERM16]
    o = np.zeros(len(names) + 1, dtype=np.uint64)
    np.cumsum([len(nm) for nm in names], out=o[1:])
    sec = np.array([1 if p in SECONDARY16 else 0 for p in PERM16], dtype=np.uint8)
    return np.ascontiguousarray(rec[PERM16]), (np.frombuffer(b"".join(names), dtype=np.uint8), o), sec


def names_list(names):
    blob, off = names
    return [bytes(blob[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]


def sort_rule(records, names, secondary=None):
    """(order, group_off): the surviving input indices by (name bytes, primary first, index), cut where the name changes"""
    nl = names_list(names)
    sec = np.zeros(len(records), dtype=np.uint8) if secondary is None else np.asarray(secondary)
    order = sorted((i for i in range(len(records)) if not records["flags"][i] & U), key=lambda i: (nl[i], bool(sec[i]), i))
    group_off = [p for p in range(len(order)) if p == 0 or nl[order[p]] != nl[order[p - 1]]] + [len(order)]
    return np.array(order, dtype=np.int64), np.array(group_off if order else [0], dtype=np.uint64)
