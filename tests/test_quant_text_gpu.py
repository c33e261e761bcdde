"""GPU tests of oem_quant_text and oem_ambig_text: `.quant` and `.ambig_info.tsv` formatted on the device.

The reference is existing code: every case compares the device bytes with the files `writers.write_output` writes for
the same columns (the host writer, pinned by tests/test_writers.py), byte for byte.  One set of 1000 transcripts is
written once by that writer; every case takes a prefix of its lines.  The cases with knobs run in the test-only
library, where OEM_QUANT_BUF_BYTES cuts the transcripts into chunks and OEM_QUANT_GRID_BLOCKS makes a workgroup walk
several tiles; its hook oem_debug_quant_last_call says how many chunks a call took and how many workgroup tiles went
through the LDS stage or were written directly.

The columns (see `columns`): lines 0 .. 255, the first workgroup at the defaults, have short names and short counts
around the longest text an f64 has (327 bytes, next to a `0`), and fit the stage; lines 256 .. 511 have 300-byte names
and overflow it; the rest draw their counts from the edge list of tests/test_shortest_f64.py.

The 10^5 seeded values tests/test_shortest_f64.py holds the host build of oem_shortest_f64.h to
(shortest_f64_common.seeded_bits) run through the device build too, next to 10^5 seeded (unique, total) pairs for
`.ambig_info.tsv` (the `seeded` fixture: one call of the host writer makes both references)."""
import ctypes as C
import os

import numpy as np
import pytest

from oarfish_amd import _lib, synth, writers

from .shortest_f64_common import LONGEST, as_f64, edge_bits, seeded_bits

pytestmark = pytest.mark.gpu

N = 1000
SIZES = [0, 1, 2, 255, 256, 257, 1000]
NAME_LENS = (0, 1, 15, 16, 17, 300)
LENS = (0, 9, 10, 2 ** 32, 2 ** 64 - 1, 1234)
MAX_TAIL = 1 + 20 + 1 + 327 + 1            # what follows a name at its longest: the greatest line is the name and this
STAGE_LINES = 32 * 1024 - 15               # bytes of lines a workgroup's stage holds
AMBIG_MAX_LINE = 33
QUANT_HEADER = b"tname\tlen\tnum_reads\n"
AMBIG_HEADER = b"unique_reads\tambig_reads\ttotal_reads\n"


def columns():
    edges = as_f64(edge_bits())
    rng = np.random.default_rng(20250120)
    short = np.concatenate([[0.0, 1.0, 0.1, 0.1 + 0.2, 2.0 ** 53, 1e21, 123.456, -2.5],
                            np.exp(rng.uniform(np.log(1e-9), np.log(5e6), 248))])
    counts = np.concatenate([short, edges[rng.integers(0, len(edges), N - 256)]])
    counts[100] = as_f64([LONGEST])[0]              # the longest text ...
    counts[99] = counts[101] = 0.0                  # ... between two `0`
    counts[5] = 5e-324
    counts[6] = np.finfo(np.float64).max
    name_len = [NAME_LENS[i % 5] for i in range(256)] + [300] * 256 + [NAME_LENS[i % 6] for i in range(N - 512)]
    name_len[100] = 300                             # and a long name on the longest line
    names = ["".join(chr(65 + (i + k) % 58) for k in range(l)) for i, l in enumerate(name_len)]
    lens = [LENS[i % len(LENS)] for i in range(N)]
    unique = rng.integers(0, 5000, N).astype(np.uint32)
    total = (unique + rng.integers(0, 100_000, N)).astype(np.uint32)
    unique[:8] = [0, 7, 2 ** 32 - 1, 10, 0, 2 ** 32 - 1, 999_999_999, 1_000_000_000]
    total[:8] = [0, 3, 5, 9, 2 ** 32 - 1, 2 ** 32 - 1, 1_000_000_000, 999_999_999]   # unique > total: ambig is 0
    return names, lens, counts, unique, total


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """The columns and what the host writer makes of them: the lines of the two bodies (without their newlines)."""
    names, lens, counts, unique, total = columns()
    out = str(tmp_path_factory.mktemp("ref") / "ref")
    writers.write_output(out, {}, names, lens, counts, unique, total)
    q = open(out + ".quant", "rb").read()
    a = open(out + ".ambig_info.tsv", "rb").read()
    assert q.startswith(QUANT_HEADER) and a.startswith(AMBIG_HEADER)
    ql, al = q[len(QUANT_HEADER):].split(b"\n"), a[len(AMBIG_HEADER):].split(b"\n")
    assert len(ql) == N + 1 and len(al) == N + 1 and ql[-1] == b"" and al[-1] == b""
    return dict(names=names, lens=lens, counts=counts, unique=unique, total=total, quant=ql[:-1], ambig=al[:-1])


def body_of(lines):
    return b"".join(l + b"\n" for l in lines)


def last_call():
    out = (C.c_double * 6)()
    assert _lib.testing_lib().oem_debug_quant_last_call(out) == _lib.OEM_OK
    return dict(chunks=int(out[0]), staged=int(out[1]), direct=int(out[2]))


def check(res, prefix, lines):
    """The text is the prefix and the lines; line_off are the offsets of the newline-split body."""
    got, want = res.text.tobytes(), prefix + body_of(lines)
    if got != want:
        gl, wl = got[len(prefix):].split(b"\n"), lines
        bad = next((i for i, (x, y) in enumerate(zip(gl, wl)) if x != y), min(len(gl), len(wl)))
        pytest.fail(f"line {bad}: device {gl[bad:bad + 1]!r}, writer {wl[bad:bad + 1]!r} ({len(got)} / {len(want)} bytes)")
    assert len(res.line_off) == len(lines) + 1 and res.line_off[0] == 0
    assert np.array_equal(res.line_off[1:].astype(np.int64), np.cumsum([len(l) + 1 for l in lines], dtype=np.int64))
    nl = np.flatnonzero(res.text[len(prefix):] == 10)
    assert np.array_equal(nl + 1, res.line_off[1:].astype(np.int64))          # every line ends where the next begins
    assert len(res.kept) == len(lines) and (res.kept == 1).all()
    assert res.content_bytes == len(res.text)


def quant(case, n, prefix=b""):
    return writers.quant_text_lines(case["names"][:n], case["lens"][:n], case["counts"][:n], prefix=prefix)


def ambig(case, n, prefix=b""):
    return writers.ambig_text_lines(case["unique"][:n], case["total"][:n], prefix=prefix)


def planned_chunks(bounds, cap):
    """The chunks the library cuts: consecutive lines whose greatest lengths together fit `cap`, one line at the least.
    Returns (number of chunks, whether a chunk ended because the next line would have straddled the buffer's end --
    its greatest length beginning inside the buffer and ending outside -- and not on the buffer's last byte)."""
    chunks, acc, start, straddled = 1, 0, 0, False
    for i, b in enumerate(bounds):
        if i > start and acc + b > cap:
            straddled |= acc < cap
            chunks, acc, start = chunks + 1, 0, i
        acc += b
    return chunks, straddled


def test_the_reference_lines_hold_what_the_cases_need(case):
    q = case["quant"]
    assert q[100].endswith(b"\t-0." + b"0" * 323 + b"5") and len(q[100]) == 300 + 1 + len(str(case["lens"][100])) + 1 + 327
    assert q[99].endswith(b"\t0") and q[101].endswith(b"\t0")
    assert {len(l.split(b"\t")[0]) for l in q} == set(NAME_LENS)
    assert {int(l.split(b"\t")[1]) for l in q} == set(LENS)
    first, second = sum(len(l) + 1 for l in q[:256]), sum(len(l) + 1 for l in q[256:512])
    assert first <= STAGE_LINES < second                  # the first workgroup stages its lines, the second cannot
    a = case["ambig"]
    assert a[1] == b"7\t0\t3" and a[2] == b"4294967295\t0\t5" and a[4] == b"0\t4294967295\t4294967295"
    assert a[5] == b"4294967295\t0\t4294967295" and a[6] == b"999999999\t1\t1000000000"


@pytest.mark.parametrize("n", SIZES)
def test_quant_text_equals_the_host_writer(case, n):
    check(quant(case, n), b"", case["quant"][:n])
    check(quant(case, n, QUANT_HEADER), QUANT_HEADER, case["quant"][:n])
    assert writers.quant_text(case["names"][:n], case["lens"][:n], case["counts"][:n]) == QUANT_HEADER + body_of(case["quant"][:n])


@pytest.mark.parametrize("n", SIZES)
def test_ambig_text_equals_the_host_writer(case, n):
    check(ambig(case, n), b"", case["ambig"][:n])
    assert writers.ambig_text(case["unique"][:n], case["total"][:n]) == AMBIG_HEADER + body_of(case["ambig"][:n])


def test_staged_and_direct_workgroups(case):
    """At the defaults 1000 lines are one chunk of four workgroup tiles: the first fits the LDS stage, the second (300
    byte names) does not and is written directly."""
    with _lib.testing():
        check(quant(case, 512), b"", case["quant"][:512])
        assert last_call() == dict(chunks=1, staged=1, direct=1)
        check(quant(case, N), b"", case["quant"])
        got = last_call()
        assert got["chunks"] == 1 and got["staged"] >= 1 and got["direct"] >= 1 and got["staged"] + got["direct"] == 4
        check(ambig(case, N), b"", case["ambig"])
        assert last_call() == dict(chunks=1, staged=4, direct=0)


@pytest.mark.parametrize("n", [257, 1000])
def test_chunks_and_workgroup_rounds(case, n, monkeypatch):
    """Two workgroups walk the tiles, and the text buffer is cut so that the lines take at least three chunks and a
    line's greatest length straddles the end of a buffer (it opens the next chunk): the same bytes and offsets.  Up to
    257 lines also with the smallest buffer (anything below one line counts as one line: a chunk per line)."""
    bounds = [len(x.encode()) + MAX_TAIL for x in case["names"][:n]]
    monkeypatch.setenv("OEM_QUANT_GRID_BLOCKS", "2")
    for buf in [sum(bounds) // 4 + 7] + ([sum(bounds) // 7 + 3, 1] if n <= 257 else [100_000]):
        want_chunks, straddled = planned_chunks(bounds, buf)
        assert want_chunks >= 3 and (straddled or buf == 1)
        monkeypatch.setenv("OEM_QUANT_BUF_BYTES", str(buf))
        with _lib.testing():
            check(quant(case, n, b"#" * 5), b"#" * 5, case["quant"][:n])
            got = last_call()
        assert got["chunks"] == want_chunks, buf
        if n == 1000 and buf == 100_000:
            assert got["staged"] >= 1 and got["direct"] >= 1
    for buf in (AMBIG_MAX_LINE * (n // 3) + 5, AMBIG_MAX_LINE * 100):
        monkeypatch.setenv("OEM_QUANT_BUF_BYTES", str(buf))
        with _lib.testing():
            check(ambig(case, n), b"", case["ambig"][:n])
            assert last_call()["chunks"] == -(-n // (buf // AMBIG_MAX_LINE)) >= 3


@pytest.mark.parametrize("plen", [0, 1, 15, 16, 17])
def test_body_start_alignment(case, plen, monkeypatch):
    """The device text starts at the residue of prefix_len modulo 16 in its (256-byte aligned) buffer, so these five
    prefixes start the body -- and with it every workgroup's range -- in every class the head and tail stores of
    k_lines_emit have: aligned, one byte above, one byte below, and the same one word further.  Whole and in chunks."""
    prefix = bytes(35 + (i % 60) for i in range(plen))
    for n in (1, 257, 600):
        check(quant(case, n, prefix), prefix, case["quant"][:n])
        check(ambig(case, n, prefix), prefix, case["ambig"][:n])
    monkeypatch.setenv("OEM_QUANT_BUF_BYTES", "60000")
    monkeypatch.setenv("OEM_QUANT_GRID_BLOCKS", "1")
    with _lib.testing():
        check(quant(case, 600, prefix), prefix, case["quant"][:600])
        assert last_call()["chunks"] >= 3


def test_every_workgroup_start_alignment(case):
    """A first name of 0 .. 15 bytes moves the start of the second workgroup's range through all sixteen alignments
    (asserted on the offsets)."""
    seen = set()
    assert case["quant"][0].startswith(b"\t")              # the first name is empty
    for k in range(16):
        names = ["x" * k] + case["names"][1:300]
        res = writers.quant_text_lines(names, case["lens"][:300], case["counts"][:300])
        check(res, b"", [b"x" * k + case["quant"][0]] + case["quant"][1:300])
        seen.add(int(res.line_off[256]) % 16)
    assert seen == set(range(16))


def test_edge_list_on_the_device(case, tmp_path):
    """The device build of oem_shortest_f64.h against the writer on the whole edge list tests/test_shortest_f64.py
    holds the host build to."""
    counts = as_f64(edge_bits())
    n = len(counts)
    names = [f"t{i}" for i in range(n)]
    lens = [i * 7919 for i in range(n)]
    out = str(tmp_path / "edges")
    writers.write_output(out, {}, names, lens, counts, np.zeros(n, np.uint32), np.zeros(n, np.uint32))
    want = open(out + ".quant", "rb").read()
    assert writers.quant_text(names, lens, counts) == want


def test_end_to_end_files(tmp_path):
    """A small synthetic store, the EM, then the host writer and the device writer on the same counts: three
    identical files; and the bulk driver with quant_on_device writes what write_output writes of its counts."""
    from oarfish_amd.em import em as run_em
    from oarfish_amd.bulk import BulkArgs, perform_inference_and_write_output
    from oarfish_amd.types import EMInfo, InMemoryAlignmentStore, TranscriptInfo

    st = synth.make_store(20_000, 700, seed=91)
    store = InMemoryAlignmentStore.from_arrays(st.row_ptr, st.tid, st.as_prob)
    names = [f"ENST{i:011d}.{i % 13}" for i in range(st.n_txps)]
    lens = (200 + np.arange(st.n_txps) * 37 % 9000).tolist()
    emi = EMInfo(eq_map=store, txp_info=[TranscriptInfo.with_len(int(l)) for l in lens])
    counts = run_em(emi, 3)
    aux = store.device_store(st.n_txps, 0).aux_counts()
    info = {"num_aligned_reads": st.n_reads, "nested": {"a": [1, 2]}}
    a, b = str(tmp_path / "host" / "out"), str(tmp_path / "device" / "out")
    writers.write_output(a, info, names, lens, counts, *aux)
    writers.write_output_device(b, info, names, lens, counts, aux)
    assert sorted(os.listdir(tmp_path / "host")) == sorted(os.listdir(tmp_path / "device"))
    for ext in (".meta_info.json", ".quant", ".ambig_info.tsv"):
        assert open(a + ext, "rb").read() == open(b + ext, "rb").read(), ext
    assert open(b + ".quant", "rb").read().count(b"\n") == st.n_txps + 1

    out = str(tmp_path / "bulk" / "sample")
    got = perform_inference_and_write_output(store, names, lens, BulkArgs(output=out, quant_on_device=True))
    want = str(tmp_path / "bulk_want" / "sample")
    writers.write_output(want, {}, names, lens, got, *aux)
    for ext in (".quant", ".ambig_info.tsv"):
        assert open(out + ext, "rb").read() == open(want + ext, "rb").read(), ext
    assert os.path.exists(out + ".meta_info.json")


# -- the host build's 10^5 seeded values, and 10^5 seeded pairs ---------------------------------------------------------
def ambig_pairs(n=100_000):
    """(unique, total): the first half uniform over all u32; the second half drawn from the values within 2 of a
    power of ten, 10^0 .. 10^9 (every digit-count edge of all three columns; unique > total saturates to 0)."""
    rng = np.random.default_rng(20250121)
    near = np.array(sorted({10 ** k + o for k in range(10) for o in range(-2, 3)} - {-1}), dtype=np.uint32)
    assert len(near) == 49 and near[0] == 0 and near[-1] == 1_000_000_002
    half = n // 2
    unique = np.concatenate([rng.integers(0, 1 << 32, half, dtype=np.uint64), near[rng.integers(0, len(near), n - half)]])
    total = np.concatenate([rng.integers(0, 1 << 32, half, dtype=np.uint64), near[rng.integers(0, len(near), n - half)]])
    unique[half:half + len(near)] = near                          # every one of them at least once in each column,
    total[half:half + len(near)] = near[::-1]
    unique[half + len(near):half + 2 * len(near)] = near[::-1]    # and as the difference's neighbour on either side
    total[half + len(near):half + 2 * len(near)] = near
    return unique.astype(np.uint32), total.astype(np.uint32)


@pytest.fixture(scope="module")
def seeded(tmp_path_factory):
    counts = as_f64(seeded_bits())
    n = len(counts)
    assert n == 100_000
    names = [f"t{i % 10}" if i % 3 else "" for i in range(n)]
    lens = list(range(n))
    unique, total = ambig_pairs(n)
    out = str(tmp_path_factory.mktemp("seeded") / "ref")
    writers.write_output(out, {}, names, lens, counts, unique, total)
    q = open(out + ".quant", "rb").read()[len(QUANT_HEADER):].split(b"\n")
    a = open(out + ".ambig_info.tsv", "rb").read()[len(AMBIG_HEADER):].split(b"\n")
    assert len(q) == n + 1 and len(a) == n + 1
    return dict(names=names, lens=lens, counts=counts, unique=unique, total=total, quant=q[:-1], ambig=a[:-1])


def test_seeded_values_on_the_device(seeded):
    """50 000 random finite patterns, 40 000 log-uniform, 5 000 integers, 5 000 eighths: every count field is
    `rust_display(x)`, the text and line_off are the host writer's.  The random patterns average well over 128 bytes
    a line (a tile of 256 overflows the 32 KiB stage), the EM-shaped counts under 20, so the call takes both the
    LDS-staged path and the direct one."""
    s = seeded
    res = quant(s, len(s["counts"]))
    check(res, b"", s["quant"])
    got = res.text.tobytes().split(b"\n")[:-1]
    for i, (x, line) in enumerate(zip(s["counts"], got)):
        assert line.rsplit(b"\t", 1)[1] == writers.rust_display(x).encode(), (i, hex(int(s["counts"].view(np.uint64)[i])), line)
    with _lib.testing():
        again = quant(s, len(s["counts"]))
        path = last_call()
    assert again.text.tobytes() == res.text.tobytes() and np.array_equal(again.line_off, res.line_off)
    assert path["chunks"] == 1 and path["staged"] >= 1 and path["direct"] >= 1
    assert path["staged"] + path["direct"] == -(-len(got) // 256)


def test_seeded_values_in_chunks(seeded, monkeypatch):
    """The same 10^5 lines cut into four or more chunks, 64 workgroups walking each chunk's tiles."""
    s = seeded
    bounds = [len(x) + MAX_TAIL for x in s["names"]]
    buf = sum(bounds) // 4 + 7
    want_chunks, _ = planned_chunks(bounds, buf)
    assert want_chunks >= 4
    monkeypatch.setenv("OEM_QUANT_BUF_BYTES", str(buf))
    monkeypatch.setenv("OEM_QUANT_GRID_BLOCKS", "64")
    with _lib.testing():
        check(quant(s, len(bounds), QUANT_HEADER), QUANT_HEADER, s["quant"])
        path = last_call()
    assert path["chunks"] == want_chunks and path["staged"] >= 1 and path["direct"] >= 1


def test_seeded_pairs_on_the_device(seeded, monkeypatch):
    """10^5 (unique, total) pairs against the host writer's lines: whole, and in three or more chunks."""
    s = seeded
    n = len(s["unique"])
    u, t = s["unique"].astype(np.int64), s["total"].astype(np.int64)
    assert (u[: n // 2] > 10 ** 9).sum() > 1000 and (u > t).sum() > 1000 and (u == t).sum() > 100
    assert s["ambig"][n // 2] == b"0\t1000000002\t1000000002" and s["ambig"][n // 2 + 48] == b"1000000002\t0\t0"
    check(ambig(s, n), b"", s["ambig"])
    buf = AMBIG_MAX_LINE * (n // 3) + 5
    monkeypatch.setenv("OEM_QUANT_BUF_BYTES", str(buf))
    with _lib.testing():
        check(ambig(s, n, AMBIG_HEADER), AMBIG_HEADER, s["ambig"])
        assert last_call()["chunks"] == -(-n // (buf // AMBIG_MAX_LINE)) >= 3
