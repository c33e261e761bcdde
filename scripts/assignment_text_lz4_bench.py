#!/usr/bin/env python3
"""Times `.prob.lz4` made on the device against the uncompressed call, at the bench store (C3 shape: 10 M reads, 80 M
alignments), read names of 36 bytes, display_thresh 1e-6, counts from a short EM run, the file's header lines as prefix:

  (a) oem_assignment_text      end to end (the uncompressed call: the yardstick), best of two
  (b) oem_assignment_text_lz4  end to end, best of two; the calls alternate a, b, a, b
  (c) its kernels              measure / scan / emit / k_lz4_blocks / scan + k_lz4_gather from HIP events
                               (OEM_TEXT_TIMING, test-only library)
  (d) the frame's ratio        frame bytes / content bytes, and payload bytes / content bytes
  where a system liblz4 is found (ctypes):
  (e) host compression         LZ4F_compressFrame of the text (a) returns, at level 0 and at level 4: what a caller has
                               to add to (a) today
  (f) liblz4's fast ratio      LZ4_compress_default per independent 64 KiB block of the same content (a block that does
                               not shrink counted raw): the figure (d)'s payload ratio is judged against

The device frame is decoded by liblz4 and compared with prefix + text.  Writes
profiles/assignment_text_lz4_bench.json (or --out PATH) and prints it.

usage: assignment_text_lz4_bench.py [--out PATH] [--shape c3] [--no-hc]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oarfish_amd import _lib, synth  # noqa: E402
from oarfish_amd.types import DeviceStore, pack_read_names  # noqa: E402

THRESH = 1e-6
BLOCK = 65536


class FramePrefs(C.Structure):
    _fields_ = [("blockSizeID", C.c_int), ("blockMode", C.c_int), ("contentChecksumFlag", C.c_int),
                ("frameType", C.c_int), ("contentSize", C.c_ulonglong), ("dictID", C.c_uint),
                ("blockChecksumFlag", C.c_int), ("compressionLevel", C.c_int), ("autoFlush", C.c_uint),
                ("favorDecSpeed", C.c_uint), ("reserved", C.c_uint * 3)]


def system_lz4():
    try:
        L = C.CDLL("liblz4.so.1")
        L.LZ4F_compressFrameBound.argtypes = [C.c_size_t, C.c_void_p]
        L.LZ4F_compressFrameBound.restype = C.c_size_t
        L.LZ4F_compressFrame.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
        L.LZ4F_compressFrame.restype = C.c_size_t
        L.LZ4F_isError.argtypes = [C.c_size_t]
        L.LZ4_compress_default.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.LZ4_compressBound.argtypes = [C.c_int]
        L.LZ4F_createDecompressionContext.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
        L.LZ4F_createDecompressionContext.restype = C.c_size_t
        L.LZ4F_freeDecompressionContext.argtypes = [C.c_void_p]
        L.LZ4F_decompress.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p]
        L.LZ4F_decompress.restype = C.c_size_t
        L.LZ4_versionString.restype = C.c_char_p
        return L
    except (OSError, AttributeError):
        return None


def raw_call(d, counts, blob, off, prefix=None):
    """One C call by itself: the result stays in the library's buffer; returns (seconds, handle)."""
    L = d._lib
    h = C.c_void_p()
    t = time.perf_counter()
    if prefix is None:
        _lib.check(L.oem_assignment_text(d.handle, counts.ctypes.data, THRESH, blob.ctypes.data, off.ctypes.data, C.byref(h)))
    else:
        _lib.check(L.oem_assignment_text_lz4(d.handle, counts.ctypes.data, THRESH, blob.ctypes.data, off.ctypes.data,
                                             prefix.ctypes.data, len(prefix), C.byref(h)))
    return time.perf_counter() - t, h


def result_bytes(L, h):
    nb = C.c_uint64(0)
    L.oem_text_result_dims(h, C.byref(nb), None, None)
    out = np.empty(nb.value, dtype=np.uint8)
    _lib.check(L.oem_text_result_copy(h, out.ctypes.data, None, None))
    return out


def info(L, h, key):
    v = C.c_uint64(0)
    _lib.check(L.oem_text_result_info(h, key, C.byref(v)))
    return int(v.value)


def host_frame(Z, text, level):
    p = FramePrefs()
    p.blockSizeID, p.blockMode, p.contentChecksumFlag, p.contentSize, p.compressionLevel = 4, 0, 1, len(text), level
    cap = Z.LZ4F_compressFrameBound(len(text), C.byref(p))
    dst = np.empty(cap, dtype=np.uint8)
    t = time.perf_counter()
    n = Z.LZ4F_compressFrame(dst.ctypes.data, cap, text.ctypes.data, len(text), C.byref(p))
    dt = time.perf_counter() - t
    assert not Z.LZ4F_isError(n)
    return dt, int(n)


def host_decode(Z, frame, n_out):
    ctx = C.c_void_p()
    Z.LZ4F_createDecompressionContext(C.byref(ctx), 100)
    dst = np.empty(n_out + 64, dtype=np.uint8)
    s_at = d_at = 0
    while s_at < len(frame):
        s_n, d_n = C.c_size_t(len(frame) - s_at), C.c_size_t(len(dst) - d_at)
        hint = Z.LZ4F_decompress(ctx, dst.ctypes.data + d_at, C.byref(d_n), frame.ctypes.data + s_at, C.byref(s_n), None)
        assert not Z.LZ4F_isError(hint), "liblz4 refuses the device frame"
        s_at, d_at = s_at + s_n.value, d_at + d_n.value
        if hint == 0:
            break
    Z.LZ4F_freeDecompressionContext(ctx)
    return dst[:d_at]


def main():
    args = sys.argv[1:]
    out_path = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "assignment_text_lz4_bench.json")
    shape = args[args.index("--shape") + 1] if "--shape" in args else "c3"
    st = synth.make_config(shape)
    R = st.n_reads
    names = [f"{i:08x}-0000-4000-8000-{i * 2654435761 % 2 ** 48:012x}" for i in range(R)]   # 36 bytes, uuid-shaped
    blob, off = pack_read_names(names, R)
    del names
    prefix = np.frombuffer(f"{st.n_txps}\t{R}\n".encode() + "".join(f"ENST{i:011d}.1\n" for i in range(st.n_txps)).encode(),
                           dtype=np.uint8)
    rec = {"workload": "assignment_text_lz4", "shape": shape, "n_reads": R, "n_txps": st.n_txps, "nnz": int(len(st.tid)),
           "display_thresh": THRESH, "name_bytes": 36, "prefix_bytes": int(len(prefix))}
    with DeviceStore(st.row_ptr, st.tid, st.as_prob, None, st.n_txps) as d:
        L = d._lib
        counts, _ = d.em_run(None, 100, 1e-3, 50)
        for pre in (None, prefix):                       # first use outside the timed calls
            L.oem_text_result_destroy(raw_call(d, counts, blob, off, pre)[1])
        ta, tb, text, frame = [], [], None, None
        for i in range(2):
            dt, h = raw_call(d, counts, blob, off)
            ta.append(dt)
            if i == 1:
                text = result_bytes(L, h)
            L.oem_text_result_destroy(h)
            dt, h = raw_call(d, counts, blob, off, prefix)
            tb.append(dt)
            if i == 1:
                frame = result_bytes(L, h)
                rec["content_bytes"] = info(L, h, _lib.OEM_TEXT_INFO_CONTENT_BYTES)
                rec["blocks"] = info(L, h, _lib.OEM_TEXT_INFO_BLOCKS)
                rec["raw_blocks"] = info(L, h, _lib.OEM_TEXT_INFO_RAW_BLOCKS)
            L.oem_text_result_destroy(h)
    rec["a_text_s"] = [round(x, 4) for x in ta]
    rec["b_text_lz4_s"] = [round(x, 4) for x in tb]
    rec["b_over_a"] = round(min(tb) / min(ta), 3)
    rec["text_bytes"] = int(len(text))
    rec["frame_bytes"] = int(len(frame))
    rec["d_frame_ratio"] = round(len(frame) / rec["content_bytes"], 4)
    payload = len(frame) - 19 - 8 * rec["blocks"]
    rec["d_payload_ratio"] = round(payload / rec["content_bytes"], 4)
    # (c)
    with _lib.testing():
        os.environ["OEM_TEXT_TIMING"] = "1"
        try:
            with DeviceStore(st.row_ptr, st.tid, st.as_prob, None, st.n_txps) as dt_:
                ms3, ms2 = (C.c_float * 3)(), (C.c_float * 2)()
                stages = []
                for _ in range(2):
                    _, h = raw_call(dt_, counts, blob, off, prefix)
                    dt_._lib.oem_text_result_destroy(h)
                    _lib.lib().oem_debug_text_last_timing(ms3)
                    _lib.lib().oem_debug_text_lz4_last_timing(ms2)
                    stages.append([round(float(x), 3) for x in list(ms3) + list(ms2)])
        finally:
            del os.environ["OEM_TEXT_TIMING"]
    rec["c_kernel_ms_measure_scan_emit_lz4blocks_scangather"] = stages
    Z = system_lz4()
    rec["liblz4"] = Z.LZ4_versionString().decode() if Z else None
    if Z:
        content = np.concatenate([prefix, text])
        rec["device_frame_decodes_to_prefix_and_text"] = bool(np.array_equal(host_decode(Z, frame, len(content)), content))
        t0, n0 = host_frame(Z, text, 0)
        rec["e_host_level0_s"], rec["e_host_level0_ratio"] = round(t0, 3), round(n0 / len(text), 4)
        rec["e_a_plus_level0_s"] = round(min(ta) + t0, 3)
        if "--no-hc" not in args:
            t4, n4 = host_frame(Z, text, 4)
            rec["e_host_level4_s"], rec["e_host_level4_ratio"] = round(t4, 3), round(n4 / len(text), 4)
            rec["e_a_plus_level4_s"] = round(min(ta) + t4, 3)
        dst = np.empty(Z.LZ4_compressBound(BLOCK), dtype=np.uint8)
        total, worst, raw = 0, 0.0, 0
        for at in range(0, len(content), BLOCK):
            n = min(BLOCK, len(content) - at)
            c = Z.LZ4_compress_default(content.ctypes.data + at, dst.ctypes.data, n, len(dst))
            if c <= 0 or c >= n:
                c, raw = n, raw + 1
            total += c
            worst = max(worst, c / n)
        rec["f_liblz4_fast_block_payload_ratio"] = round(total / len(content), 4)
        rec["f_liblz4_fast_worst_block"] = round(worst, 4)
        rec["f_liblz4_fast_raw_blocks"] = raw
        rec["device_over_liblz4_fast"] = round(rec["d_payload_ratio"] / rec["f_liblz4_fast_block_payload_ratio"], 4)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)
    if Z and not rec["device_frame_decodes_to_prefix_and_text"]:
        sys.exit("the device frame does not decode to prefix + text")


if __name__ == "__main__":
    main()
