"""Shared by the span-walk tests (test_parse_walk_emu.py, test_parse_walk_gpu.py): the walk kernel's source built for the lane
emulator (tests/emu/walk_emu.cpp), the front-end corpus as MP4 samples (bare raw_data_blocks: the ADTS headers cut off, as
test_corpus.py and tests/js/test_aurora.js build them) and spans over those samples."""
import ctypes as C
import os
import subprocess

import numpy as np

import aacgpu
import emu_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPAN_SIZES = (1, 3, 7, 16, 40)          # blocks per span, cycled


def build_emu(out_dir):
    """tests/emu/walk_emu.cpp + the host's table builders, as tests/emu/Makefile builds the emulator, into out_dir."""
    lib = emu_lib.build_driver("walk_emu", ["tests/emu/walk_emu.cpp", "aac.js_amd/csrc/aacg_parse_host.cpp", "aac.js_amd/csrc/aacg_tables.cpp"], out_dir)
    lib.emu_walk_last_error.restype = C.c_char_p
    lib.emu_walk.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                             C.c_void_p, C.c_void_p]
    return lib


def emu_walk(lib, sample_index, data, spans, max_frames, options=aacgpu.PARSE_REFERENCE_QUIRKS):
    """The walk kernel's source on the CPU: the same outputs as aacgpu.Parser.walk."""
    entries, counts = aacgpu.standard_codebooks()
    data = np.ascontiguousarray(data, np.uint8)
    spans = np.ascontiguousarray(spans)
    assert spans.dtype == aacgpu.PARSE_FRAME_DTYPE
    frames = np.zeros((len(spans), max_frames), aacgpu.PARSE_FRAME_DTYPE)
    results = np.zeros(len(spans), aacgpu.WALK_RESULT_DTYPE)
    rc = lib.emu_walk(sample_index, entries.ctypes.data, counts.ctypes.data, data.ctypes.data, data.size, spans.ctypes.data, len(spans),
                      max_frames, options, frames.ctypes.data, results.ctypes.data)
    if rc:
        raise RuntimeError("emu_walk rc=%d: %s" % (rc, lib.emu_walk_last_error().decode()))
    return frames, results


def adts_table(data):
    out, off = [], 0
    while off + 7 <= len(data):
        assert data[off] == 0xFF and (data[off + 1] & 0xF0) == 0xF0
        length = ((int(data[off + 3]) & 3) << 11) | (int(data[off + 4]) << 3) | (int(data[off + 5]) >> 5)
        out.append((off, length))
        off += length
    return np.array(out, aacgpu.PARSE_FRAME_DTYPE)


def bare_blocks(data):
    """The stream's raw_data_blocks back to back (each ADTS header cut off: 7 bytes, 9 with a CRC) and their table in that buffer."""
    table = adts_table(data)
    hdr = np.array([7 if data[int(o) + 1] & 1 else 9 for o in table["byte_offset"]], np.uint32)
    pieces = [data[int(o) + int(h):int(o) + int(n)] for (o, n), h in zip(table, hdr)]
    out = np.zeros(len(pieces), aacgpu.PARSE_FRAME_DTYPE)
    out["byte_length"] = [len(p) for p in pieces]
    out["byte_offset"] = np.concatenate([[0], np.cumsum(out["byte_length"])[:-1]]).astype(np.uint32) if len(pieces) else []
    return (np.concatenate(pieces) if pieces else np.zeros(0, np.uint8)), out


def group(table, base=0, sizes=SPAN_SIZES, phase=0):
    """Spans over consecutive blocks of `table` (offsets + base), sizes cycled from `phase`: (spans, index of each span's first block)."""
    spans, firsts, k, i = [], [], 0, phase
    while k < len(table):
        n = min(sizes[i % len(sizes)], len(table) - k)
        start = int(table["byte_offset"][k])
        end = int(table["byte_offset"][k + n - 1]) + int(table["byte_length"][k + n - 1])
        spans.append((base + start, end - start))
        firsts.append(k)
        k += n
        i += 1
    return np.array(spans, aacgpu.PARSE_FRAME_DTYPE), firsts


def regenerate_corpus(out_dir, corpus):
    """tests/js/corpus_cases.js writes the corpus streams byte for byte (node, no GPU)."""
    r = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "corpus_cases.js"), str(out_dir)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return {e["name"]: np.fromfile(os.path.join(str(out_dir), e["name"] + ".aac"), np.uint8) for e in corpus}


def corpus_spans(streams, corpus):
    """Per sample-rate index: one buffer with every stream of that rate as bare blocks, the spans over it (SPAN_SIZES cycled,
    a different phase per stream), and per span (stream name, the table of the blocks it covers)."""
    groups = {}
    for j, e in enumerate(corpus):
        bare, table = bare_blocks(streams[e["name"]])
        g = groups.setdefault(e["si"], {"pieces": [], "size": 0, "spans": [], "cover": []})
        spans, firsts = group(table, g["size"], phase=j)
        for s, k in zip(spans, firsts):
            n = int(np.searchsorted(table["byte_offset"], int(s["byte_offset"]) - g["size"] + int(s["byte_length"])))
            cover = table[k:n].copy()
            cover["byte_offset"] += g["size"]
            g["spans"].append(s)
            g["cover"].append((e["name"], cover))
        g["pieces"].append(bare)
        g["size"] += len(bare)
    out = {}
    for si, g in groups.items():
        data = np.concatenate(g["pieces"] + [np.zeros(0, np.uint8)])
        out[si] = (data, np.array(g["spans"], aacgpu.PARSE_FRAME_DTYPE), g["cover"])
    return out
