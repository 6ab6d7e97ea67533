#!/usr/bin/env python3
"""Rate of the device front end (aacg_parse_frames) and of bytes -> PCM with both stages on the device.

    python tools/parse_rate.py [--frames 65536] [--steps 50] [--standin]
    python tools/parse_rate.py --walk [--spans 256] [--blocks-per-span 16]

--walk: the span walk (aacg_parse_walk_spans) instead: the frames as bare blocks back to back (MP4 samples), --spans runs of
--blocks-per-span blocks each; reports us per 4096 blocks, next to the frame parser on the same blocks.

Streams: the 600 stereo 48 kHz frames of tests/js/parse_cases.js (synthetic writer; the standard codebooks unless --standin),
repeated to --frames.  Timed with HIP events on the launch stream, inputs
resident in HBM.  Prints one JSON line."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aac.js_amd", "python"))
import aacgpu  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--standin", action="store_true")
    ap.add_argument("--uniform", action="store_true", help="only the frames within 10 %% of the median length (a constant-bit-rate stream)")
    ap.add_argument("--decode", action="store_true", help="also time parse + plan-reuse decode of the same batch")
    ap.add_argument("--walk", action="store_true", help="time the span walk (aacg_parse_walk_spans) instead")
    ap.add_argument("--spans", type=int, default=256)
    ap.add_argument("--blocks-per-span", type=int, default=16)
    a = ap.parse_args()
    import torch
    d = tempfile.mkdtemp()
    r = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "parse_cases.js"), d, "synthetic" if a.standin else "standard"],
                       capture_output=True, text=True)
    assert r.returncode == 0 and "SKIP" not in r.stdout, r.stdout + r.stderr
    entries = np.fromfile(os.path.join(d, "codebooks.entries"), aacgpu.CODE_ENTRY_DTYPE)
    counts = np.fromfile(os.path.join(d, "codebooks.counts"), np.uint32)
    data = np.fromfile(os.path.join(d, "stereo600.bytes"), np.uint8)
    frames = np.fromfile(os.path.join(d, "stereo600.frames"), aacgpu.PARSE_FRAME_DTYPE)
    if a.uniform:
        med = float(np.median(frames["byte_length"]))
        frames = frames[(frames["byte_length"] > 0.9 * med) & (frames["byte_length"] < 1.1 * med)]
    if a.walk:
        return walk_rate(a, entries, counts, data, frames)
    reps = (a.frames + len(frames) - 1) // len(frames)
    pad = (-len(data)) % 16
    one = np.concatenate([data, np.zeros(pad, np.uint8)])
    big = np.concatenate([np.tile(one, reps), np.zeros(32, np.uint8)])
    table = np.tile(frames, reps)
    table["byte_offset"] += np.repeat(np.arange(reps, dtype=np.uint32) * len(one), len(frames))
    table = table[:a.frames]
    n = len(table)
    dev = torch.device("cuda:0")
    t = lambda arr: torch.from_numpy(arr.view(np.uint8).reshape(-1)).to(dev)
    d_bytes, d_frames = t(big), t(table)
    d_units = torch.zeros(n * 64, dtype=torch.uint8, device=dev)
    d_q = torch.zeros(n * 2 * 1024, dtype=torch.int16, device=dev)
    d_meta = torch.zeros(n * 2 * 120, dtype=torch.int16, device=dev)
    d_res = torch.zeros(n * 8, dtype=torch.uint8, device=dev)
    p = aacgpu.Parser(entries, counts, sample_index=3)
    side = torch.cuda.Stream()                          # a real stream handle: 0 would select the parser's own stream
    stream = side.cuda_stream
    torch.cuda.synchronize()
    go = lambda: p.parse_device(d_bytes.data_ptr(), d_frames.data_ptr(), n, 1, 2, aacgpu.PARSE_REFERENCE_QUIRKS,
                                d_units.data_ptr(), d_q.data_ptr(), d_meta.data_ptr(), None, d_res.data_ptr(), stream)
    for _ in range(a.warmup):
        go()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(side)
    for _ in range(a.steps):
        go()
    e1.record(side)
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.steps
    res = d_res.cpu().numpy().view(aacgpu.PARSE_RESULT_DTYPE)
    assert not res["status"].any()
    in_bytes = int(table["byte_length"].sum())
    out = {"kernel": "aacg_parse_frames", "frames": n, "us_per_batch": ms * 1e3, "frames_per_s": n / (ms * 1e-3),
           "bytes_per_frame": in_bytes / n, "stream_GBps": in_bytes / (ms * 1e-3) / 1e9,
           "written_GBps": n * (2 * 2048 + 2 * 240 + 64 + 8) / (ms * 1e-3) / 1e9, "codebooks": "stand-in" if a.standin else "standard"}
    print(json.dumps(out))


def timed(go, stream, steps, warmup):
    import torch
    for _ in range(warmup):
        go()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(steps):
        go()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def walk_rate(a, entries, counts, data, frames):
    """--walk: spans of bare blocks back to back, one lane per span, against the frame parser on the same blocks."""
    import torch
    n = a.spans * a.blocks_per_span
    pick = np.arange(n) % len(frames)
    pieces = [data[int(frames["byte_offset"][i]):int(frames["byte_offset"][i]) + int(frames["byte_length"][i])] for i in pick]
    table = np.zeros(n, aacgpu.PARSE_FRAME_DTYPE)
    table["byte_length"] = [len(x) for x in pieces]
    table["byte_offset"] = np.concatenate([[0], np.cumsum(table["byte_length"])[:-1]])
    buf = np.concatenate(pieces + [np.zeros(32 + (-sum(len(x) for x in pieces)) % 16, np.uint8)])
    first, last = table[::a.blocks_per_span], table[a.blocks_per_span - 1::a.blocks_per_span]
    spans = np.zeros(a.spans, aacgpu.PARSE_FRAME_DTYPE)
    spans["byte_offset"] = first["byte_offset"]
    spans["byte_length"] = last["byte_offset"] + last["byte_length"] - first["byte_offset"]
    dev = torch.device("cuda:0")
    t = lambda arr: torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1)).to(dev)
    d_bytes, d_spans, d_table = t(buf), t(spans), t(table)
    d_out = torch.zeros(a.spans * a.blocks_per_span * 8, dtype=torch.uint8, device=dev)
    d_wres = torch.zeros(a.spans * 16, dtype=torch.uint8, device=dev)
    d_units = torch.zeros(n * 64, dtype=torch.uint8, device=dev)
    d_q = torch.zeros(n * 2 * 1024, dtype=torch.int16, device=dev)
    d_meta = torch.zeros(n * 2 * 120, dtype=torch.int16, device=dev)
    d_res = torch.zeros(n * 8, dtype=torch.uint8, device=dev)
    p = aacgpu.Parser(entries, counts, sample_index=3)
    side = torch.cuda.Stream()
    stream = side.cuda_stream
    torch.cuda.synchronize()
    walk = lambda: p.walk_device(d_bytes.data_ptr(), d_spans.data_ptr(), a.spans, a.blocks_per_span, aacgpu.PARSE_REFERENCE_QUIRKS,
                                 d_out.data_ptr(), d_wres.data_ptr(), stream)
    parse = lambda: p.parse_device(d_bytes.data_ptr(), d_table.data_ptr(), n, 1, 2, aacgpu.PARSE_REFERENCE_QUIRKS,
                                   d_units.data_ptr(), d_q.data_ptr(), d_meta.data_ptr(), None, d_res.data_ptr(), stream)
    ms_walk = timed(walk, side, a.steps, a.warmup)
    got = d_out.cpu().numpy().view(aacgpu.PARSE_FRAME_DTYPE).reshape(a.spans, a.blocks_per_span)
    wres = d_wres.cpu().numpy().view(aacgpu.WALK_RESULT_DTYPE)
    assert not wres["status"].any() and (wres["n_frames"] == a.blocks_per_span).all(), "the walk did not find the blocks"
    assert np.array_equal(got.reshape(-1), table), "the walk's block table is not the frames' table"
    ms_parse = timed(parse, side, a.steps, a.warmup)
    assert not d_res.cpu().numpy().view(aacgpu.PARSE_RESULT_DTYPE)["status"].any()
    p.close()
    print(json.dumps({"kernel": "aacg_parse_walk_spans", "spans": a.spans, "blocks_per_span": a.blocks_per_span, "blocks": n,
                      "bytes_per_block": float(table["byte_length"].mean()), "us_per_walk": ms_walk * 1e3,
                      "us_per_4096_blocks": ms_walk * 1e3 * 4096 / n, "blocks_per_s": n / (ms_walk * 1e-3),
                      "parse_us_same_blocks": ms_parse * 1e3, "parse_us_per_4096_frames": ms_parse * 1e3 * 4096 / n,
                      "codebooks": "stand-in" if a.standin else "standard"}))


if __name__ == "__main__":
    main()
