"""The span walk (aacg_parse_walk: where the raw_data_blocks of an MP4 sample run lie) on the CPU: its kernel source
(aacg_parse.h walk_body) in the lane emulator, on the front-end corpus as bare blocks (the ADTS headers cut off) grouped into
spans of 1, 3, 7, 16 and 40 blocks.  It must list exactly the blocks the ADTS headers delimited, stop at the block the frame
parser refuses with the frame parser's status, resume where it says it stopped, and refuse a block a span cuts off."""
import json
import os

import numpy as np
import pytest

import aacgpu
import walk_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORPUS = json.load(open(os.path.join(ROOT, "tests", "golden", "corpus.json")))["streams"]
Q = aacgpu.PARSE_REFERENCE_QUIRKS
INSUFFICIENT_DATA = 1            # AACG_PARSE_INSUFFICIENT_DATA


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    return walk_cases.build_emu(tmp_path_factory.mktemp("walk_emu"))


@pytest.fixture(scope="module")
def streams(tmp_path_factory):
    return walk_cases.regenerate_corpus(tmp_path_factory.mktemp("corpus"), CORPUS)


@pytest.fixture(scope="module")
def block_status(streams):
    """Per stream: the frame parser's status (its kernel source, tests/emu) for each bare block, given its true length."""
    import emu_lib
    emu = emu_lib.Emu()
    entries, counts = aacgpu.standard_codebooks()
    out = {}
    for e in CORPUS:
        bare, table = walk_cases.bare_blocks(streams[e["name"]])
        got = emu_lib.emu_parse(emu, e["si"], entries, counts, bare, table, 8, 8, Q, False)
        out[e["name"]] = got["results"]
    return out


def expected(span, cover, results):
    """What the walk must report for a span covering the blocks `cover` whose frame-parser results are `results`."""
    bad = np.flatnonzero(results["status"])
    n = int(bad[0]) + 1 if len(bad) else len(cover)
    frames = cover[:n].copy()
    status = 0
    if len(bad):
        status = int(results["status"][bad[0]])
        frames["byte_length"][-1] = int(span["byte_offset"]) + int(span["byte_length"]) - int(frames["byte_offset"][-1])
    consumed = int(cover["byte_length"][:n - 1 if len(bad) else n].sum())
    return frames, status, consumed


def test_walk_lists_the_corpus_blocks(walk, streams, block_status):
    n_spans = n_blocks = n_stopped = 0
    for si, (data, spans, cover) in sorted(walk_cases.corpus_spans(streams, CORPUS).items()):
        frames, res = walk_cases.emu_walk(walk, si, data, spans, 40, Q)
        first = {}
        for i, (name, blocks) in enumerate(cover):
            k = first.get(name, 0)
            first[name] = k + len(blocks)
            parsed = block_status[name][k:k + len(blocks)]
            if block_status[name]["status"][:k].any():
                continue                                   # behind the block the reference gave up on
            want, status, consumed = expected(spans[i], blocks, parsed)
            n = int(res["n_frames"][i])
            assert n == len(want) and int(res["status"][i]) == status, (name, i, n, len(want), int(res["status"][i]), status)
            assert np.array_equal(frames[i][:n], want), (name, i)
            assert not frames[i][n:].view(np.uint64).any()
            assert int(res["bytes_consumed"][i]) == consumed, (name, i)
            if status == 0:                                # the walk's length is the frame parser's bits_used / 8
                assert (parsed["bits_used"] == 8 * blocks["byte_length"]).all(), name
            n_spans += 1
            n_blocks += n
            n_stopped += status != 0
    assert n_spans >= 350 and n_blocks >= 1000 and n_stopped == sum(1 for e in CORPUS if e["error"]), (n_spans, n_blocks, n_stopped)


def test_walk_stops_where_the_parser_refuses(walk, streams, block_status):
    """The 30 malformed streams, each as ONE span: the walk stops at the frame the reference threw at, with its message."""
    lib = aacgpu.load_library()
    bad = [e for e in CORPUS if e["error"]]
    assert len(bad) == 30
    for e in bad:
        bare, table = walk_cases.bare_blocks(streams[e["name"]])
        span = np.array([(0, len(bare))], aacgpu.PARSE_FRAME_DTYPE)
        frames, res = walk_cases.emu_walk(walk, e["si"], bare, span, 64, Q)
        t = e["error"]["frame"]
        status = int(res["status"][0])
        assert int(res["n_frames"][0]) == t + 1 and status == int(block_status[e["name"]]["status"][t]) != 0, e["name"]
        assert e["error"]["message"].startswith(lib.aacg_parse_status_string(status).decode()), e["name"]
        assert np.array_equal(frames[0][:t], table[:t]) and int(frames[0][t]["byte_offset"]) == int(table["byte_offset"][t])
        assert int(res["bytes_consumed"][0]) == int(table["byte_offset"][t])


def test_walk_resumes_after_max_frames(walk, streams):
    """Spans of 40 blocks walked 16 at a time: resumed from bytes_consumed, the pieces add up to the block table."""
    e = max((e for e in CORPUS if not e["error"]), key=lambda e: e["frames"])
    bare, table = walk_cases.bare_blocks(streams[e["name"]])
    reps = (40 + len(table) - 1) // len(table) * 3
    data = np.concatenate([bare] * reps)
    full = np.concatenate([table] * reps)
    full["byte_offset"] = np.concatenate([[0], np.cumsum(full["byte_length"])[:-1]])
    full = full[:len(full) // 40 * 40]
    spans, _ = walk_cases.group(full, sizes=(40,))
    got = [[] for _ in spans]
    todo = spans.copy()
    live = list(range(len(spans)))
    rounds = 0
    while live:
        frames, res = walk_cases.emu_walk(walk, e["si"], data, todo[live], 16, Q)
        assert not res["status"].any()
        nxt = []
        for j, i in enumerate(live):
            n = int(res["n_frames"][j])
            assert n == min(16, 40 - len(got[i]))
            got[i].extend(frames[j][:n].tolist())
            c = int(res["bytes_consumed"][j])
            assert c == int(frames[j][:n]["byte_length"].sum())
            todo[i]["byte_offset"] += c
            todo[i]["byte_length"] -= c
            if todo[i]["byte_length"]:
                nxt.append(i)
        live = nxt
        rounds += 1
    assert rounds == 3
    assert np.array_equal(np.array(sum(got, []), aacgpu.PARSE_FRAME_DTYPE), full[:40 * len(spans)])


def test_walk_edges(walk, streams):
    """An empty span lists nothing; a span that ends inside a block refuses that block (AV.Bitstream underflow); a span of ADTS
    frames (headers kept) is walked frame by frame, as the frame parser reads a block that starts with 0xFFF."""
    e = next(e for e in CORPUS if not e["error"] and e["frames"] >= 4 and e["channels"] == 2)
    data = streams[e["name"]]
    bare, table = walk_cases.bare_blocks(data)
    cut = int(table["byte_offset"][3]) + int(table["byte_length"][3]) // 2
    spans = np.array([(0, 0), (0, cut), (int(table["byte_offset"][1]), 0)], aacgpu.PARSE_FRAME_DTYPE)
    frames, res = walk_cases.emu_walk(walk, e["si"], bare, spans, 8, Q)
    assert res[0].tolist() == (0, 0, 0, 0) and res[2].tolist() == (0, 0, 0, 0)
    assert res[1].tolist() == (4, INSUFFICIENT_DATA, int(table["byte_offset"][3]), 0)
    assert np.array_equal(frames[1][:3], table[:3]) and frames[1][3].tolist() == (int(table["byte_offset"][3]), cut - int(table["byte_offset"][3]))
    adts = walk_cases.adts_table(data)
    frames, res = walk_cases.emu_walk(walk, e["si"], data, np.array([(0, len(data))], aacgpu.PARSE_FRAME_DTYPE), len(adts) + 1, Q)
    assert res[0].tolist() == (len(adts), 0, len(data), 0)
    assert np.array_equal(frames[0][:len(adts)], adts)
