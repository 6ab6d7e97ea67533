"""GPU: the span walk (aacg_parse_walk, aacg_parse_walk_device) on the MI355X equals its kernel source in the lane emulator byte for
byte, on the front-end corpus as bare blocks in spans of 1, 3, 7, 16 and 40; its block table fed to the frame parser parses every
block as the ADTS frame table does."""
import json
import os

import numpy as np
import pytest

import aacgpu
import walk_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORPUS = json.load(open(os.path.join(ROOT, "tests", "golden", "corpus.json")))["streams"]
Q = aacgpu.PARSE_REFERENCE_QUIRKS


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    return walk_cases.build_emu(tmp_path_factory.mktemp("walk_emu"))


@pytest.fixture(scope="module")
def streams(tmp_path_factory):
    return walk_cases.regenerate_corpus(tmp_path_factory.mktemp("corpus"), CORPUS)


@pytest.mark.gpu
def test_gpu_walk_equals_the_emulator_on_the_corpus(walk, streams):
    import torch
    dev = torch.device("cuda:0")
    n_blocks = 0
    for si, (data, spans, _) in sorted(walk_cases.corpus_spans(streams, CORPUS).items()):
        want_f, want_r = walk_cases.emu_walk(walk, si, data, spans, 40, Q)
        p = aacgpu.Parser(sample_index=si)
        got_f, got_r = p.walk(data, spans, 40, Q)
        assert got_f.tobytes() == want_f.tobytes() and got_r.tobytes() == want_r.tobytes(), si
        # the device entry on the parser's own stream (stream 0; no torch side stream: its pool of streams would shift the HIP
        # runtime's stream -> hardware queue assignment for the tests that follow): 16-byte aligned bytes, 32 readable bytes behind
        buf = np.concatenate([data, np.zeros(32 + (-len(data)) % 16, np.uint8)])
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)
        d_bytes, d_spans = t(buf), t(spans)
        d_frames = torch.full((len(spans) * 40 * 8,), 0xAB, dtype=torch.uint8, device=dev)
        d_res = torch.full((len(spans) * 16,), 0xAB, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        p.walk_device(d_bytes.data_ptr(), d_spans.data_ptr(), len(spans), 40, Q, d_frames.data_ptr(), d_res.data_ptr(), 0)
        torch.cuda.synchronize()
        res = d_res.cpu().numpy().view(aacgpu.WALK_RESULT_DTYPE)
        frames = d_frames.cpu().numpy().view(aacgpu.PARSE_FRAME_DTYPE).reshape(len(spans), 40)
        assert res.tobytes() == want_r.tobytes(), si
        for i, n in enumerate(res["n_frames"]):          # the device entry leaves the slots beyond a span's count alone
            assert frames[i][:n].tobytes() == want_f[i][:n].tobytes(), (si, i)
        n_blocks += int(res["n_frames"].sum())
        p.close()
    assert n_blocks >= 1000


@pytest.mark.gpu
def test_gpu_walked_table_parses_like_the_adts_table(streams):
    """Every fourth corpus stream as one span of bare blocks: the walk's table, given to aacg_parse_batch, yields the records the
    stripped ADTS table yields (up to the block the reference gave up on)."""
    n = 0
    for e in CORPUS[::4]:
        bare, table = walk_cases.bare_blocks(streams[e["name"]])
        p = aacgpu.Parser(sample_index=e["si"])
        frames, res = p.walk(bare, np.array([(0, len(bare))], aacgpu.PARSE_FRAME_DTYPE), len(table), Q)
        k = int(res["n_frames"][0])
        assert k == (e["error"]["frame"] + 1 if e["error"] else len(table)), e["name"]
        good = k - (1 if e["error"] else 0)
        assert np.array_equal(frames[0][:good], table[:good]), e["name"]
        a = p.parse_batch(bare, frames[0][:k], 8, 8, Q)
        b = p.parse_batch(bare, table[:k], 8, 8, Q)
        assert a["results"]["status"].tolist() == b["results"]["status"].tolist(), e["name"]
        for key in ("units", "q", "meta"):
            assert a[key][:good * 8].tobytes() == b[key][:good * 8].tobytes(), (e["name"], key)      # 8 records / blocks per frame
        p.close()
        n += 1
    assert n >= 60


@pytest.mark.gpu
def test_gpu_walk_resumes_and_refuses_a_cut_block(walk, streams):
    e = max((e for e in CORPUS if not e["error"]), key=lambda e: e["frames"])
    bare, table = walk_cases.bare_blocks(streams[e["name"]])
    data = np.concatenate([bare] * 40)
    full = np.concatenate([table] * 40)
    full["byte_offset"] = np.concatenate([[0], np.cumsum(full["byte_length"])[:-1]])
    full = full[:len(full) // 40 * 40]
    spans, _ = walk_cases.group(full, sizes=(40,))
    cut = spans[-1].copy()
    cut["byte_length"] -= int(full["byte_length"][-1]) // 2
    spans = np.concatenate([spans, [cut], np.array([(0, 0)], aacgpu.PARSE_FRAME_DTYPE)])
    p = aacgpu.Parser(sample_index=e["si"])
    todo, got = spans.copy(), [[] for _ in spans]
    for _ in range(3):                                   # 40 blocks, 16 at a time
        frames, res = p.walk(data, todo, 16, Q)
        want_f, want_r = walk_cases.emu_walk(walk, e["si"], data, todo, 16, Q)
        assert frames.tobytes() == want_f.tobytes() and res.tobytes() == want_r.tobytes()
        for i in range(len(spans)):
            got[i].extend(frames[i][:int(res["n_frames"][i])].tolist())
            if res["status"][i] == 0:
                todo[i]["byte_offset"] += res["bytes_consumed"][i]
                todo[i]["byte_length"] -= res["bytes_consumed"][i]
    p.close()
    for i in range(len(spans) - 2):
        assert np.array_equal(np.array(got[i], aacgpu.PARSE_FRAME_DTYPE), full[40 * i:40 * i + 40])
    assert len(got[-2]) == 40 and int(res["status"][-2]) == 1 and got[-1] == []    # AACG_PARSE_INSUFFICIENT_DATA; the empty span
