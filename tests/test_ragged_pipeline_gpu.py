"""Ragged batches on the resident route (aacg_pipeline_decode_ragged / _submit_ragged): each stream of a batch brings its own number
of frames, packed stream after stream (frames, PCM and results alike), on a real MI355X.

Parity: every committed stream (mono, stereo, 5.1, the coupling stream) and every fourth clean corpus stream, decoded through
ragged batches with seeded random per-stream counts, gives the reference's PCM (the tolerances of test_pipeline_gpu.py and
test_corpus.py) and the same bits as the same frames decoded stream by stream through the rectangular aacg_pipeline_decode: no
arithmetic crosses streams.  Then batches in flight on five lanes, refusals at packed indices, a stream without a layout, a
narrower layout after a wider one on the same lane, and the calls that are refused before anything is enqueued."""
import os
import subprocess

import numpy as np
import pytest

import aacgpu
from resident_kit import CASES, CORPUS, ERR_CAPACITY, ERR_INVALID_ARG, NODE, ROOT, adts_frame_table, check_corpus_pcm, close_to, load, packed
from resident_kit import corpus_streams          # noqa: F401  (fixture)


def ragged_run(members, C, si, max_frames, rng):
    """members: [(bytes, frame table)], one slot each.  Ragged batches with random counts (1..max_frames, at most what is left),
    streams that are done drop out.  -> (per-stream PCM by ragged batches, the same frames stream by stream, rectangular)"""
    S = len(members)
    data = np.concatenate([m[0] for m in members])
    bases = np.cumsum([0] + [len(m[0]) for m in members])[:-1]
    tables = [m[1] for m in members]
    p = aacgpu.Pipeline(channels=C, max_streams=S, max_frames=max_frames, sample_index=si)
    o = aacgpu.Pipeline(channels=C, max_streams=S, max_frames=max_frames, sample_index=si, lanes=1)
    at = [0] * S
    got = [[] for _ in range(S)]
    alone = [[] for _ in range(S)]
    while any(at[s] < len(tables[s]) for s in range(S)):
        live = [s for s in range(S) if at[s] < len(tables[s])]
        counts = [int(rng.integers(1, min(max_frames, len(tables[s]) - at[s]) + 1)) for s in live]
        fr = packed([tables[s] for s in live], [bases[s] for s in live], [at[s] for s in live], counts)
        pcm, res, refused = p.decode(data, fr, np.array(live, np.uint32), np.array(counts, np.uint32))
        assert refused == 0 and not res["status"].any()
        first = np.concatenate([[0], np.cumsum(counts)])
        per = 1024 * C
        for k, s in enumerate(live):
            got[s].append(pcm[first[k] * per:first[k + 1] * per])
            one, r1, ref1 = o.decode(data, fr[first[k]:first[k + 1]].copy(), [s], counts[k])
            assert ref1 == 0
            alone[s].append(one)
            at[s] += counts[k]
    p.close()
    o.close()
    return [np.concatenate(g) for g in got], [np.concatenate(a) for a in alone]


@pytest.mark.gpu
def test_ragged_batches_decode_the_committed_streams():
    """four copies of every committed stream in one pipeline (four slots, each with its own random counts per batch)"""
    rng = np.random.default_rng(2026)
    for case in CASES:
        data, table, refpcm = load(case)
        got, alone = ragged_run([(data, table)] * 4, case["channels"], case["sampleIndex"], 16 if case["frames"] > 8 else 4, rng)
        for s in range(4):
            close_to(got[s], refpcm)
            assert np.array_equal(got[s].view(np.uint32), alone[s].view(np.uint32)), (case["name"], s)


@pytest.mark.gpu
def test_ragged_batches_decode_every_fourth_corpus_stream(corpus_streams):
    """one pipeline per (sample rate, channels), every stream a slot of its own, random counts 1..4 per batch"""
    rng = np.random.default_rng(4)
    groups = {}
    for j, e in enumerate(CORPUS):
        if j % 4 == 0 and not e["error"] and e["decoded"] == e["frames"]:
            groups.setdefault((e["si"], e["channels"]), []).append(e)
    assert sum(len(m) for m in groups.values()) >= 30
    for (si, C), members in sorted(groups.items()):
        mem = [(corpus_streams[e["name"]], adts_frame_table(corpus_streams[e["name"]])) for e in members]
        got, alone = ragged_run(mem, C, si, 4, rng)
        for s, e in enumerate(members):
            check_corpus_pcm(e, got[s])
            assert np.array_equal(got[s].view(np.uint32), alone[s].view(np.uint32)), e["name"]


@pytest.mark.gpu
def test_ragged_batches_in_flight_equal_batches_one_at_a_time():
    """64 streams (the stereo stream from different starting frames), five ragged batches submitted on five lanes and collected
    late, against the same batches one at a time on one lane — bit for bit"""
    data, table, refpcm = load(CASES[0])
    rng = np.random.default_rng(5)
    S, B = 64, 5
    counts = rng.integers(1, 4, (B, S))
    starts = [s % (len(table) - int(counts[:, s].sum()) + 1) for s in range(S)]
    at = np.array(starts)
    batches = []
    for b in range(B):
        batches.append(packed([table] * S, [0] * S, list(at), list(counts[b])))
        at = at + counts[b]
    a = aacgpu.Pipeline(channels=2, max_streams=S, max_frames=3, lanes=5)
    o = aacgpu.Pipeline(channels=2, max_streams=S, max_frames=3, lanes=1)
    pinned = [a.pinned(int(counts[b].sum()) * 2048, np.float32) for b in range(B)]
    tickets = [a.submit(data, batches[b], np.arange(S), counts[b], pcm=pinned[b]) for b in range(B)]
    for b in range(B):
        got, res, refused = a.collect(tickets[b])
        want, res1, refused1 = o.decode(data, batches[b], np.arange(S), counts[b])
        assert refused == 0 and refused1 == 0 and not res["status"].any()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), b
    first = np.concatenate([[0], np.cumsum(counts[0])])
    for s in range(S):                                      # a stream that starts at frame 0: the reference's first frames
        if starts[s] == 0:
            ref = refpcm[:counts[0][s] * 2048]
            pcm = pinned[0][first[s] * 2048:first[s + 1] * 2048]
            assert np.abs(pcm.astype(np.float64) - ref).max() <= 1e-5 * max(1.0, 4.0 * float(np.sqrt(np.mean(ref.astype(np.float64) ** 2))))
    a.close()
    o.close()


@pytest.mark.gpu
def test_a_refused_frame_inside_a_ragged_stream_has_its_packed_index():
    data, table, _ = load(CASES[0])
    bad = data.copy()
    off, length = int(table[3]["byte_offset"]), int(table[3]["byte_length"])
    bad[off + 7: off + length] = 0xFF                        # frame 3 of the middle stream: a raw_data_block with no CPE in it
    both = np.concatenate([data, bad])
    counts = [2, 6, 4]
    fr = packed([table] * 3, [0, len(data), 0], [0, 0, 0], counts)
    p = aacgpu.Pipeline(channels=2, max_streams=3, max_frames=8)
    pcm, res, refused = p.decode(both, fr, np.arange(3), np.array(counts, np.uint32))
    assert refused == 1
    assert res["status"][2 + 3] != 0 and np.count_nonzero(res["status"]) == 1
    q = aacgpu.Pipeline(channels=2, max_streams=3, max_frames=8)    # the neighbours as if the stream were not there
    want, _, _ = q.decode(data, packed([table] * 2, [0, 0], [0, 0], [2, 4]), np.array([0, 2]), np.array([2, 4], np.uint32))
    assert np.array_equal(np.concatenate([pcm[:2 * 2048], pcm[8 * 2048:]]).view(np.uint32), want.view(np.uint32))
    p.close()
    q.close()


@pytest.mark.gpu
def test_a_stream_whose_first_frame_does_not_parse_is_silent_and_alone():
    """5.1 streams (layouts learnt from their first frames): the middle stream's first frame does not parse — no layout, every
    frame of it in the batch AACG_PARSE_LAYOUT (or its own parse error) and silent; its neighbours are what they are alone"""
    sur = CASES[1]
    data, table, refpcm = load(sur)
    bad = data.copy()
    off, length = int(table[0]["byte_offset"]), int(table[0]["byte_length"])
    bad[off + 7: off + length] = 0xFF
    both = np.concatenate([data, bad])
    counts = [3, 4, 5]
    fr = packed([table] * 3, [0, len(data), 0], [0, 0, 0], counts)
    p = aacgpu.Pipeline(channels=6, max_streams=3, max_frames=8, sample_index=sur["sampleIndex"])
    pcm, res, refused = p.decode(both, fr, np.arange(3), np.array(counts, np.uint32))
    mid = slice(3, 7)
    assert refused == 4 and (res["status"][mid] != 0).all() and (res["status"][4:7] == aacgpu.PARSE_LAYOUT).all()
    assert not res["status"][:3].any() and not res["status"][7:].any()
    assert not pcm[3 * 6144:7 * 6144].any()
    close_to(pcm[:3 * 6144], refpcm[:3 * 6144])
    close_to(pcm[7 * 6144:], refpcm[:5 * 6144])
    q = aacgpu.Pipeline(channels=6, max_streams=3, max_frames=8, sample_index=sur["sampleIndex"])
    want, _, _ = q.decode(data, packed([table] * 2, [0, 0], [0, 0], [3, 5]), np.array([0, 2]), np.array([3, 5], np.uint32))
    assert np.array_equal(np.concatenate([pcm[:3 * 6144], pcm[7 * 6144:]]).view(np.uint32), want.view(np.uint32))
    p.close()
    q.close()


@pytest.mark.gpu
def test_a_stereo_stream_after_a_surround_batch_leaves_the_other_channels_zero():
    """one lane, channels = 6: a ragged 5.1 batch, then a ragged batch of a stereo stream (CPE only) in the same PCM buffers: its
    channels 2..5 are exact zeros, channels 0..1 the stereo stream's PCM"""
    sur, st = CASES[1], CASES[0]
    d5, t5, ref5 = load(sur)
    d2, t2, ref2 = load(st)
    p = aacgpu.Pipeline(channels=6, max_streams=4, max_frames=8, sample_index=3, lanes=1)
    pcm, res, refused = p.decode(d5, packed([t5] * 2, [0, 0], [0, 0], [5, 3]), np.array([0, 1]), np.array([5, 3], np.uint32))
    assert refused == 0
    close_to(pcm[:5 * 6144], ref5)
    pcm, res, refused = p.decode(d2, packed([t2], [0], [0], [7]), np.array([2]), np.array([7], np.uint32))
    assert refused == 0 and not res["status"].any()
    x = pcm.reshape(7, 1024, 6)
    assert not x[:, :, 2:].any()
    close_to(x[:, :, :2].reshape(-1), ref2[:7 * 2048])
    p.close()


@pytest.mark.gpu
def test_bad_ragged_batches_are_refused_before_anything_is_enqueued():
    data, table, _ = load(CASES[0])
    p = aacgpu.Pipeline(channels=2, max_streams=2, max_frames=4)
    bad = [([1, 0], ERR_INVALID_ARG, [0, 1]), ([1, 5], ERR_CAPACITY, [0, 1]), ([4, 4, 4], ERR_CAPACITY, [0, 1, 1]),
           ([2, 2], ERR_INVALID_ARG, [1, 1])]
    for counts, code, slots in bad:
        fr = packed([table] * len(counts), [0] * len(counts), [0] * len(counts), counts)
        with pytest.raises(aacgpu.AacgError) as e:
            p.submit(data, fr, np.array(slots), np.array(counts, np.uint32))
        assert e.value.code == code, (counts, e.value)
        assert p.lib.aacg_pipeline_last_error(p.handle).decode()
    t = p.submit(data, packed([table] * 2, [0, 0], [0, 0], [1, 3]), np.arange(2), np.array([1, 3], np.uint32))
    assert t == 1, "a refused call takes no ticket"
    pcm, res, refused = p.collect(t)
    assert refused == 0 and not res["status"].any()
    p.close()


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None or not os.path.exists("/usr/include/node/node_api.h"), reason="node / node_api.h not present on this machine")
def test_jittered_streams_on_a_ragged_shared_engine():
    """256 jittered streams on SharedEngine({ resident: true, ragged: true }) against decoders of their own, frame by frame"""
    subprocess.run(["make", "-C", os.path.join(ROOT, "aac.js_amd", "napi")], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "test_ragged_shared.js"), "gpu"], capture_output=True, text=True, timeout=500)
    assert r.returncode == 0 and "ragged shared gpu tests ok" in r.stdout, r.stdout + r.stderr
