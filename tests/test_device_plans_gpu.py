"""Device plans on the resident route (aacg_pipeline_config.plan_mode 1, aacgpu.Pipeline(device_plans=True)): ONE plan shaped on the
device for every batch (aacg_plan_shape, aac.js_amd/csrc/aacg_plan_shape.h) instead of a kept plan per batch shape, on a real
MI355X.  plan_mode 0 — the path every pipeline took until now — is the reference for the bits: a shaped plan holds the same unit,
run and link records as the host planner's, so the PCM must be the same bit for bit; the reference decoder's PCM bounds both with
the project's tolerances (tests/test_ragged_pipeline_gpu.py).  Then: no plan is built per shape, batches in flight on five lanes,
chains of up to three runs, the steady feed's overlap, layouts, malformed frames, and what a shaped plan and its capacity refuse."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import aacgpu
from resident_kit import CASES, CORPUS, ERR_CAPACITY, ERR_INVALID_ARG, ERR_UNSUPPORTED, NODE, ROOT, adts_frame_table, check_corpus_pcm, close_to, load, packed
from resident_kit import ragged_script, run_script, same_bits, steady
from resident_kit import corpus_streams          # noqa: F401  (fixture)


def both_modes(members, C_, si, max_frames, rng, **kw):
    script = ragged_script([m[1] for m in members], max_frames, rng)
    kept = run_script(members, script, C_, si, max_frames, False, **kw)
    shaped = run_script(members, script, C_, si, max_frames, True, **kw)
    assert shaped[3] == 0 and shaped[4]["shaped"] == shaped[4]["launches"] > 0 and kept[4]["shaped"] == 0 and kept[3] > 0
    assert kept[4]["launches"] == shaped[4]["launches"]
    return kept, shaped


@pytest.mark.gpu
def test_same_bits_as_kept_plans_on_the_committed_streams():
    """four copies of every committed stream (mono, stereo, 5.1, the coupling stream, the 8 kHz one), each slot its own random counts"""
    rng = np.random.default_rng(2026)
    for case in CASES:
        data, table, refpcm = load(case)
        kept, shaped = both_modes([(data, table)] * 4, case["channels"], case["sampleIndex"], 16 if case["frames"] > 8 else 4, rng)
        assert kept[2] == 0 and shaped[2] == 0
        for s in range(4):
            assert not kept[1][s].any() and not shaped[1][s].any()
            assert same_bits(shaped[0][s], kept[0][s]), (case["name"], s)
            close_to(shaped[0][s], refpcm)
            close_to(kept[0][s], refpcm)


@pytest.mark.gpu
def test_same_bits_as_kept_plans_on_every_fourth_corpus_stream(corpus_streams):
    """one pipeline per (sample rate, channels) and plan mode, every stream a slot of its own, random counts 1..4 per batch"""
    rng = np.random.default_rng(4)
    groups = {}
    for j, e in enumerate(CORPUS):
        if j % 4 == 0 and not e["error"] and e["decoded"] == e["frames"]:
            groups.setdefault((e["si"], e["channels"]), []).append(e)
    assert sum(len(m) for m in groups.values()) >= 30
    compared = 0
    for (si, C_), members in sorted(groups.items()):
        mem = [(corpus_streams[e["name"]], adts_frame_table(corpus_streams[e["name"]])) for e in members]
        kept, shaped = both_modes(mem, C_, si, 4, rng)
        for s, e in enumerate(members):
            assert same_bits(shaped[0][s], kept[0][s]), e["name"]
            assert np.array_equal(shaped[1][s], kept[1][s])
            check_corpus_pcm(e, shaped[0][s])
            compared += 1
    assert compared == sum(len(m) for m in groups.values()), "every stream that the kept-plan run decodes is compared"


def distinct_shapes(n, S, max_frames, rng):
    shapes = []
    while len(shapes) < n:
        k = int(rng.integers(1, S + 1))
        slots = tuple(int(x) for x in rng.permutation(S)[:k])
        counts = tuple(int(x) for x in rng.integers(1, max_frames + 1, k))
        if (slots, counts) not in shapes:
            shapes.append((slots, counts))
    assert len(set(shapes)) == n, "the shapes are pairwise different"
    return shapes


@pytest.mark.gpu
def test_no_plan_is_built_per_shape():
    """48 consecutive batches of pairwise different shapes: kept plans build one plan per batch, device plans none at all"""
    data, table, _ = load(CASES[0])
    rng = np.random.default_rng(8)
    shapes = distinct_shapes(48, 8, 16, rng)
    builds = {}
    pcm = {}
    for mode in (False, True):
        p = aacgpu.Pipeline(channels=2, max_streams=8, max_frames=16, device_plans=mode)
        builds[mode], pcm[mode] = [], []
        for slots, counts in shapes:
            fr = packed([table] * len(slots), [0] * len(slots), [0] * len(slots), list(counts))
            out, res, refused = p.decode(data, fr, np.array(slots, np.uint32), np.array(counts, np.uint32))
            assert refused == 0 and not res["status"].any()
            builds[mode].append(p.plan_builds())
            pcm[mode].append(out)
        if mode:
            assert p.launch_counts()["shaped"] == len(shapes)
        p.close()
    assert builds[False] == list(range(1, len(shapes) + 1)), "kept plans: one build per new shape"
    assert builds[True][-1] == builds[True][0] == 0, "device plans: no host plan build after set-up"
    for a, b in zip(pcm[False], pcm[True]):
        assert same_bits(a, b)


@pytest.mark.gpu
def test_batches_in_flight_with_a_shape_each():
    """five lanes, a different shape per batch (one of them with a malformed frame), submitted ahead and collected late, against
    the same batches one at a time on one lane in either plan mode: PCM, results and refusals bit for bit"""
    data, table, refpcm = load(CASES[0])
    bad = data.copy()
    off, length = int(table[0]["byte_offset"]), int(table[0]["byte_length"])
    bad[off + 7: off + length] = 0xFF                        # frame 0: a raw_data_block with no CPE in it
    both = np.concatenate([data, bad])
    rng = np.random.default_rng(15)
    S, B = 24, 12
    shapes = distinct_shapes(B, S, 3, rng)
    at = np.zeros(S, np.int64)
    batches = []
    for b, (slots, counts) in enumerate(shapes):
        bases = [len(data) if (b == 4 and k == 0) else 0 for k in range(len(slots))]
        starts = [0 if bases[k] else int(at[s]) % 12 for k, s in enumerate(slots)]
        batches.append((packed([table] * len(slots), bases, starts, list(counts)), np.array(slots, np.uint32), np.array(counts, np.uint32)))
        for s, c in zip(slots, counts):
            at[s] += c
    a = aacgpu.Pipeline(channels=2, max_streams=S, max_frames=3, lanes=5, device_plans=True)
    one = [aacgpu.Pipeline(channels=2, max_streams=S, max_frames=3, lanes=1, device_plans=m) for m in (False, True)]
    results = []
    for start in range(0, B, 6):                              # six ahead on five lanes: the sixth finishes the first's lane
        chunk = batches[start:start + 6]
        pinned = [a.pinned(int(c.sum()) * 2048, np.float32) for _, _, c in chunk]
        tickets = [a.submit(both, fr, sl, c, pcm=pin) for (fr, sl, c), pin in zip(chunk, pinned)]
        results += [a.collect(t) for t in tickets]
    refused_total = 0
    for b, (fr, sl, c) in enumerate(batches):
        got, res, refused = results[b]
        refused_total += refused
        for o in one:
            want, res1, refused1 = o.decode(both, fr, sl, c)
            assert refused == refused1 and np.array_equal(res, res1), b
            assert same_bits(got, want), b
    assert refused_total >= 1 and a.plan_builds() == 0 and a.launch_counts()["shaped"] == B
    a.close()
    for o in one:
        o.close()


@pytest.mark.gpu
def test_long_chains():
    """max_frames 40: chains of one, two and three runs in one batch (no link, one link, two links per chain), bit for bit against
    kept plans; the committed stereo stream has 18 frames, so every stream is fed it again and again — its first 18 frames (across
    the first run's end at frame 16) are the reference's, the rest is bounded by the kept-plan bits"""
    data, table, refpcm = load(CASES[0])
    n = len(table)
    counts = [10, 20, 40, 33, 16, 17, 1, 32]
    assert sorted(set(-(-c // 16) for c in counts)) == [1, 2, 3]
    slots = [5, 0, 7, 2, 6, 1, 4, 3]
    out = {}
    for mode in (False, True):
        p = aacgpu.Pipeline(channels=2, max_streams=8, max_frames=40, device_plans=mode)
        out[mode] = []
        for rep in range(3):                                  # the second and third batch continue every chain's state
            fr = np.concatenate([table[[(rep * c + f) % n for f in range(c)]] for c in counts]).copy()
            pcm, res, refused = p.decode(data, fr, np.array(slots, np.uint32), np.array(counts, np.uint32))
            assert refused == 0 and not res["status"].any()
            out[mode].append(pcm)
        assert p.plan_builds() == (0 if mode else 1)
        p.close()
    for a, b in zip(out[False], out[True]):
        assert same_bits(a, b)
    first = np.concatenate([[0], np.cumsum(counts)])
    for k, c in enumerate(counts):
        m = min(c, n)
        close_to(out[True][0][first[k] * 2048:(first[k] + m) * 2048], refpcm[:m * 2048])


@pytest.mark.gpu
def test_the_steady_feed_still_overlaps():
    """the same shape 32 times, submitted ahead on five lanes: as many launches continue their predecessor with device plans as with
    kept plans (the parent's path is the yardstick), and one batch of another shape in the middle costs exactly two continuations —
    its own and its successor's"""
    data, table, _ = load(CASES[0])
    feed = lambda mode, odd_at=None: steady(data, table, 16, 32, 16, mode, odd_at)
    (kept, pcm0), (shaped, pcm1) = feed(False), feed(True)
    kept, shaped = kept["chained"], shaped["chained"]
    print("continued launches of 32: kept plans %d, device plans %d" % (kept, shaped))
    assert shaped == kept and shaped > 0
    for a, b in zip(pcm0, pcm1):
        assert same_bits(a, b)
    odd, pcm2 = feed(True, odd_at=16)
    odd = odd["chained"]
    print("... with another shape at batch 16: %d" % odd)
    assert odd == shaped - 2
    odd0, pcm3 = feed(False, odd_at=16)
    for a, b in zip(pcm2, pcm3):
        assert same_bits(a, b)


@pytest.mark.gpu
def test_layouts_reset_and_int16(corpus_streams):
    """channels = 8 at 48 kHz: a 5.1 stream, a 7-channel corpus stream, a stereo stream (narrower than the channels: the rest exact
    zeros) and a stream whose first frame does not parse (no layout: silent, refused) in one batch; then the 5.1 slot reset and
    given the stereo stream; every batch bit for bit against kept plans.  int16 PCM once."""
    d5, t5, ref5 = load(CASES[1])
    d2, t2, ref2 = load(CASES[0])
    wide = next(e for e in CORPUS if e["si"] == 3 and e["channels"] == 7 and not e["error"] and e["decoded"] == e["frames"])
    d7 = corpus_streams[wide["name"]]
    t7 = adts_frame_table(d7)
    bad = d5.copy()
    off, length = int(t5[0]["byte_offset"]), int(t5[0]["byte_length"])
    bad[off + 7: off + length] = 0xFF
    data = np.concatenate([d5, d7, d2, bad])
    bases = [0, len(d5), len(d5) + len(d7), len(d5) + len(d7) + len(d2)]
    assert len(t7) >= 3
    counts = [5, 2, 7, 4]
    seen = {}
    for mode in (False, True):
        p = aacgpu.Pipeline(channels=8, max_streams=4, max_frames=8, sample_index=3, device_plans=mode)
        a = p.decode(data, packed([t5, t7, t2, t5], bases, [0, 0, 0, 0], counts), np.array([2, 0, 3, 1]), np.array(counts, np.uint32))
        layouts = [p.stream_layout(s) for s in range(4)]
        b = p.decode(data, packed([t5, t2], [0, bases[2]], [0, 7], [5, 6]), np.array([1, 3]), np.array([5, 6], np.uint32))     # the unlearnt slot learns; stereo goes on
        p.reset_stream(2)
        c = p.decode(data, packed([t2, t7], [bases[2], bases[1]], [0, counts[1]], [8, 1]), np.array([2, 0]), np.array([8, 1], np.uint32))
        seen[mode] = (a, b, c, layouts, p.stream_layout(2), p.plan_builds())
        p.close()
    k, s = seen[False], seen[True]
    assert k[3] == s[3] and k[4] == s[4] == ([2], 1) and s[5] == 0 and k[5] >= 3
    assert s[3][2] == ([1, 2, 2, 1], 4) and s[3][3] == ([2], 1) and s[3][1] == ([], 0) and s[3][0][1] >= 1
    for x, y in zip(k[:3], s[:3]):
        assert same_bits(x[0], y[0]) and np.array_equal(x[1], y[1]) and x[2] == y[2]
    pcm, res, refused = s[0]
    first = np.concatenate([[0], np.cumsum(counts)])
    assert refused == 4 and (res["status"][first[3]:] != 0).all() and not res["status"][:first[3]].any()
    assert not pcm[first[3] * 8192:].any()
    x = pcm[:5 * 8192].reshape(5, 1024, 8)
    assert not x[:, :, 6:].any()
    close_to(x[:, :, :6].reshape(-1), ref5)
    y = pcm[first[2] * 8192:first[3] * 8192].reshape(7, 1024, 8)
    assert not y[:, :, 2:].any()
    close_to(y[:, :, :2].reshape(-1), ref2[:7 * 2048])
    z = s[2][0][:8 * 8192].reshape(8, 1024, 8)                  # the reset slot: the stereo stream from its start
    assert not z[:, :, 2:].any()
    close_to(z[:, :, :2].reshape(-1), ref2[:8 * 2048])
    # int16 PCM
    out = {}
    for mode in (False, True):
        p = aacgpu.Pipeline(channels=2, max_streams=3, max_frames=16, output_kind=aacgpu.OUTPUT_I16, device_plans=mode)
        out[mode] = [p.decode(d2, packed([t2] * 3, [0] * 3, [at] * 3, cnt), np.array([1, 2, 0]), np.array(cnt, np.uint32)) for at, cnt in [(0, [5, 1, 3]), (5, [2, 13, 7])]]
        p.close()
    for x, y in zip(out[False], out[True]):
        assert x[0].dtype == np.int16 and same_bits(x[0], y[0]) and x[2] == y[2] == 0
    assert out[True][0][0].any()


@pytest.mark.gpu
def test_malformed_corpus_frames_among_clean_ones(corpus_streams):
    """the corpus' malformed streams at 48 kHz between clean ones, ragged: the same statuses at the same packed indices, the same
    refusal count and the same bits (the refused frames', decoded as silent ones, included) in both plan modes"""
    checked = 0
    for C_ in (1, 2):
        members = [e for e in CORPUS if e["si"] == 3 and e["channels"] == C_]
        assert any(e["error"] for e in members) and any(not e["error"] for e in members)
        mem = [(corpus_streams[e["name"]], adts_frame_table(corpus_streams[e["name"]])) for e in members]
        kept, shaped = both_modes(mem, C_, 3, 4, np.random.default_rng(C_))
        assert kept[2] == shaped[2] >= sum(1 for e in members if e["error"])
        for s, e in enumerate(members):
            assert np.array_equal(kept[1][s], shaped[1][s]), e["name"]
            assert same_bits(kept[0][s], shaped[0][s]), e["name"]
            checked += int(np.count_nonzero(shaped[1][s]))     # (a refused frame decodes as a silent one: its PCM is the frame before's tail, bit for bit as above)
            if e["error"]:
                assert shaped[1][s][e["error"]["frame"]] != 0, e["name"]
    assert checked > 0


@pytest.mark.gpu
def test_what_a_shaped_plan_refuses():
    """a shaped plan handed to the entry points that need what it does not hold: AACG_ERR_UNSUPPORTED with a text, and the engine
    goes on working; a shape over the capacity: AACG_ERR_CAPACITY, nothing enqueued, the next batch decodes"""
    import aacgpu_workload
    import orc
    import torch
    wl = aacgpu_workload.make_batch(n_streams=2, n_frames=10, mix=True, intensity=True, seed=99)
    eng = aacgpu.Engine(aacgpu.INPUT_QUANT_I16, max_streams=2, max_channels=2)
    plan = eng.plan_shaped(2, 16, 1, 2)
    d = torch.zeros(1 << 16, dtype=torch.float32, device="cuda")
    for call in (lambda: eng.decode_device(plan, d.data_ptr(), d.data_ptr(), d.data_ptr()),
                 lambda: eng.plan_refresh_units(plan, wl["units"]),
                 lambda: eng.spectral_device(plan, d.data_ptr(), d.data_ptr(), d.data_ptr()),
                 lambda: eng._check(eng.lib.aacg_plan_set_unit_sets(eng.handle, plan.handle, 3))):
        with pytest.raises(aacgpu.AacgError) as e:
            call()
        assert e.value.code == ERR_UNSUPPORTED and "aacg_plan_create_shaped" in str(e.value)
    with pytest.raises(aacgpu.AacgError) as e:                 # nothing shaped yet: nothing to launch
        eng.decode_pipelined(plan, d.data_ptr(), d.data_ptr(), d.data_ptr())
    assert e.value.code == ERR_INVALID_ARG
    # the engine's own capacity check, before anything is enqueued or the table touched
    tab = np.zeros(2, aacgpu.SHAPE_STREAM_DTYPE)
    tab["frames"], tab["frame_first"], tab["unit_first"], tab["frame_units"], tab["slot"], tab["nch"] = [17, 3], [0, 17], [0, 17], 0x101, [1, 0], 2
    with pytest.raises(aacgpu.AacgError) as e:
        eng.plan_shape_table(plan, 0, tab, 2)
    assert e.value.code == ERR_CAPACITY and not tab["run_first"].any() and not tab["rot"].any()
    tab["frames"], tab["frame_first"], tab["unit_first"] = [16, 3], [0, 16], [0, 16]
    assert eng.plan_shape_table(plan, 1, tab, 2) == 19 and list(tab["run_first"]) == [1, 0]
    with pytest.raises(aacgpu.AacgError) as e:                 # a third set does not exist
        eng.plan_shape_table(plan, 2, tab, 2)
    assert e.value.code == ERR_INVALID_ARG
    pcm = eng.decode_batch(wl["units"], wl["q"], wl["meta"], wl["n_pcm"])
    ref = orc.load().decode_batch(wl["units"], wl["q"], wl["meta"], wl["n_pcm"], np.zeros((2, 2, 1024), np.float32))
    assert float(np.sqrt(np.mean((pcm.astype(np.float64) - ref) ** 2))) < 1e-5
    plan.destroy()
    eng.close()
    # an engine with optional stages has no shaped plans
    eng = aacgpu.Engine(aacgpu.INPUT_QUANT_I16, max_streams=2, max_channels=2, tns_mode=aacgpu.TNS_SPEC)
    with pytest.raises(aacgpu.AacgError) as e:
        eng.plan_shaped(2, 16)
    assert e.value.code == ERR_UNSUPPORTED
    eng.close()
    # through the pipeline: shapes over its capacity are refused whole, take no ticket, and the next batch decodes
    data, table, refpcm = load(CASES[0])
    p = aacgpu.Pipeline(channels=2, max_streams=2, max_frames=4, device_plans=True)
    for counts, code, slots in [([1, 5], ERR_CAPACITY, [0, 1]), ([4, 4, 4], ERR_CAPACITY, [0, 1, 1]), ([2, 2], ERR_INVALID_ARG, [1, 1]), ([1, 0], ERR_INVALID_ARG, [0, 1])]:
        fr = packed([table] * len(counts), [0] * len(counts), [0] * len(counts), counts)
        with pytest.raises(aacgpu.AacgError) as e:
            p.submit(data, fr, np.array(slots), np.array(counts, np.uint32))
        assert e.value.code == code, (counts, e.value)
    t = p.submit(data, packed([table] * 2, [0, 0], [0, 0], [1, 4]), np.arange(2), np.array([1, 4], np.uint32))
    assert t == 1, "a refused call takes no ticket"
    pcm, res, refused = p.collect(t)
    assert refused == 0 and not res["status"].any()
    close_to(pcm[2048:], refpcm[:4 * 2048])
    p.close()


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None or not os.path.exists("/usr/include/node/node_api.h"), reason="node / node_api.h not present on this machine")
def test_jittered_streams_on_a_shared_engine_with_device_plans():
    """128 jittered streams on SharedEngine({ resident: true, ragged: true, devicePlans: true }) against the same engine with kept
    plans: the same checksums stream by stream, no plan built, every batch shaped on the device"""
    subprocess.run(["make", "-C", os.path.join(ROOT, "aac.js_amd", "napi")], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "test_device_plans.js"), "gpu"], capture_output=True, text=True, timeout=500)
    assert r.returncode == 0 and "device plans gpu tests ok" in r.stdout, r.stdout + r.stderr
