"""The mix on the resident route (aacg_pipeline_set_mix, aacgpu.Pipeline(mix=...)) on a real MI355X: a mixed pipeline's PCM equals, BIT FOR
BIT, the rule of include/aacgpu.h applied in numpy float32 (mix_kit.mix_rule) to the PCM an unmixed pipeline of the same configuration
delivers for the same script (resident_kit.run_script) — delivered into page-locked and pageable host memory, left on the device packed
and planar — with the statuses, refusal counts and transform launch counts of the unmixed run.  Every buffer is poisoned first and is
larger than the batch needs, so that an element nobody wrote and an element written outside the batch's block both show."""
import numpy as np
import pytest

import aacgpu
import mix_kit
from resident_kit import CASES, ERR_INVALID_ARG, NODE, OPTIONS, load, members_of, packed, ragged_script, rect_script, run_script, same_bits
from resident_kit import stage_streams          # noqa: F401  (fixture: tests/js/stage_cases.js)

pytestmark = pytest.mark.gpu
CASE = {c["name"]: c for c in CASES}
I16_POISON = 0x7F7F
WAYS = ["pinned", "pageable", "packed", "planar"]


def poison_host(a):
    a[:] = I16_POISON if a.dtype == np.int16 else np.nan
    return a


def is_poison(a):
    return bool((a == I16_POISON).all()) if a.dtype == np.int16 else bool(np.isnan(a).all())


def poisoned_device(shape, i16):
    import torch
    t = torch.full(shape, I16_POISON, dtype=torch.int16, device="cuda") if i16 else torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()                                  # the fill is torch's stream's, the batch a lane's
    return t


def mixed_run(members, script, C_, si, max_frames, device_plans, way, mix, i16=False, **kw):
    """resident_kit.run_script on a pipeline with a mix, the PCM delivered `way` -> (per-stream PCM of O channels, per-stream statuses,
    refusals in all, plan builds, launch counts)"""
    S, O = len(members), len(mix)
    data = np.concatenate([m[0] for m in members])
    bases = np.cumsum([0] + [len(m[0]) for m in members])[:-1]
    tables = [m[1] for m in members]
    dtype = np.int16 if i16 else np.float32
    if i16:
        kw["output_kind"] = aacgpu.OUTPUT_I16
    p = aacgpu.Pipeline(channels=C_, max_streams=S, max_frames=max_frames, sample_index=si, device_plans=device_plans, mix=mix, **kw)
    assert p.channels == O and p.in_channels == C_
    got, status, refusals = [[] for _ in range(S)], [[] for _ in range(S)], 0
    per = 1024 * O
    for live, counts, at in script:
        fr = packed([tables[s] for s in live], [bases[s] for s in live], at, counts)
        n = int(sum(counts))
        first = np.concatenate([[0], np.cumsum(counts)])
        slots, cnt = np.array(live, np.uint32), np.array(counts, np.uint32)
        if way in ("pinned", "pageable"):
            buf = poison_host(p.pinned((n + 1) * per, dtype) if way == "pinned" else np.empty((n + 1) * per, dtype))
            pcm, res, refused = p.decode(data, fr, slots, cnt, pcm=buf)
            assert pcm is buf and is_poison(buf[n * per:]), "the frame behind the batch was written"
            flat = buf[:n * per].copy()
        else:
            planar = way == "planar"
            out = poisoned_device((len(live) + 1, O, max_frames * 1024) if planar else ((n + 1) * per,), i16)
            t = p.submit_device(data, fr, slots, cnt, out, planar=planar, stride_frames=max_frames if planar else None)
            back, res, refused = p.collect(t)
            assert back is out
            dev = out.cpu().numpy()
            if planar:
                assert is_poison(dev[len(live)]), "the row behind the last stream was written"
                parts = []
                for k in range(len(live)):
                    m = counts[k] * 1024
                    parts.append(np.ascontiguousarray(dev[k, :, :m].T).reshape(-1))      # [sample][channel], as the host call's
                    assert not dev[k, :, m:].view(np.uint16 if i16 else np.uint32).any(), "the padding behind a stream's samples is not exactly zero"
                flat = np.concatenate(parts)
            else:
                assert is_poison(dev[n * per:]), "the frame behind the batch was written"
                flat = dev[:n * per]
        refusals += refused
        for k, s in enumerate(live):
            got[s].append(flat[first[k] * per:first[k + 1] * per])
            status[s].append(res["status"][first[k]:first[k + 1]].copy())
    builds, counts_ = p.plan_builds(), p.launch_counts()
    p.close()
    return [np.concatenate(g) for g in got], [np.concatenate(x) for x in status], refusals, builds, counts_


def ruled(run, C_, mix):
    """an unmixed run's per-stream PCM through the rule"""
    return [mix_kit.mix_rule(x.reshape(-1, C_), mix).reshape(-1) for x in run[0]]


def same_as_rule(got, unmixed, C_, mix, what):
    for s, (x, y) in enumerate(zip(got[0], ruled(unmixed, C_, mix))):
        assert same_bits(x, y), "%s: stream %d's mixed PCM differs from the rule over the unmixed pipeline's at %d of %d samples" % (
            what, s, int((x.view(np.uint16 if x.dtype == np.int16 else np.uint32) != y.view(np.uint16 if y.dtype == np.int16 else np.uint32)).sum()), x.size)
    for x, y in zip(got[1], unmixed[1]):
        assert np.array_equal(x, y), what
    assert got[2] == unmixed[2], what
    assert got[4]["launches"] == unmixed[4]["launches"] and got[4]["shaped"] == unmixed[4]["shaped"], what


def committed(name, copies):
    c = CASE[name]
    data, table, _ = load(c)
    return [(data, table[:12])] * copies, c["channels"], c["sampleIndex"]


MIXES = {"surround48-standard": ("surround48", lambda: aacgpu.mix_standard(6, 2)), "surround48-hostile": ("surround48", lambda: mix_kit.hostile_matrix(2, 6)),
         "stereo48-mono": ("stereo48", lambda: aacgpu.mix_standard(2, 1)), "mono22-stereo": ("mono22", lambda: mix_kit.hostile_matrix(2, 1))}
_unmixed = {}


def unmixed_run(name, i16, mode):
    """the yardstick, once per stream, element type and plan mode: the four ways and the matrices share it (and leave it unchanged)"""
    key = (name, i16, mode)
    if key not in _unmixed:
        mem, C_, si = committed(name, 2)
        script = ragged_script([m[1] for m in mem], 4, np.random.default_rng(11))
        assert len(script) >= 2
        _unmixed[key] = (mem, C_, si, script, run_script(mem, script, C_, si, 4, mode, **(dict(output_kind=aacgpu.OUTPUT_I16) if i16 else {})))
    return _unmixed[key]


@pytest.mark.parametrize("way", WAYS)
@pytest.mark.parametrize("case", sorted(MIXES))
def test_mixed_pcm_is_the_rule_over_the_unmixed_pipeline(case, way):
    """test 1: two streams, seeded ragged batches of at most 4 frames, both plan modes, f32 and int16, each way out"""
    name, make = MIXES[case]
    mix = make()
    for i16 in (False, True):
        for mode in (False, True):
            mem, C_, si, script, want = unmixed_run(name, i16, mode)
            got = mixed_run(mem, script, C_, si, 4, mode, way, mix, i16=i16)
            same_as_rule(got, want, C_, mix, "%s, %s, %s, plan mode %d" % (case, way, "int16" if i16 else "f32", mode))
            assert got[2] == 0 and np.abs(got[0][0].astype(np.float64)).max() > (100 if i16 else 1e-3), "the streams are music"
            assert got[0][0].size == want[0][0].size // C_ * len(mix)


def test_lanes_are_reused():
    """test 2: two lanes, stereo48 to mono, eight batches of 2 frames submitted ahead, so that each lane's d_pcm and d_mix serve four
    batches; f32 into page-locked memory and int16 into pageable"""
    data, table, _ = load(CASE["stereo48"])
    mix = mix_kit.hostile_matrix(1, 2)
    script = rect_script(1, 2, 16)
    assert len(script) == 8
    for i16 in (False, True):
        kw = dict(output_kind=aacgpu.OUTPUT_I16) if i16 else {}
        want = run_script([(data, table)], script, 2, 3, 2, False, lanes=2, **kw)
        p = aacgpu.Pipeline(channels=2, max_streams=1, max_frames=2, lanes=2, mix=mix, **kw)
        dtype = np.int16 if i16 else np.float32
        tickets = [p.submit(data, table[a[0]:a[0] + 2], [0], 2, pcm=np.empty(2048, dtype) if i16 else p.pinned(2048, dtype)) for _, _, a in script]
        pcm = np.concatenate([p.collect(t)[0].copy() for t in tickets])
        counts = p.launch_counts()
        p.close()
        assert counts["launches"] == 8 == want[4]["launches"]
        assert same_bits(pcm, mix_kit.mix_rule(want[0][0].reshape(-1, 2), mix).reshape(-1)), "int16" if i16 else "f32"


def test_the_mix_is_positional_over_channels_a_stream_does_not_cover():
    """test 3: a channels = 6 pipeline with a matrix that weighs every position; lane 0 takes a 5.1 batch, then a stereo stream's second
    batch: its output is the rule over (its two channels, four zeros) — what the unmixed pipeline delivers for the same sequence —, so
    nothing of the 5.1 batch that the lane's buffer held leaks through the coefficients of channels 2..5"""
    d51, t51, _ = load(CASE["surround48"])
    d2, t2, _ = load(CASE["stereo48"])
    F = 5
    data = np.concatenate([d51, d2])
    t2 = t2.copy()
    t2["byte_offset"] += len(d51)
    mix = mix_kit.hostile_matrix(2, 6)
    assert (mix[:, 2:] != 0).all()

    def sequence(**kw):
        p = aacgpu.Pipeline(channels=6, max_streams=2, max_frames=F, sample_index=3, lanes=2, **kw)
        tickets = [p.submit(data, t51[:F], [0], F), p.submit(data, t2[:F], [1], F), p.submit(data, t2[F:2 * F], [1], F)]      # lanes 0, 1, 0
        out = []
        for t in tickets:
            pcm, res, refused = p.collect(t)
            assert refused == 0 and not res["status"].any()
            out.append(pcm.copy())
        assert p.stream_layout(1) == ([2], 1)
        p.close()
        return out

    plain, mixed = sequence(), sequence(mix=mix)
    for k in (1, 2):
        frames = plain[k].reshape(F * 1024, 6)
        assert not frames[:, 2:].any() and frames[:, :2].any()
        two = np.concatenate([frames[:, :2], np.zeros((F * 1024, 4), np.float32)], axis=1)
        assert same_bits(mixed[k], mix_kit.mix_rule(two, mix).reshape(-1)), "batch %d" % k
    assert same_bits(mixed[0], mix_kit.mix_rule(plain[0].reshape(-1, 6), mix).reshape(-1))


@pytest.mark.parametrize("way", ["pageable", "packed", "planar"])
def test_refused_and_unlearnt_frames_are_the_mix_of_zeros(way):
    """test 4a: three 5.1 streams — one clean, one whose first frame is malformed (no layout is learnt: every frame of the stream in that
    batch is refused and nothing of them is decoded), one with a malformed frame behind a learnt layout.  Statuses and the refusal count
    are the unmixed run's, the PCM the rule over it, and the unlearnt stream's frames exactly zero samples"""
    c = CASE["surround48"]
    data, table, _ = load(c)

    def broken(at):
        bad = data.copy()
        off, length = int(table[at]["byte_offset"]), int(table[at]["byte_length"])
        bad[off + 7: off + length] = 0xFF                      # a raw_data_block with none of the stream's elements in it
        return bad

    mem = [(data, table), (broken(0), table), (broken(2), table)]
    script = [([0, 1, 2], [2, 1, 3], [0, 0, 0]), ([0, 1, 2], [3, 4, 2], [2, 1, 3])]
    mix = mix_kit.hostile_matrix(2, 6)
    for mode in (False, True):
        want = run_script(mem, script, 6, c["sampleIndex"], 4, mode)
        assert want[2] >= 2 and want[1][1][0] != 0 and want[1][2][2] != 0 and not want[1][0].any(), want[1]
        got = mixed_run(mem, script, 6, c["sampleIndex"], 4, mode, way, mix)
        same_as_rule(got, want, 6, mix, "%s, plan mode %d" % (way, mode))
        assert (got[0][1][:2 * 1024] == 0).all(), "the unlearnt stream's frame is not silent"
        assert got[0][1][2 * 1024:].any() and got[0][2].any() and all(np.isfinite(x).all() for x in got[0])


def test_set_mix_refusals_leave_the_pipeline_as_it_was():
    """test 4b: out_channels 0 and 3, a null matrix, a NaN coefficient, a second call, a call after the first batch: each is
    AACG_ERR_INVALID_ARG with a reason, and the pipeline decodes its next batch exactly as one that never saw the call"""
    data, table, _ = load(CASE["stereo48"])
    fr = [packed([table] * 2, [0, 0], [a, a], [3, 3]) for a in (0, 3)]
    slots = np.arange(2, dtype=np.uint32)
    fresh = aacgpu.Pipeline(channels=2, max_streams=2, max_frames=3)
    want = [fresh.decode(data, f, slots, 3)[0].copy() for f in fr]
    fresh.close()
    good, nan = np.array([[0.25, 0.75]], np.float32), np.array([[0.5, np.nan]], np.float32)

    def refused(p, out_channels, matrix):
        rc = p.lib.aacg_pipeline_set_mix(p.handle, out_channels, None if matrix is None else matrix.ctypes.data)
        assert rc == ERR_INVALID_ARG, (out_channels, matrix, rc)
        reason = p.lib.aacg_pipeline_last_error(p.handle).decode()
        assert "aacg_pipeline_set_mix" in reason and len(reason) > 30, reason
        assert p.lib.aacg_pipeline_out_channels(p.handle) == p.channels
        return reason

    p = aacgpu.Pipeline(channels=2, max_streams=2, max_frames=3)
    reasons = [refused(p, 0, good), refused(p, 3, good), refused(p, 1, None), refused(p, 1, nan), refused(p, 2, np.array([[1, 0], [0, np.inf]], np.float32))]
    assert len(set(reasons[1:4])) == 3
    assert same_bits(p.decode(data, fr[0], slots, 3)[0], want[0])
    refused(p, 1, good)                                        # after the first batch
    assert same_bits(p.decode(data, fr[1], slots, 3)[0], want[1]) and p.launch_counts()["launches"] == 2
    p.close()

    p = aacgpu.Pipeline(channels=2, max_streams=2, max_frames=3, mix=good)
    assert p.channels == 1 and p.lib.aacg_pipeline_out_channels(p.handle) == 1
    refused(p, 2, np.eye(2, dtype=np.float32))                 # a second call
    with pytest.raises(aacgpu.AacgError):
        p.set_mix(np.eye(2, dtype=np.float32))
    assert p.channels == 1
    for f, w in zip(fr, want):
        assert same_bits(p.decode(data, f, slots, 3)[0], mix_kit.mix_rule(w.reshape(-1, 2), good).reshape(-1))
    p.close()


@pytest.mark.skipif(NODE is None, reason="node not present")
@pytest.mark.parametrize("way", ["pinned", "planar"])
def test_with_the_spec_stages_and_a_carried_window_shape(stage_streams, way):
    """test 5: tns_spec + pns_spec + carry_window_shape on the stage streams, stereo to the hostile pair of rows, against the unmixed
    pipeline with the same options by the rule"""
    kw = dict(tns_spec=True, pns_spec=True, carry_window_shape=True, parse_options=OPTIONS)
    mem = members_of(stage_streams, ["stereo48", "split48"], 2)
    script = ragged_script([m[1] for m in mem], 4, np.random.default_rng(5))
    mix = mix_kit.hostile_matrix(2, 2)
    want = run_script(mem, script, 2, 3, 4, False, **kw)
    got = mixed_run(mem, script, 2, 3, 4, False, way, mix, **kw)
    same_as_rule(got, want, 2, mix, "stages, %s" % way)
    assert want[0][0].any()
