"""The resampler on the resident route (aacg_pipeline_set_resample, aacgpu.Pipeline(resample=...) / (out_rate=...)) on a real MI355X: a
resampled pipeline's PCM equals, BIT FOR BIT, the rule of include/aacgpu.h applied in numpy float32 (resample_kit.resample_rule) to the PCM
that a pipeline WITHOUT a resampler delivers for the same script (resident_kit.run_script), concatenated per slot across the batches —
behind mix_kit.mix_rule where a mix is set.  Delivered into page-locked and pageable host memory, left on the device packed and planar;
statuses, refusal counts and transform launch counts are the unresampled run's.  Every buffer is poisoned first and is larger than the
batch needs, so that an element nobody wrote and an element written outside the batch's block both show."""
import numpy as np
import pytest

import aacgpu
import mix_kit
import resample_kit as kit
from resident_kit import CASES, ERR_CAPACITY, ERR_INVALID_ARG, NODE, OPTIONS, load, members_of, packed, ragged_script, run_script, same_bits
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


def resampled_run(members, script, C_, si, max_frames, device_plans, way, resample, mix=None, i16=False, ahead=False, reset=None, **kw):
    """resident_kit.run_script on a pipeline with a resampler (and a mix), the PCM delivered `way`; ahead: every batch is submitted before
    the first is collected; reset: {batch index: slots reset in front of it} -> (per-stream [samples x O] arrays, per-stream statuses,
    refusals in all, plan builds, launch counts)"""
    S, O = len(members), len(mix) if mix is not None else C_
    data = np.concatenate([m[0] for m in members])
    bases = np.cumsum([0] + [len(m[0]) for m in members])[:-1]
    tables = [m[1] for m in members]
    dtype = np.int16 if i16 else np.float32
    if i16:
        kw["output_kind"] = aacgpu.OUTPUT_I16
    L, M, table = resample
    p = aacgpu.Pipeline(channels=C_, max_streams=S, max_frames=max_frames, sample_index=si, device_plans=device_plans, mix=mix, resample=resample, **kw)
    assert p.channels == O and p.in_channels == C_ and p.resample[:2] == (L, M) and abs(p.rate * M - aacgpu.SAMPLE_RATES[si] * L) < 1e-6
    got, status, refusals, pending = [[] for _ in range(S)], [[] for _ in range(S)], 0, []
    clock = [0] * S                                          # the test's own count of what each slot has consumed

    def finish(item):
        nonlocal refusals
        ticket, live, counts, n_out, buf = item
        back, res, refused, lengths = p.collect(ticket)
        assert back is buf and lengths.tolist() == n_out
        total, first = sum(n_out), np.concatenate([[0], np.cumsum(counts)])
        if way in ("pinned", "pageable"):
            assert is_poison(buf[total * O:]), "the samples behind the batch were written"
            parts = np.split(buf[:total * O].copy(), np.cumsum(n_out)[:-1] * O)
        else:
            dev = buf.cpu().numpy()
            if way == "planar":
                assert is_poison(dev[len(live)]), "the row behind the last stream was written"
                parts = []
                for k in range(len(live)):
                    parts.append(np.ascontiguousarray(dev[k, :, :n_out[k]].T).reshape(-1))      # [sample][channel], as the host call's
                    assert not dev[k, :, n_out[k]:].view(np.uint16 if i16 else np.uint32).any(), "the padding behind a stream's samples is not exactly zero"
            else:
                assert is_poison(dev[total * O:]), "the samples behind the batch were written"
                parts = np.split(dev[:total * O], np.cumsum(n_out)[:-1] * O)
        refusals += refused
        for k, s in enumerate(live):
            got[s].append(parts[k].reshape(-1, O))
            status[s].append(res["status"][first[k]:first[k + 1]].copy())

    for b, (live, counts, at) in enumerate(script):
        for s in (reset or {}).get(b, []):
            for item in pending:
                finish(item)
            pending = []
            p.reset_stream(s)
            clock[s] = 0
        fr = packed([tables[s] for s in live], [bases[s] for s in live], at, counts)
        slots, cnt = np.array(live, np.uint32), np.array(counts, np.uint32)
        n_out = [kit.n_out(clock[s], clock[s] + 1024 * c, L, M) for s, c in zip(live, counts)]
        assert p.out_samples(slots, cnt).tolist() == n_out, "aacg_pipeline_out_samples against the formula"
        total = sum(n_out)
        if way in ("pinned", "pageable"):
            buf = poison_host(p.pinned((total + 64) * O, dtype) if way == "pinned" else np.empty((total + 64) * O, dtype))
            t = p.submit(data, fr, slots, cnt, pcm=buf)
        else:
            planar = way == "planar"
            stride = (max(n_out) + 1023) // 1024 + (b % 2)       # (every other batch a row longer than it need be)
            buf = poisoned_device((len(live) + 1, O, stride * 1024) if planar else ((total + 64) * O,), i16)
            t = p.submit_device(data, fr, slots, cnt, buf, planar=planar, stride_frames=stride if planar else None)
        for s, c in zip(live, counts):
            clock[s] += 1024 * c
        pending.append((t, live, counts, n_out, buf))
        if not ahead:
            finish(pending.pop())
    for item in pending:
        finish(item)
    builds, counts_ = p.plan_builds(), p.launch_counts()
    p.close()
    return [np.concatenate(g) for g in got], [np.concatenate(x) for x in status], refusals, builds, counts_


def ruled(plain, C_, resample, mix=None, cuts=None):
    """a run's per-stream PCM without a resampler through the rule (behind the mix's); cuts: {stream: samples at which its clock was reset}"""
    L, M, table = resample
    out = []
    for s, x in enumerate(plain[0]):
        x = x.reshape(-1, C_)
        if mix is not None:
            x = mix_kit.mix_rule(x, mix)
        pieces = np.split(x, (cuts or {}).get(s, []))
        out.append(np.concatenate([kit.resample_rule(piece, L, M, table) for piece in pieces]))
    return out


def same_as_rule(got, plain, C_, resample, what, mix=None, cuts=None):
    for s, (x, y) in enumerate(zip(got[0], ruled(plain, C_, resample, mix, cuts))):
        assert same_bits(x, y), "%s: stream %d's resampled PCM differs from the rule over the plain pipeline's at %s of %d samples" % (
            what, s, "?" if x.shape != y.shape else int((x.view(np.uint16 if x.dtype == np.int16 else np.uint32) != y.view(np.uint16 if y.dtype == np.int16 else np.uint32)).sum()), y.size)
    for x, y in zip(got[1], plain[1]):
        assert np.array_equal(x, y), what
    assert got[2] == plain[2], what
    assert got[4]["launches"] == plain[4]["launches"] and got[4]["shaped"] == plain[4]["shaped"], what


def committed(name, copies, frames=12):
    c = CASE[name]
    data, table, _ = load(c)
    return [(data, table[:frames])] * copies, c["channels"], c["sampleIndex"]


# stream, the resampler, the mix in front of it
SETUPS = {"stereo48-to-16k": ("stereo48", lambda: aacgpu.resample_design(48000, 16000, 32), None),
          "stereo48-up-hostile": ("stereo48", lambda: (160, 147, kit.hostile_table(160, 8)), None),
          "surround48-stereo-16k": ("surround48", lambda: aacgpu.resample_design(48000, 16000, 32), lambda: aacgpu.mix_standard(6, 2)),
          "mono22-to-16k": ("mono22", lambda: aacgpu.resample_design(22050, 16000, 16), None)}
_plain = {}


def plain_run(name, i16, mode):
    """the yardstick, once per stream, element type and plan mode: the four ways and the resamplers share it (and leave it unchanged)"""
    key = (name, i16, mode)
    if key not in _plain:
        mem, C_, si = committed(name, 2)
        script = ragged_script([m[1] for m in mem], 4, np.random.default_rng(11))
        assert len(script) >= 2
        _plain[key] = (mem, C_, si, script, run_script(mem, script, C_, si, 4, mode, **(dict(output_kind=aacgpu.OUTPUT_I16) if i16 else {})))
    return _plain[key]


@pytest.mark.parametrize("way", WAYS)
@pytest.mark.parametrize("case", sorted(SETUPS))
def test_resampled_pcm_is_the_rule_over_the_plain_pipeline(case, way):
    """two streams, seeded ragged batches of at most 4 frames, both plan modes, f32 and int16, each way out; 48 kHz stereo to 16 kHz, up by
    160 / 147 with a hostile table, six channels to two to 16 kHz, 22.05 kHz mono to 16 kHz (320 / 441)"""
    name, make, make_mix = SETUPS[case]
    resample, mix = make(), make_mix() if make_mix else None
    for i16 in (False, True):
        for mode in (False, True):
            mem, C_, si, script, want = plain_run(name, i16, mode)
            got = resampled_run(mem, script, C_, si, 4, mode, way, resample, mix=mix, i16=i16)
            same_as_rule(got, want, C_, resample, "%s, %s, %s, plan mode %d" % (case, way, "int16" if i16 else "f32", mode), mix=mix)
            assert got[2] == 0 and np.abs(got[0][0].astype(np.float64)).max() > (100 if i16 else 1e-3), "the streams are music"
            frames = want[0][0].size // (1024 * C_)
            assert len(got[0][0]) == kit.ceil_div(frames * 1024 * resample[0], resample[1])


@pytest.mark.parametrize("way,i16", [("pinned", False), ("pageable", True), ("planar", False), ("packed", True)])
def test_history_crosses_lanes_in_order(way, i16):
    """seven consecutive ragged batches of the same two slots on five lanes, ALL submitted before the first is collected: every batch's
    resample launch reads the history the one before it wrote, from another lane's stream, and batches six and seven reuse lanes one
    and two.  44.1-style ratio 160 / 441 with 64 taps, so that every frame boundary falls mid-phase"""
    data, table, _ = load(CASE["stereo48"])
    mem = [(data, table[:18]), (data, table[:18])]
    counts = [[3, 1, 4, 2, 1, 3, 4], [1, 4, 2, 3, 3, 1, 4]]
    at = [np.concatenate([[0], np.cumsum(c)]) for c in counts]
    script = [([0, 1], [counts[0][b], counts[1][b]], [int(at[0][b]), int(at[1][b])]) for b in range(7)]
    resample = (160, 441, kit.hostile_table(160, 64))
    kw = dict(output_kind=aacgpu.OUTPUT_I16) if i16 else {}
    for mode in (False, True):
        want = run_script(mem, script, 2, 3, 4, mode, lanes=5, **kw)
        got = resampled_run(mem, script, 2, 3, 4, mode, way, resample, i16=i16, ahead=True, lanes=5)
        same_as_rule(got, want, 2, resample, "%s, plan mode %d" % (way, mode))
        assert got[4]["launches"] == 7 and len(got[0][0]) == kit.ceil_div(18 * 1024 * 160, 441)


def test_lanes_are_reused_and_a_reset_starts_clock_and_history_again():
    """two lanes, one slot, six batches submitted ahead; aacg_pipeline_reset_stream in front of the fourth, at 7 frames — a clock that is
    no multiple of M: from there on the output is the rule over the frames since the reset, with zeros in front of them"""
    data, table, _ = load(CASE["stereo48"])
    mem = [(data, table[:18])]
    script = [([0], [c], [a]) for c, a in zip([3, 2, 2, 4, 3, 4], [0, 3, 5, 7, 11, 14])]
    resample = (160, 441, kit.hostile_table(160, 32))
    assert (7 * 1024) % 441 != 0

    def plain():
        p = aacgpu.Pipeline(channels=2, max_streams=1, max_frames=4, lanes=2)
        out = []
        for b, (live, counts, at) in enumerate(script):
            if b == 3:
                p.reset_stream(0)
            out.append(p.decode(data, table[at[0]:at[0] + counts[0]], [0], counts[0])[0].copy())
        res = ([np.concatenate(out)], [np.zeros(18, np.uint32)], 0, p.plan_builds(), p.launch_counts())
        p.close()
        return res

    want = plain()
    for way in ("pinned", "packed"):
        got = resampled_run(mem, script, 2, 3, 4, False, way, resample, ahead=True, reset={3: [0]}, lanes=2)
        same_as_rule(got, want, 2, resample, way, cuts={0: [7 * 1024]})
        assert len(got[0][0]) == kit.ceil_div(7 * 1024 * 160, 441) + kit.ceil_div(11 * 1024 * 160, 441)


@pytest.mark.parametrize("way", ["pageable", "planar"])
def test_silence_flows_through_the_filter(way):
    """three 5.1 streams mixed to two channels and brought to 16 kHz — one clean, one whose first frame is malformed (no layout is learnt in
    the first batch: every frame of it there is refused, 1024 zeros each, and the stream is learnt late, in the second), one with a
    malformed frame behind a learnt layout (a refused frame: silence between music).  The frames of silence advance the clock and pass
    through the filter like any other; statuses and the refusal count are the plain run's"""
    c = CASE["surround48"]
    data, table, _ = load(c)

    def broken(at):
        bad = data.copy()
        off, length = int(table[at]["byte_offset"]), int(table[at]["byte_length"])
        bad[off + 7: off + length] = 0xFF                      # a raw_data_block with none of the stream's elements in it
        return bad

    mem = [(data, table), (broken(0), table), (broken(2), table)]
    script = [([0, 1, 2], [2, 1, 3], [0, 0, 0]), ([0, 1, 2], [3, 4, 2], [2, 1, 3])]
    mix, resample = mix_kit.hostile_matrix(2, 6), aacgpu.resample_design(48000, 16000, 32)
    for mode in (False, True):
        want = run_script(mem, script, 6, c["sampleIndex"], 4, mode)
        assert want[2] >= 2 and want[1][1][0] != 0 and want[1][2][2] != 0 and not want[1][0].any(), want[1]
        got = resampled_run(mem, script, 6, c["sampleIndex"], 4, mode, way, resample, mix=mix)
        same_as_rule(got, want, 6, resample, "%s, plan mode %d" % (way, mode), mix=mix)
        assert (got[0][1][:342] == 0).all() and got[0][1][342:].any(), "the unlearnt stream's frame is not silent, or what follows it is"
        assert got[0][2].any() and all(np.isfinite(x).all() for x in got[0])


def test_set_resample_refusals_leave_the_pipeline_as_it_was():
    """a limit broken, a null table, a coefficient that is not finite, a second call, a call after the first batch; on a resampled
    pipeline a planar stride too short and a d_pcm_bytes too small: each is refused with a reason before anything is enqueued, and the
    pipeline decodes its next batch exactly as one that never saw the call"""
    import torch
    data, table, _ = load(CASE["stereo48"])
    fr = [packed([table] * 2, [0, 0], [a, a], [3, 3]) for a in (0, 3)]
    slots = np.arange(2, dtype=np.uint32)
    fresh = aacgpu.Pipeline(channels=2, max_streams=2, max_frames=3)
    want = [fresh.decode(data, f, slots, 3)[0].copy() for f in fr]
    fresh.close()
    L, M, h = aacgpu.resample_design(48000, 16000, 32)
    nan = h.copy()
    nan[0, 5] = np.nan

    def refused(p, L_, M_, taps, t):
        rc = p.lib.aacg_pipeline_set_resample(p.handle, L_, M_, taps, None if t is None else t.ctypes.data)
        assert rc == ERR_INVALID_ARG, (L_, M_, taps, rc)
        reason = p.lib.aacg_pipeline_last_error(p.handle).decode()
        assert reason.startswith("aacg_pipeline_set_resample: ") and len(reason) > len("aacg_pipeline_set_resample: "), reason
        return reason

    p = aacgpu.Pipeline(channels=2, max_streams=2, max_frames=3)
    big = np.zeros(16384 * 2, np.float32)
    reasons = [refused(p, 1, 3, 30, h), refused(p, 1, 3, 68, h), refused(p, 1025, 1024, 4, big), refused(p, 441, 160, 64, big), refused(p, 1, 9, 4, big),
               refused(p, 9, 1, 4, big), refused(p, 1, 3, 32, None), refused(p, 1, 3, 32, nan)]
    assert len(set(reasons)) == 6
    assert p.resample is None and p.out_samples(slots, 3).tolist() == [3072, 3072]
    assert same_bits(p.decode(data, fr[0], slots, 3)[0], want[0])
    refused(p, L, M, 32, h)                                     # after the first batch
    assert same_bits(p.decode(data, fr[1], slots, 3)[0], want[1]) and p.launch_counts()["launches"] == 2
    p.close()

    p = aacgpu.Pipeline(channels=2, max_streams=2, max_frames=3, resample=(L, M, h))
    assert "already" in refused(p, L, M, 32, h)                 # a second call
    with pytest.raises(aacgpu.AacgError):
        p.set_mix(np.eye(2, dtype=np.float32))                  # the mix comes first
    out = torch.zeros(2 * 2 * 1024, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(aacgpu.AacgError) as e:                  # three frames are 1024 samples at 16 kHz: 2 x 2 x 1024 elements packed
        p.submit_device(data, fr[0], slots, 3, (out.data_ptr(), 2 * 2 * 1024 * 4 - 4))
    assert e.value.code == ERR_CAPACITY and "d_pcm_bytes" in str(e.value)
    up = aacgpu.Pipeline(channels=2, max_streams=2, max_frames=3, resample=(2, 1, kit.hostile_table(2, 4)))
    with pytest.raises(aacgpu.AacgError) as e:                  # 3 frames are 6144 samples at twice the rate: rows of 5 x 1024 do not hold them
        up.submit_device(data, fr[0], slots, 3, torch.zeros(2 * 2 * 6 * 1024, dtype=torch.float32, device="cuda"), planar=True, stride_frames=5)
    assert e.value.code == ERR_INVALID_ARG and "stride_frames" in str(e.value)
    assert up.out_samples(slots, 3).tolist() == [6144, 6144], "a refused submission moved the clocks"
    up.close()
    # the refused submissions left clocks and histories alone: both batches, as if nothing had happened
    got = np.concatenate([p.decode(data, f, slots, 3)[0].reshape(2, -1, 2) for f in fr], axis=1)
    for s in range(2):
        plain = np.concatenate([w.reshape(2, 3 * 1024, 2)[s] for w in want])
        assert same_bits(np.ascontiguousarray(got[s]), kit.resample_rule(plain, L, M, h))
    assert not (out.cpu().numpy() != 0).any(), "a refused submission wrote the caller's memory"
    p.close()


@pytest.mark.skipif(NODE is None, reason="node not present")
@pytest.mark.parametrize("way", ["pinned", "planar"])
def test_with_the_spec_stages_and_a_carried_window_shape(stage_streams, way):
    """tns_spec + pns_spec + carry_window_shape on the stage streams to 16 kHz, against the plain pipeline with the same options by the
    rule: the shape carry's cross-lane order and the resampler's side by side"""
    kw = dict(tns_spec=True, pns_spec=True, carry_window_shape=True, parse_options=OPTIONS)
    mem = members_of(stage_streams, ["stereo48", "split48"], 2)
    script = ragged_script([m[1] for m in mem], 4, np.random.default_rng(5))
    resample = aacgpu.resample_design(48000, 16000, 32)
    want = run_script(mem, script, 2, 3, 4, False, **kw)
    got = resampled_run(mem, script, 2, 3, 4, False, way, resample, ahead=True, **kw)
    same_as_rule(got, want, 2, resample, "stages, %s" % way)
    assert want[0][0].any()


def test_decode_tensor_and_out_rate():
    """Pipeline(out_rate=) designs from the pipeline's sample rate; decode_tensor returns the planar tensor and the lengths"""
    data, table, _ = load(CASE["stereo48"])
    plain = aacgpu.Pipeline(channels=2, max_streams=2, max_frames=4)
    fr = packed([table] * 2, [0, 0], [0, 0], [4, 2])
    want = plain.decode(data, fr, [0, 1], [4, 2])[0].reshape(-1, 2)
    plain.close()
    p = aacgpu.Pipeline(channels=2, max_streams=2, max_frames=4, out_rate=16000)
    L, M, h = p.resample
    assert (L, M) == (1, 3) and p.rate == 16000 and same_bits(h, aacgpu.resample_design(48000, 16000, 32)[2])
    out, lengths, res, refused = p.decode_tensor(data, fr, [0, 1], [4, 2])
    assert tuple(out.shape) == (2, 2, 2048) and lengths.tolist() == [1366, 683] and refused == 0
    dev = out.cpu().numpy()
    assert same_bits(np.ascontiguousarray(dev[0, :, :1366].T), kit.resample_rule(want[:4096], L, M, h))
    assert same_bits(np.ascontiguousarray(dev[1, :, :683].T), kit.resample_rule(want[4096:], L, M, h))
    assert not dev[0, :, 1366:].any() and not dev[1, :, 683:].any()
    p.close()
