"""Refused frames concealed on the resident route (aacg_pipeline_set_concealment, aacgpu.Pipeline(conceal=...)), on a real MI355X:
behind every refresh one launch of aacg_units_conceal replaces a refused frame's records by its stream's last good frame, faded.

The yardstick is the conceal kit's host route: aacg_parse_batch -> the numpy rule applied to units, q and meta -> Engine.plan ->
decode_pipelined.  The pipeline's PCM is bit-identical to it — the equality the resident route holds against the host-planned route
anyway, so no tolerance is introduced; the oracle's decode_batch of the same substituted records bounds both with the project's
tolerances.

Streams: tests/js/shape_cases.js (12 frames each: mono, stereo and 5.1 at sample index 3; short windows and KBD).  max_frames 4, three
to four slots, five lanes with every batch submitted before the first is collected, ragged counts.  A frame is dropped by cutting
its table entry to 9 bytes; every stream keeps at least 7 good frames of 12."""
import numpy as np
import pytest

import aacgpu
import conceal_kit as kit
import mix_kit
import resample_kit
from resident_kit import ERR_INVALID_ARG, ERR_UNSUPPORTED, GROUPS, NODE, close_to, members_of, packed, same_bits
from resident_kit import oracle          # noqa: F401  (fixture)
from resident_kit import shape_streams as streams          # noqa: F401  (fixture: tests/js/shape_cases.js)

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not present")]

FADE, HOLD = 2, 3
# four batches, each stream's 12 frames: (live slots, counts, first frames); the fourth slot only where there is one
SCRIPT4 = [([0, 1, 2, 3], [4, 2, 3, 1], [0, 0, 0, 0]), ([0, 1, 2, 3], [1, 4, 3, 4], [4, 2, 3, 1]),
           ([0, 1, 2, 3], [3, 4, 2, 4], [5, 6, 6, 5]), ([0, 1, 2, 3], [4, 2, 4, 3], [8, 10, 8, 9])]
SCRIPT3 = [(live[:3], counts[:3], at[:3]) for live, counts, at in SCRIPT4]
# the drop patterns of the emulator test on those batches.  Slot 0: its part of a batch (one frame) all refused, and a refusal in
# mid-batch.  Slot 1: a run that ends a batch and begins the next.  Slot 2: a run longer than the hold (its part of a batch all
# refused), then good frames.  Slot 3: no good frame yet for two batches, and a refusal in mid-batch.
DROPS = [[4, 9], [5, 6, 7], [3, 4, 5, 6, 7], [0, 1, 6]]
CONCEALED = [[4, 9], [5, 6, 7], [3, 4, 5], [6]]                 # what the rule makes of them at a hold of 3
S3_GROUPS = [g for g in GROUPS if g[2] == 3]


def members(streams, names, C_):
    names = names.split("+")
    mem = members_of(streams, names, 4 // len(names) if C_ <= 2 else 3)
    return mem[:4] if C_ <= 2 else mem[:3]


def feed(mem, drops):
    """-> (bytes, bases, frame tables with the dropped entries cut)"""
    data = np.concatenate([m[0] for m in mem])
    bases = np.cumsum([0] + [len(m[0]) for m in mem])[:-1]
    tables = [kit.dropped(m[1], drops[s]) if drops else m[1].copy() for s, m in enumerate(mem)]
    return data, bases, tables


def pipe_run(mem, script, C_, drops, conceal=True, i16=False, reset=None, way="pinned", **kw):
    """the script on a pipeline with device plans and five lanes, every batch submitted before the first is collected ->
    (per-stream PCM, per-stream results, refusals in all, concealed frames in all)"""
    S = len(mem)
    data, bases, tables = feed(mem, drops)
    if i16:
        kw["output_kind"] = aacgpu.OUTPUT_I16
    p = aacgpu.Pipeline(channels=C_, max_streams=S, max_frames=4, sample_index=3, device_plans=True, lanes=5,
                        conceal=dict(fade_steps=FADE, hold_frames=HOLD) if conceal else None, **kw)
    elem, per = np.int16 if i16 else np.float32, 1024 * C_
    got, results, refusals, pending, outs = [[] for _ in range(S)], [[] for _ in range(S)], 0, [], []
    for b, (live, counts, at) in enumerate(script):
        for s in (reset or {}).get(b, []):
            outs += [p.collect(t) for t in pending]
            pending = []
            p.reset_stream(s)
        fr = packed([tables[s] for s in live], [bases[s] for s in live], at, counts)
        slots, cnt = np.array(live, np.uint32), np.array(counts, np.uint32)
        if way == "planar":
            t, lengths, res, refused = p.decode_tensor(data, fr, slots, cnt, planar=True)
            host = t.cpu().numpy()
            assert not any(host[k, :, counts[k] * 1024:].view(np.uint16 if i16 else np.uint32).any() for k in range(len(live))), "the padding is not zero"
            flat = np.concatenate([np.ascontiguousarray(host[k, :, :counts[k] * 1024].T).reshape(-1) for k in range(len(live))])
            outs.append((flat, res, refused))
        else:
            pending.append(p.submit(data, fr, slots, cnt, pcm=p.pinned(int(sum(counts)) * per, elem)))
    outs += [p.collect(t) for t in pending]
    for (live, counts, at), (pcm, res, refused) in zip(script, outs):
        refusals += refused
        first = np.concatenate([[0], np.cumsum(counts)])
        for k, s in enumerate(live):
            got[s].append(pcm[first[k] * per:first[k + 1] * per].copy())
            results[s].append(res[first[k]:first[k + 1]].copy())
    concealed = p.concealed() if conceal else 0
    p.close()
    return [np.concatenate(g) for g in got], [np.concatenate(r) for r in results], refusals, concealed


def host_run(mem, script, C_, drops, oracle=None, reset=None, **kw):
    """the script on the yardstick -> (per-stream PCM, per-stream oracle PCM or None, the route, closed)"""
    S = len(mem)
    data, bases, tables = feed(mem, drops)
    host = kit.ConcealRoute(S, C_, 3, FADE, HOLD, oracle, **kw)
    want, ref, per = [[] for _ in range(S)], [[] for _ in range(S)], 1024 * C_
    for b, (live, counts, at) in enumerate(script):
        for s in (reset or {}).get(b, []):
            host.reset(s)
        fr = packed([tables[s] for s in live], [bases[s] for s in live], at, counts)
        pcm, r, _ = host.decode(data, fr, live, counts)
        first = np.concatenate([[0], np.cumsum(counts)])
        for k, s in enumerate(live):
            want[s].append(pcm[first[k] * per:first[k + 1] * per])
            if r is not None:
                ref[s].append(r[first[k] * per:first[k + 1] * per])
    host.close()
    return [np.concatenate(w) for w in want], [np.concatenate(r) for r in ref] if oracle is not None else None, host


def exactly_the_dropped(results, drops, what):
    for s, res in enumerate(results):
        assert np.flatnonzero(res["status"]).tolist() == sorted(drops[s]), "%s: stream %d's refused frames are not exactly the dropped ones" % (what, s)


CASES = [(g, True) for g in S3_GROUPS] + [(S3_GROUPS[1], False)]


@pytest.mark.parametrize("group,carry", CASES, ids=["%s-%s" % (g[0], "carry" if c else "sine") for g, c in CASES])
def test_concealed_pcm_equals_the_host_route_bit_for_bit_and_the_oracle(streams, oracle, group, carry):
    """mono, stereo (with and without the carried window shape) and 5.1: the drop patterns of the emulator test — mid-batch, a
    batch's first frame, a run across two batches, a run longer than the hold, a stream's part of a batch all refused, no good frame
    yet — with four batches in flight on five lanes"""
    names, C_, si = group
    mem = members(streams, names, C_)
    S = len(mem)
    script, drops = (SCRIPT4, DROPS) if S == 4 else (SCRIPT3, DROPS[:3])
    assert all(12 - len(d) >= 7 for d in drops)
    want, ref, host = host_run(mem, script, C_, drops, oracle, carry=carry)
    got, results, refusals, concealed = pipe_run(mem, script, C_, drops, carry_window_shape=carry)
    exactly_the_dropped(results, drops, "the pipeline")
    assert refusals == host.refused == sum(len(d) for d in drops)
    for s in range(S):
        assert np.array_equal(results[s]["status"], np.concatenate(host.statuses[s]))
        marked = np.flatnonzero(results[s]["flags"] & aacgpu.PARSE_CONCEALED).tolist()
        assert marked == CONCEALED[s] == np.flatnonzero(np.concatenate(host.flags[s]) & aacgpu.PARSE_CONCEALED).tolist(), "stream %d" % s
        assert same_bits(got[s], want[s]), "stream %d: the device's concealed frames decode to other bits than the rule's" % s
    assert concealed == host.concealed == sum(len(c) for c in CONCEALED[:S])
    close_to(np.concatenate(got), np.concatenate(ref))


def test_int16_output_and_pcm_left_on_the_device(streams):
    """AACG_OUTPUT_I16 against the int16 host route, and the same feed into a planar tensor on the device: the same bits"""
    names, C_, si = S3_GROUPS[1]
    mem = members(streams, names, C_)
    want, _, host = host_run(mem, SCRIPT4, C_, DROPS, i16=True)
    got, results, refusals, concealed = pipe_run(mem, SCRIPT4, C_, DROPS, i16=True, carry_window_shape=True)
    planar = pipe_run(mem, SCRIPT4, C_, DROPS, i16=True, carry_window_shape=True, way="planar")
    exactly_the_dropped(results, DROPS, "int16")
    for s in range(4):
        assert got[s].dtype == np.int16 and same_bits(got[s], want[s]), "stream %d, int16" % s
        assert same_bits(planar[0][s], want[s]), "stream %d, planar on the device" % s
        assert np.array_equal(planar[1][s], results[s])
    assert concealed == planar[3] == host.concealed and refusals == planar[2]


def test_behind_mix_and_resampler(streams):
    """stereo mixed to mono and resampled 48 -> 16 kHz behind the stage: the resample kit's rule over the mix kit's rule over the
    yardstick's PCM, bit for bit — the exit stages see the concealed PCM"""
    names, C_, si = S3_GROUPS[1]
    mem = members(streams, names, C_)
    mix, rs = aacgpu.mix_standard(2, 1), aacgpu.resample_design(48000, 16000, 32)
    want, _, host = host_run(mem, SCRIPT4, C_, DROPS, carry=False)
    data, bases, tables = feed(mem, DROPS)
    p = aacgpu.Pipeline(channels=C_, max_streams=4, max_frames=4, sample_index=3, device_plans=True, lanes=5, mix=mix, resample=rs,
                        conceal=dict(fade_steps=FADE, hold_frames=HOLD))
    got = [[] for _ in range(4)]
    for live, counts, at in SCRIPT4:
        fr = packed([tables[s] for s in live], [bases[s] for s in live], at, counts)
        pcm, res, refused, lengths = p.decode(data, fr, np.array(live, np.uint32), np.array(counts, np.uint32))
        for k, part in enumerate(np.split(pcm[:int(lengths.sum())], np.cumsum(lengths)[:-1])):
            got[live[k]].append(part.copy())
    assert p.concealed() == host.concealed
    p.close()
    for s in range(4):
        rule = resample_kit.resample_rule(mix_kit.mix_rule(want[s].reshape(-1, C_), mix), rs[0], rs[1], rs[2])
        assert same_bits(np.concatenate(got[s]).reshape(-1, 1), rule.reshape(-1, 1)), "stream %d" % s


def test_results_and_refusals_are_those_without_the_stage_and_a_clean_feed_is_untouched(streams):
    """the same script without the stage: every result record and the refusal count identical apart from the new flag bit, and the
    frames that are neither dropped nor behind a dropped frame the same bits; with the stage set and nothing dropped the PCM is
    bit-identical to the pipeline without it and nothing is counted"""
    names, C_, si = S3_GROUPS[1]
    mem = members(streams, names, C_)
    with_, without = pipe_run(mem, SCRIPT4, C_, DROPS), pipe_run(mem, SCRIPT4, C_, DROPS, conceal=False)
    assert with_[2] == without[2] == sum(len(d) for d in DROPS) and without[3] == 0
    for s in range(4):
        a, b = with_[1][s].copy(), without[1][s]
        assert not (b["flags"] & aacgpu.PARSE_CONCEALED).any() and np.count_nonzero(a["flags"] & aacgpu.PARSE_CONCEALED) == len(CONCEALED[s])
        a["flags"] &= 0xff ^ aacgpu.PARSE_CONCEALED
        assert a.tobytes() == b.tobytes(), "stream %d: a result differs by more than the flag bit" % s
        x, y = with_[0][s].reshape(12, -1), without[0][s].reshape(12, -1)
        for f in range(12):
            near = any(d in DROPS[s] for d in (f - 1, f))
            assert near or same_bits(x[f], y[f]), "stream %d frame %d: far from any dropped frame and yet other bits" % (s, f)
            if f in CONCEALED[s]:
                assert not same_bits(x[f], y[f])
    clean_with, clean_without = pipe_run(mem, SCRIPT4, C_, None), pipe_run(mem, SCRIPT4, C_, None, conceal=False)
    assert clean_with[2] == clean_with[3] == 0
    for s in range(4):
        assert same_bits(clean_with[0][s], clean_without[0][s]) and clean_with[1][s].tobytes() == clean_without[1][s].tobytes()


def test_a_reset_between_batches(streams):
    """slot 1 is reset in front of the third batch, whose first two frames of that slot are dropped: they stay silent — the frame the
    slot held belongs to the stream that left — while the host route, reset alike, agrees bit for bit"""
    names, C_, si = S3_GROUPS[1]
    mem = members(streams, names, C_)
    drops = [[], [6, 7], [1], [9]]
    want, _, host = host_run(mem, SCRIPT4, C_, drops, reset={2: [1]})
    got, results, refusals, concealed = pipe_run(mem, SCRIPT4, C_, drops, reset={2: [1]}, carry_window_shape=True)
    exactly_the_dropped(results, drops, "with a reset")
    assert [np.flatnonzero(r["flags"] & aacgpu.PARSE_CONCEALED).tolist() for r in results] == [[], [], [1], [9]] and concealed == host.concealed == 2
    for s in range(4):
        assert same_bits(got[s], want[s]), "stream %d" % s
    assert not got[1].reshape(12, -1)[6].any(), "a silent frame in front of a fresh overlap state"


def test_set_concealment_refusals(streams):
    """every refusal that needs a live pipeline leaves it as it was: plan mode 0 and the spec stages are unsupported, parameters out of
    range, a second call and a call after the first batch invalid"""
    names, C_, si = S3_GROUPS[1]
    mem = members(streams, names, C_)[:1]
    data, bases, tables = feed(mem, None)
    for kw, code, word in ((dict(device_plans=False), ERR_UNSUPPORTED, "plan_mode 0"), (dict(device_plans=True, tns_spec=True), ERR_UNSUPPORTED, "AACG_PIPELINE_STAGE_TNS"),
                           (dict(device_plans=True, pns_spec=True), ERR_UNSUPPORTED, "AACG_PIPELINE_STAGE_PNS")):
        with pytest.raises(aacgpu.AacgError) as e:
            aacgpu.Pipeline(channels=2, max_streams=1, max_frames=4, conceal=True, **kw)
        assert e.value.code == code and word in str(e.value), str(e.value)
    p = aacgpu.Pipeline(channels=2, max_streams=1, max_frames=4, device_plans=True)
    for bad in (dict(fade_steps=65), dict(hold_frames=0), dict(hold_frames=256)):
        with pytest.raises(aacgpu.AacgError) as e:
            p.set_concealment(**bad)
        assert e.value.code == ERR_INVALID_ARG and p.conceal is None
    assert p.lib.aacg_pipeline_set_concealment(p.handle, None) == ERR_INVALID_ARG
    p.set_concealment(fade_steps=0, hold_frames=255)
    with pytest.raises(aacgpu.AacgError) as e:
        p.set_concealment()
    assert e.value.code == ERR_INVALID_ARG and "already" in str(e.value)
    fr = packed([kit.dropped(tables[0], [1])], [0], [0], [4])
    pcm, res, refused = p.decode(data, fr, np.array([0], np.uint32), np.array([4], np.uint32))
    assert refused == 1 and res["flags"][1] & aacgpu.PARSE_CONCEALED and p.concealed() == 1
    p.close()
    q = aacgpu.Pipeline(channels=2, max_streams=1, max_frames=4, device_plans=True)
    q.decode(data, packed([tables[0]], [0], [0], [2]), np.array([0], np.uint32), np.array([2], np.uint32))
    with pytest.raises(aacgpu.AacgError) as e:
        q.set_concealment()
    assert e.value.code == ERR_INVALID_ARG and "before the first" in str(e.value)
    q.close()
