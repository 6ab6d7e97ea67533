"""The gain and look-ahead limiter on the resident route (aacg_pipeline_set_limiter, aacg_pipeline_set_gain, aacgpu.Pipeline(limiter=...))
on a real MI355X.  A script of ragged batches is decoded by a pipeline WITHOUT the stage; the rule of include/aacgpu.h in numpy float32
(limiter_kit.rule) is applied to that PCM per slot, batch after batch, with the gains as they stood when each batch was enqueued; the same
script on a pipeline WITH the stage must deliver those bits.  The ceiling is taken from the unlimited decode itself, half its largest
sample, so that the stage demonstrably engages — asserted on the kit's result.  Host memory page-locked and pageable, device memory
packed and planar; f32 and int16; stereo, mono and 5.1 through the standard downmix; a reset in mid-run, gains set between batches in
flight, a refused frame and an unlearnt stream; beside the mix, the resampler, the feature stage and the meter; the refusals.
Six frames a stream, batches of at most 3 frames, two lanes, every batch submitted before the one before it is collected."""
import ctypes as C

import numpy as np
import pytest

import aacgpu
import features_kit
import limiter_kit as kit
import loudness_kit
import mix_kit
import resample_kit
from resident_kit import CASES, ERR_INVALID_ARG, load, packed, ragged_script, same_bits

pytestmark = pytest.mark.gpu
CASE = {c["name"]: c for c in CASES}
F = np.float32
WAYS = ["pinned", "pageable", "packed", "planar"]
RELEASE = 0.0625
I16_POISON = 0x7F7F


def committed(name, copies, frames=6):
    """`frames` frames of a committed stream, its own in rotation where it has fewer; each copy starts a frame later"""
    c = CASE[name]
    data, table, _ = load(c)
    return [(data, table[(np.arange(frames) + k) % len(table)]) for k in range(copies)], c["channels"], c["sampleIndex"]


def run(mem, script, C_, si, way="pageable", i16=False, limiter=None, gains=None, gain_at=None, reset=None, mix=None, resample=None,
        features=None, loudness=None, lanes=2):
    """the script on a pipeline with or without the stage -> dict(out: per stream (rows, width) of what left, status, refusals, counts,
    records: the meter's per stream or None).  gains: {slot: G} set before the first batch; gain_at: {batch: {slot: G}} set in front of
    that batch while the one before it is in flight; reset: {batch: slots reset in front of it}"""
    import torch
    S = len(mem)
    data = np.concatenate([m[0] for m in mem])
    bases = np.cumsum([0] + [len(m[0]) for m in mem])[:-1]
    tables = [m[1] for m in mem]
    kw = dict(output_kind=aacgpu.OUTPUT_I16) if i16 else {}
    p = aacgpu.Pipeline(channels=C_, max_streams=S, max_frames=3, sample_index=si, mix=mix, resample=resample, features=features, loudness=loudness,
                        limiter=limiter, lanes=lanes, **kw)
    width = p.features["n_mels"] if features else p.channels
    dtype = np.float32 if features or not i16 else np.int16
    for slot, g in (gains or {}).items():
        p.set_gain(slot, g)
    out = dict(out=[[] for _ in range(S)], status=[[] for _ in range(S)], refusals=0, records=[[] for _ in range(S)] if loudness else None)
    pending = []

    def finish(item):
        ticket, live, counts, n_out, buf = item
        recs = p.take_loudness(ticket) if loudness else None
        back, res, refused, *_ = p.collect(ticket)
        assert back is buf
        host = buf if way in ("pinned", "pageable") else buf.cpu().numpy()
        total, first = sum(n_out), np.concatenate([[0], np.cumsum(counts)])
        if way == "planar":
            parts = [np.ascontiguousarray(host[k, :, :n_out[k]].T) for k in range(len(live))]
        else:
            tail = host[total * width:]
            assert (np.isnan(tail).all() if dtype == np.float32 else (tail == I16_POISON).all()), "the elements behind the batch were written"
            parts = [x.reshape(-1, width) for x in np.split(host[:total * width].copy(), np.cumsum(n_out)[:-1] * width)]
        out["refusals"] += refused
        for k, s in enumerate(live):
            out["out"][s].append(parts[k])
            out["status"][s].append(res["status"][first[k]:first[k + 1]].copy())
            if loudness:
                out["records"][s].append(recs[k])

    for b, (live, counts, at) in enumerate(script):
        for s in (reset or {}).get(b, []):
            for item in pending:
                finish(item)
            pending = []
            p.reset_stream(s)
        for slot, g in (gain_at or {}).get(b, {}).items():
            p.set_gain(slot, g)                                   # (the batch before is in flight: its gain went up with it)
        fr = packed([tables[s] for s in live], [bases[s] for s in live], at, counts)
        slots, cnt = np.array(live, np.uint32), np.array(counts, np.uint32)
        n_out = [int(v) for v in (p.out_samples(slots, cnt) if resample or features else cnt.astype(np.int64) * 1024)]
        total = sum(n_out)
        if way in ("pinned", "pageable"):
            buf = p.pinned(((total + 64) * width,), dtype) if way == "pinned" else np.empty((total + 64) * width, dtype)
            buf[:] = np.nan if dtype == np.float32 else I16_POISON
            t = p.submit(data, fr, slots, cnt, pcm=buf)
        else:
            planar = way == "planar"
            stride = max(n_out) if features else (max(n_out) + 1023) // 1024
            shape = (len(live), width, max(n_out) if features else stride * 1024) if planar else ((total + 64) * width,)
            buf = torch.full(shape, I16_POISON, dtype=torch.int16, device="cuda") if dtype == np.int16 else torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()                              # the fill is torch's stream's, the batch a lane's
            t = p.submit_device(data, fr, slots, cnt, buf, planar=planar, stride_frames=stride if planar else None)
        pending.append((t, live, counts, n_out, buf))
        if len(pending) == 2:
            finish(pending.pop(0))
    for item in pending:
        finish(item)
    out["counts"] = p.launch_counts()
    out["gains"] = [p.gain(s) for s in range(S)] if limiter else None
    p.close()
    out["out"] = [np.concatenate(g) for g in out["out"]]
    return out


def ruled(plain, script, c, gains, gain_at=None, reset=None):
    """per stream: the rule over the unlimited run's PCM, batch after batch as the script cuts it, with the gains as they stood when each
    batch was enqueued and the slots reset where the script says -> (what must leave per stream, the kit's states)"""
    S = len(plain)
    width = plain[0].shape[1]
    G = [F(1.0)] * S
    for slot, g in gains.items():
        G[slot] = F(g)
    states, done, out = [kit.State(width) for _ in range(S)], [0] * S, [[] for _ in range(S)]
    seen = []
    for b, (live, counts, at) in enumerate(script):
        for s in (reset or {}).get(b, []):
            seen.append(states[s])
            states[s] = kit.State(width)
        for slot, g in (gain_at or {}).get(b, {}).items():
            G[slot] = F(g)
        for s, n in zip(live, counts):
            out[s].append(kit.rule(plain[s][done[s]:done[s] + 1024 * n], G[s], c, RELEASE, states[s]))
            done[s] += 1024 * n
    return [np.concatenate(o) for o in out], states + seen


def ceiling_of(plain):
    """half the unlimited decode's largest sample, in full-scale units"""
    peak = max(float(np.abs(x.astype(np.float64)).max()) for x in plain)
    c = F(0.5 * peak / (32768.0 if plain[0].dtype == np.int16 else 1.0))
    assert c > 0
    return c


def engaged(states):
    under, at = zip(*[s.engaged() for s in states])
    assert sum(under) > 0 and sum(at) > 0, "the kit never limited, or always: the case does not test what it is for"


def same_out(got, want, what):
    for s, (x, y) in enumerate(zip(got, want)):
        assert x.shape == y.shape and x.dtype == y.dtype, (what, s, x.shape, y.shape, x.dtype, y.dtype)
        view = np.uint16 if x.dtype == np.int16 else np.uint32
        wrong = np.argwhere(np.ascontiguousarray(x).view(view) != np.ascontiguousarray(y).view(view))
        assert wrong.size == 0, "%s: stream %d differs from the rule over the unlimited pipeline's PCM at %d of %d values, first at %s: %r against %r" % (
            what, s, len(wrong), y.size, wrong[0], x[tuple(wrong[0])], y[tuple(wrong[0])])


# (stream, the mix)
SETUPS = {"stereo": ("stereo48", None), "mono": ("mono22", None), "surround-to-stereo": ("surround48", lambda: aacgpu.mix_standard(6, 2))}
_plain = {}


def plain_run(case, i16):
    """the yardstick, once per configuration: two slots, seeded ragged batches of at most 3 frames, decoded WITHOUT the stage; the ways and
    the tests share it and leave it unchanged"""
    key = (case, i16)
    if key not in _plain:
        name, make_mix = SETUPS[case]
        mem, C_, si = committed(name, 2)
        script = ragged_script([m[1] for m in mem], 3, np.random.default_rng(17))
        assert len(script) >= 3, "three or more submissions on two lanes: lanes are reused"
        mix = make_mix() if make_mix else None
        plain = run(mem, script, C_, si, i16=i16, mix=mix)
        _plain[key] = dict(mem=mem, C=C_, si=si, script=script, mix=mix, plain=plain, c=ceiling_of(plain["out"]))
    return _plain[key]


@pytest.mark.parametrize("way", WAYS)
@pytest.mark.parametrize("i16", [False, True], ids=["f32", "i16"])
@pytest.mark.parametrize("case", sorted(SETUPS))
def test_the_rule_through_the_abi(case, i16, way):
    """G = 1 for one stream, G = 4 for the other, the ceiling half the unlimited decode's peak: bit for bit the kit over the unlimited PCM"""
    P = plain_run(case, i16)
    gains = {0: 1.0, 1: 4.0}
    want, states = ruled(P["plain"]["out"], P["script"], P["c"], gains)
    engaged(states)
    got = run(P["mem"], P["script"], P["C"], P["si"], way=way, i16=i16, mix=P["mix"], limiter=(P["c"], RELEASE), gains=gains)
    same_out(got["out"], want, "%s, %s, %s" % (case, "i16" if i16 else "f32", way))
    for x, y in zip(got["status"], P["plain"]["status"]):
        assert np.array_equal(np.concatenate(x), np.concatenate(y))
    assert got["refusals"] == P["plain"]["refusals"] and got["counts"] == P["plain"]["counts"] and got["gains"] == [1.0, 4.0]
    if not i16:
        lim = float(P["c"]) * (1 + 2.0 ** -21)
        assert max(float(np.abs(x.astype(np.float64)).max()) for x in got["out"]) <= lim, "consequence (a) of the rule"


@pytest.mark.parametrize("way", ["pageable", "packed"])
def test_a_reset_in_mid_run(way):
    """aacg_pipeline_reset_stream(0) in front of the third batch: from there on slot 0 leaves as a new stream does — a block of zeros first,
    a0 = th = G — with the gain it had, while slot 1 goes on"""
    P = plain_run("stereo", False)
    reset, gains = {2: [0]}, {0: 3.0, 1: 4.0}
    plain = run(P["mem"], P["script"], 2, P["si"], reset=reset)
    want, states = ruled(plain["out"], P["script"], P["c"], gains, reset=reset)
    engaged(states)
    got = run(P["mem"], P["script"], 2, P["si"], way=way, limiter=(P["c"], RELEASE), gains=gains, reset=reset)
    same_out(got["out"], want, way)
    cut = sum(n for live, counts, at in P["script"][:2] for s, n in zip(live, counts) if s == 0) * 1024
    assert plain["out"][0][cut - 64:cut].any(), "the block held at the reset was music: it must not leave"
    assert not got["out"][0][cut:cut + 64].any() and got["out"][0][cut + 64:].any() and got["gains"] == [3.0, 4.0]


@pytest.mark.parametrize("i16", [False, True], ids=["f32", "i16"])
def test_a_gain_set_between_batches_in_flight(i16):
    """set_gain while the batch before is in flight: that batch keeps the gain it was enqueued with, the next one has the new — up for
    one slot, down for the other, then to 0"""
    P = plain_run("stereo", i16)
    assert len(P["script"]) >= 4
    gains, gain_at = {0: 1.0, 1: 4.0}, {1: {0: 6.0}, 2: {1: 0.5}, 3: {0: 0.0}}
    want, states = ruled(P["plain"]["out"], P["script"], P["c"], gains, gain_at=gain_at)
    engaged(states)
    got = run(P["mem"], P["script"], 2, P["si"], way="pinned", i16=i16, limiter=(P["c"], RELEASE), gains=gains, gain_at=gain_at)
    same_out(got["out"], want, "gains in flight")
    assert got["gains"] == [0.0, 0.5]


@pytest.mark.parametrize("way", ["pageable", "planar"])
def test_a_refused_frame_and_an_unlearnt_stream(way):
    """three 5.1 streams — one clean, one whose first frame is malformed (no layout is learnt in the first batch: its frames there are
    zeros), one with a malformed frame behind a learnt layout (a refused frame: zeros between music).  The zeros pass like any other"""
    c = CASE["surround48"]
    data, table, _ = load(c)

    def broken(at):
        bad = data.copy()
        off, length = int(table[at]["byte_offset"]), int(table[at]["byte_length"])
        bad[off + 7: off + length] = 0xFF                      # a raw_data_block with none of the stream's elements in it
        return bad

    mem = [(data, table), (broken(0), table), (broken(2), table)]
    script = [([0, 1, 2], [2, 1, 3], [0, 0, 0]), ([0, 1, 2], [2, 3, 1], [2, 1, 3]), ([0, 1, 2], [1, 1, 1], [4, 4, 4])]
    plain = run(mem, script, 6, c["sampleIndex"])
    status = [np.concatenate(x) for x in plain["status"]]
    assert plain["refusals"] >= 2 and status[1][0] != 0 and status[2][2] != 0 and not status[0].any(), status
    assert not plain["out"][1][:1024].any() and plain["out"][2][:2048].any()       # (the refused frame's samples are the overlap's tail, then nothing)
    ceil, gains = ceiling_of(plain["out"]), {0: 1.0, 1: 2.0, 2: 4.0}
    want, states = ruled(plain["out"], script, ceil, gains)
    engaged(states)
    got = run(mem, script, 6, c["sampleIndex"], way=way, limiter=(ceil, RELEASE), gains=gains)
    same_out(got["out"], want, way)
    assert got["refusals"] == plain["refusals"] and not got["out"][1][:1024 + 64].any()


def test_beside_mix_resampler_and_meter():
    """mix + limiter + resampler + meter: the PCM is the resampler's rule over the kit over the mixed PCM, per slot over the whole run; the
    meter taps the transform in front of all this, so its records are those of the same pipeline without the limiter"""
    P = plain_run("stereo", False)
    mix, rs = mix_kit.hostile_matrix(2, 2), aacgpu.resample_design(48000, 16000, 32)
    meter = {"hop": 1000, "coeffs": loudness_kit.hostile_coeffs(3)}
    mixed = run(P["mem"], P["script"], 2, P["si"], mix=mix)
    ceil, gains = ceiling_of(mixed["out"]), {0: 1.0, 1: 4.0}
    limited, states = ruled(mixed["out"], P["script"], ceil, gains)
    engaged(states)
    want = [resample_kit.resample_rule(x, rs[0], rs[1], rs[2]) for x in limited]
    bare = run(P["mem"], P["script"], 2, P["si"], way="packed", mix=mix, resample=rs, loudness=meter)
    got = run(P["mem"], P["script"], 2, P["si"], way="packed", mix=mix, resample=rs, loudness=meter, limiter=(ceil, RELEASE), gains=gains)
    same_out(got["out"], want, "mix + limiter + resampler")
    for x, y in zip(got["records"], bare["records"]):
        assert same_bits(np.concatenate(x), np.concatenate(y)) and len(np.concatenate(x)) == 6, "the meter's records differ with the limiter"
    assert got["counts"] == bare["counts"] and not same_bits(got["out"][1], bare["out"][1])


def test_beside_mix_resampler_and_features(tmp_path_factory):
    """mix(-> 1) + limiter + resampler + features: the feature frames are the feature rule over the resampler's rule over the kit over
    the mixed mono PCM (linear output: bit for bit)"""
    lib = features_kit.driver(tmp_path_factory.mktemp("features_emu"))
    P = plain_run("stereo", False)
    mix, rs = aacgpu.mix_standard(2, 1), aacgpu.resample_design(48000, 16000, 32)
    basis, fb = features_kit.hostile_tables(64, 33, 5)
    features = dict(frame_length=64, hop=24, pad_left=17, basis=basis, fb=fb, floor=1e-3, log=False)
    mixed = run(P["mem"], P["script"], 2, P["si"], mix=mix)
    ceil, gains = ceiling_of(mixed["out"]), {0: 1.0, 1: 4.0}
    limited, states = ruled(mixed["out"], P["script"], ceil, gains)
    engaged(states)
    want = [features_kit.rule(lib, resample_kit.resample_rule(x, rs[0], rs[1], rs[2])[:, 0], 64, 24, 17, basis, fb) for x in limited]
    for way in ("pageable", "planar"):
        got = run(P["mem"], P["script"], 2, P["si"], way=way, mix=mix, resample=rs, features=features, limiter=(ceil, RELEASE), gains=gains)
        same_out(got["out"], want, "mix + limiter + resampler + features, %s" % way)


def test_refusals_leave_the_pipeline_as_it_was():
    """aacg_pipeline_set_limiter: a null config, a ceiling or release outside the limits, a second call, a call after the first batch;
    aacg_pipeline_set_gain and aacg_pipeline_gain: no limiter, a slot out of range, a gain outside 0..1024 or not finite; a mix behind the
    limiter.  Each is refused with a reason, and a pipeline whose set_limiter was refused decodes the bits of one that never called it"""
    data, table, _ = load(CASE["stereo48"])
    fr = [packed([table] * 2, [0, 0], [a, a], [3, 3]) for a in (0, 3)]
    slots = np.arange(2, dtype=np.uint32)
    fresh = aacgpu.Pipeline(channels=2, max_streams=2, max_frames=3)
    want = [fresh.decode(data, f, slots, 3)[0].copy() for f in fr]
    launches = fresh.launch_counts()
    fresh.close()

    def refused(p, cfg):
        rc = p.lib.aacg_pipeline_set_limiter(p.handle, None if cfg is None else C.byref(aacgpu.LimiterConfig(*cfg)))
        assert rc == ERR_INVALID_ARG, (cfg, rc)
        reason = p.lib.aacg_pipeline_last_error(p.handle).decode()
        assert reason.startswith("aacg_pipeline_set_limiter: ") and len(reason) > 35, reason
        return reason

    p = aacgpu.Pipeline(channels=2, max_streams=2, max_frames=3)
    reasons = [refused(p, None)] + [refused(p, (c, 0.5)) for c in (0.0, -1.0, np.inf, np.nan)] + [refused(p, (0.5, r)) for r in (0.0, -0.5, 1.0001, np.inf, np.nan)]
    assert len(set(reasons)) == 3
    g = C.c_float(7.0)
    assert p.lib.aacg_pipeline_set_gain(p.handle, 0, 2.0) == ERR_INVALID_ARG and "no limiter" in p.lib.aacg_pipeline_last_error(p.handle).decode()
    assert p.lib.aacg_pipeline_gain(p.handle, 0, C.byref(g)) == ERR_INVALID_ARG and g.value == 7.0
    assert same_bits(p.decode(data, fr[0], slots, 3)[0], want[0])
    assert "submitted" in refused(p, (0.5, 0.5))                        # after the first batch
    assert same_bits(p.decode(data, fr[1], slots, 3)[0], want[1]) and p.launch_counts() == launches
    p.close()

    p = aacgpu.Pipeline(channels=2, max_streams=2, max_frames=3, limiter=(8.0, 0.5))
    assert (p.limiter.ceiling, p.limiter.release) == (8.0, 0.5)
    assert "already" in refused(p, (0.5, 0.5))                          # a second call
    with pytest.raises(aacgpu.AacgError, match="limiter already"):
        p.set_mix(aacgpu.mix_standard(2, 1))                            # the mix is set before the limiter
    assert p.channels == 2 and p.gain(0) == 1.0 and p.gain(1) == 1.0
    p.set_gain(1, 1024.0)
    p.set_gain(0, 0.0)
    for slot, gain in ((2, 1.0), (0, -0.5), (0, 1024.5), (0, np.inf), (0, np.nan)):
        assert p.lib.aacg_pipeline_set_gain(p.handle, slot, gain) == ERR_INVALID_ARG, (slot, gain)
        assert p.lib.aacg_pipeline_last_error(p.handle).decode().startswith("aacg_pipeline_set_gain: ")
    assert p.lib.aacg_pipeline_gain(p.handle, 2, C.byref(g)) == ERR_INVALID_ARG and p.lib.aacg_pipeline_gain(p.handle, 0, None) == ERR_INVALID_ARG
    assert (p.gain(0), p.gain(1)) == (0.0, 1024.0)
    p.set_gain(0, 1.0)
    p.set_gain(1, 0.25)
    # far below the ceiling: gain 1 is the decode delayed by one block, gain 0.25 a quarter of it, exactly
    got = p.decode(data, fr[0], slots, 3)[0].reshape(2, 3 * 1024, 2)
    plain = want[0].reshape(2, 3 * 1024, 2)
    assert np.abs(plain).max() < 8.0
    assert same_bits(got[0, 64:], plain[0, :-64]) and same_bits(got[1, 64:], plain[1, :-64] * F(0.25)) and not got[:, :64].any()
    p.reset_stream(1)
    assert p.gain(1) == 0.25, "the gain is the caller's: a reset leaves it"
    p.close()
