"""The loudness meter on the resident route (aacg_pipeline_set_loudness, aacgpu.Pipeline(loudness=...)) on a real MI355X.  Every
configuration runs twice, with and without the meter: with it, everything the pipeline delivered without it — every byte of every
destination buffer, poison behind the batch included, statuses, refusal counts, plan builds and launch counts — is bit-identical; and the
records equal, BIT FOR BIT, the rule of include/aacgpu.h as a plain numpy-float32 loop (loudness_kit.rule) over the transform PCM that a
pipeline without meter, mix or resampler delivers for the same script (resident_kit.run_script), per slot across the batches.  Hops of
1000 and 4800, batches of at most 3 frames, at most 3 streams."""
import ctypes as C

import numpy as np
import pytest

import aacgpu
import loudness_kit as kit
import mix_kit
from resident_kit import CASES, ERR_CAPACITY, ERR_INVALID_ARG, load, packed, ragged_script, run_script, same_bits

pytestmark = pytest.mark.gpu
CASE = {c["name"]: c for c in CASES}
I16_POISON = 0x7F7F
WAYS = ["host", "packed", "planar"]


def poison_host(a):
    a[:] = I16_POISON if a.dtype == np.int16 else np.nan
    return a


def poisoned_device(shape, i16):
    import torch
    t = torch.full(shape, I16_POISON, dtype=torch.int16, device="cuda") if i16 else torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()                                  # the fill is torch's stream's, the batch a lane's
    return t


def run(members, script, C_, si, device_plans, way, meter, i16=False, ahead=True, reset=None, lanes=2, **kw):
    """the script on a pipeline with or without a meter, the PCM delivered `way`; ahead: every batch is submitted before the first is
    collected; reset: {batch index: slots reset in front of it} -> dict(raw: every batch's whole destination buffer, status, refusals,
    builds, counts, records: per stream (n, C, 2) or None)"""
    S = len(members)
    data = np.concatenate([m[0] for m in members])
    bases = np.cumsum([0] + [len(m[0]) for m in members])[:-1]
    tables = [m[1] for m in members]
    if i16:
        kw["output_kind"] = aacgpu.OUTPUT_I16
    p = aacgpu.Pipeline(channels=C_, max_streams=S, max_frames=3, sample_index=si, device_plans=device_plans, lanes=lanes, loudness=meter, **kw)
    O, dtype = p.channels, np.int16 if i16 else np.float32
    out = dict(raw=[], status=[[] for _ in range(S)], refusals=0, records=[[] for _ in range(S)] if meter else None)
    clock, pending = [0] * S, []

    def finish(item):
        b, ticket, live, counts, buf, n_rec = item
        if meter and b % 2:                                    # the records first, which finishes the batch; the PCM is still collect's
            recs = p.take_loudness(ticket)
        back, res, refused, *_ = p.collect(ticket)
        if meter and not b % 2:
            recs = p.take_loudness(ticket)
        assert back is buf
        out["raw"].append(buf.copy() if way == "host" else buf.cpu().numpy())
        out["refusals"] += refused
        first = np.concatenate([[0], np.cumsum(counts)])
        for k, s in enumerate(live):
            out["status"][s].append(res["status"][first[k]:first[k + 1]].copy())
            if meter:
                assert recs[k].shape == (n_rec[k], C_, 2) and recs[k].dtype == np.float32
                out["records"][s].append(recs[k])

    for b, (live, counts, at) in enumerate(script):
        for s in (reset or {}).get(b, []):
            for item in pending:
                finish(item)
            pending = []
            p.reset_stream(s)
            clock[s] = 0
        fr = packed([tables[s] for s in live], [bases[s] for s in live], at, counts)
        slots, cnt = np.array(live, np.uint32), np.array(counts, np.uint32)
        n_out = [int(v) for v in (p.out_samples(slots, cnt) if p.resample else cnt.astype(np.int64) * 1024)]
        n_rec = [(clock[s] + 1024 * c) // meter["hop"] - clock[s] // meter["hop"] for s, c in zip(live, counts)] if meter else None
        if meter:
            assert p.loudness_counts(slots, cnt).tolist() == n_rec, "aacg_pipeline_loudness_counts against the formula"
        total = sum(n_out)
        if way == "host":
            buf = poison_host(np.empty((total + 64) * O, dtype))
            t = p.submit(data, fr, slots, cnt, pcm=buf)
        else:
            planar = way == "planar"
            stride = (max(n_out) + 1023) // 1024
            buf = poisoned_device((len(live) + 1, O, stride * 1024) if planar else ((total + 64) * O,), i16)
            t = p.submit_device(data, fr, slots, cnt, buf, planar=planar, stride_frames=stride if planar else None)
        for s, c in zip(live, counts):
            clock[s] += 1024 * c
        pending.append((b, t, live, counts, buf, n_rec))
        if not ahead:
            finish(pending.pop())
    for item in pending:
        finish(item)
    out["builds"], out["counts"] = p.plan_builds(), p.launch_counts()
    p.close()
    return out


def raw_bits(a):
    return np.ascontiguousarray(a).view(np.uint16 if a.dtype.itemsize == 2 else np.uint32)


def same_delivery(got, want, what):
    """with the meter everything else is what it was without: the destination buffers whole, statuses, refusals, builds, launch counts"""
    assert len(got["raw"]) == len(want["raw"]), what
    for b, (x, y) in enumerate(zip(got["raw"], want["raw"])):
        assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(raw_bits(x), raw_bits(y)), "%s: batch %d's destination differs with the meter" % (what, b)
    for x, y in zip(got["status"], want["status"]):
        assert np.array_equal(np.concatenate(x), np.concatenate(y)), what
    assert got["refusals"] == want["refusals"] and got["builds"] == want["builds"] and got["counts"] == want["counts"], what


def ruled(plain_pcm, C_, meter, cuts=None):
    """per stream: the rule over the plain pipeline's transform PCM; cuts: {stream: samples at which its slot was reset}"""
    out = []
    for s, x in enumerate(plain_pcm):
        pieces = np.split(x.reshape(-1, C_), (cuts or {}).get(s, []))
        out.append(np.concatenate([kit.rule(piece, meter["hop"], meter["coeffs"], kit.State(C_)) for piece in pieces]))
    return out


def same_as_rule(got, want_records, what):
    for s, (parts, y) in enumerate(zip(got["records"], want_records)):
        x = np.concatenate(parts)
        assert x.shape == y.shape, (what, s, x.shape, y.shape)
        wrong = np.argwhere(x.view(np.uint32) != y.view(np.uint32))
        assert wrong.size == 0, "%s: stream %d's records differ from the rule over the plain pipeline's PCM at %d of %d values, first at (hop, channel, e|peak) %s: %r against %r" % (
            what, s, len(wrong), y.size, wrong[0], x[tuple(wrong[0])], y[tuple(wrong[0])])


def committed(name, copies, frames=12):
    """`frames` frames of a committed stream, its own in rotation where it has fewer (any sequence of a stream's frames decodes)"""
    c = CASE[name]
    data, table, _ = load(c)
    return [(data, table[np.arange(frames) % len(table)])] * copies, c["channels"], c["sampleIndex"]


def bs1770(rate, hop):
    return aacgpu.loudness_design(rate, hop=hop)


def hostile(seed, hop):
    return {"hop": hop, "coeffs": kit.hostile_coeffs(seed)}


# stream, int16, the meter
SETUPS = {"stereo48-f32-hop1000-hostile": ("stereo48", False, lambda: hostile(3, 1000)),
          "stereo48-i16-hop4800-bs1770": ("stereo48", True, lambda: bs1770(48000, 4800)),
          "surround48-f32-hop4800-bs1770": ("surround48", False, lambda: bs1770(48000, 4800)),
          "surround48-i16-hop1000-hostile": ("surround48", True, lambda: hostile(4, 1000))}
_plain = {}


def plain_run(name, i16, mode=False, **kw):
    """the yardstick, once per stream, element type and options: two slots, seeded ragged batches of at most 3 frames, decoded by a pipeline
    without meter, mix or resampler; the ways and the tests share it (and leave it unchanged), and the rule over it per meter"""
    key = (name, i16, mode, tuple(sorted(kw)))
    if key not in _plain:
        mem, C_, si = committed(name, 2)
        script = ragged_script([m[1] for m in mem], 3, np.random.default_rng(11))
        assert len(script) >= 3, "three or more submissions on two lanes: lanes are reused"
        opts = dict(kw, **(dict(output_kind=aacgpu.OUTPUT_I16) if i16 else {}))
        _plain[key] = dict(mem=mem, C=C_, si=si, script=script, pcm=run_script(mem, script, C_, si, 3, mode, **opts)[0], ruled={})
    return _plain[key]


def expected(P, meter):
    key = (meter["hop"], meter["coeffs"].tobytes())
    if key not in P["ruled"]:
        P["ruled"][key] = ruled(P["pcm"], P["C"], meter)
    return P["ruled"][key]


@pytest.mark.parametrize("way", WAYS)
@pytest.mark.parametrize("case", sorted(SETUPS))
def test_records_are_the_rule_and_nothing_else_differs(case, way):
    """stereo and 5.1, f32 and int16, hostile sections and BS.1770's, hops of 1000 and 4800 (several batches emit nothing); ragged batches
    on two lanes, all submitted before the first is collected: every launch reads the state the one before it wrote on the other lane's
    stream.  Host memory; the caller's device memory packed — the transform writes it and the meter reads it —; and planar"""
    name, i16, make = SETUPS[case]
    meter, P = make(), plain_run(name, i16)
    want = run(P["mem"], P["script"], P["C"], P["si"], False, way, None, i16=i16)
    got = run(P["mem"], P["script"], P["C"], P["si"], False, way, meter, i16=i16)
    same_delivery(got, want, "%s, %s" % (case, way))
    same_as_rule(got, expected(P, meter), "%s, %s" % (case, way))
    total = sum(len(r) for r in got["records"][0])
    assert total == 12 * 1024 // meter["hop"] and np.concatenate(got["records"][0])[:, :, 0].max() > 0, "the streams are music"
    if meter["hop"] == 4800:
        assert any(len(r) == 0 for r in got["records"][0]), "a hop that spans batches: some emit nothing"
    assert got["counts"]["launches"] == len(P["script"])


def test_bs1770_over_music_integrates_to_a_plausible_level():
    """the Python surface end to end: design, Pipeline(loudness=), decode, take_loudness(), loudness_integrate — against the float64
    restatement over the same records"""
    P = plain_run("stereo48", False)
    data, table = P["mem"][0]
    p = aacgpu.Pipeline(channels=2, max_streams=1, max_frames=3, loudness=aacgpu.loudness_design(48000))
    recs = []
    for a in range(0, 12, 3):
        pcm, res, refused = p.decode(data, table[a:a + 3], [0], 3)
        recs += p.take_loudness()
    p.close()
    rec = np.concatenate(recs)
    assert rec.shape == (2, 2, 2)                                # 12288 samples: two hops of 4800 — fewer than four: no block
    assert np.isneginf(aacgpu.loudness_integrate(rec, 4800))
    x = P["pcm"][0].reshape(-1, 2)
    assert np.array_equal(rec[:, :, 1], np.abs(x[:9600]).reshape(2, 4800, 2).max(axis=1)), "peak is the hop's max |x|"
    fine = aacgpu.Pipeline(channels=2, max_streams=1, max_frames=3, loudness=aacgpu.loudness_design(48000, hop=1000))
    rec = np.concatenate([fine.decode(data, table[a:a + 3], [0], 3) and fine.take_loudness()[0] for a in range(0, 12, 3)])
    fine.close()
    got, want = aacgpu.loudness_integrate(rec, 1000), kit.integrate64(rec, 1000)[0]
    assert len(rec) == 12 and -70.0 < got < 0.0 and abs(got - want) <= 1e-9


@pytest.mark.parametrize("way", ["host", "packed"])
def test_a_reset_in_mid_run(way):
    """two lanes, two slots, the seeded script with aacg_pipeline_reset_stream(0) in front of the third batch: from there on slot 0's
    records are the rule over the frames since the reset from nothing, while slot 1 goes on"""
    P = plain_run("stereo48", False)
    script, meter = P["script"], hostile(8, 1000)
    cut = sum(c for live, counts, at in script[:2] for s, c in zip(live, counts) if s == 0) * 1024
    assert cut % 1000 != 0, "the reset falls in mid-hop"

    def plain():
        """(the transform PCM with the same reset: the overlap starts again too)"""
        mem, data = P["mem"], np.concatenate([m[0] for m in P["mem"]])
        bases = np.cumsum([0] + [len(m[0]) for m in mem])[:-1]
        p = aacgpu.Pipeline(channels=2, max_streams=2, max_frames=3, lanes=2)
        parts = [[], []]
        for b, (live, counts, at) in enumerate(script):
            if b == 2:
                p.reset_stream(0)
            pcm = p.decode(data, packed([mem[s][1] for s in live], [bases[s] for s in live], at, counts), np.array(live, np.uint32), np.array(counts, np.uint32))[0]
            first = np.concatenate([[0], np.cumsum(counts)]) * 2048
            for k, s in enumerate(live):
                parts[s].append(pcm[first[k]:first[k + 1]].copy())
        p.close()
        return [np.concatenate(x) for x in parts]

    want = run(P["mem"], script, 2, P["si"], False, way, None, reset={2: [0]})
    got = run(P["mem"], script, 2, P["si"], False, way, meter, reset={2: [0]})
    same_delivery(got, want, way)
    same_as_rule(got, ruled(plain(), 2, meter, cuts={0: [cut]}), way)
    assert sum(len(r) for r in got["records"][0]) == cut // 1000 + (12 * 1024 - cut) // 1000


@pytest.mark.parametrize("way", ["host", "planar"])
def test_silence_flows_through_the_filters(way):
    """three 5.1 streams — one clean, one whose first frame is malformed (no layout is learnt in the first batch: its frames there are
    1024 zeros each and the transform's destination is cleared for them), one with a malformed frame behind a learnt layout (a refused
    frame: silence between music).  The zeros advance the clock and pass through the filters like any other"""
    c = CASE["surround48"]
    data, table, _ = load(c)

    def broken(at):
        bad = data.copy()
        off, length = int(table[at]["byte_offset"]), int(table[at]["byte_length"])
        bad[off + 7: off + length] = 0xFF                      # a raw_data_block with none of the stream's elements in it
        return bad

    mem = [(data, table), (broken(0), table), (broken(2), table)]
    script = [([0, 1, 2], [2, 1, 3], [0, 0, 0]), ([0, 1, 2], [2, 3, 1], [2, 1, 3]), ([0, 1, 2], [1, 1, 1], [4, 4, 4])]
    assert len(table) == 5
    meter = hostile(21, 1000)
    plain = run_script(mem, script, 6, c["sampleIndex"], 3, False)
    assert plain[2] >= 2 and plain[1][1][0] != 0 and plain[1][2][2] != 0 and not plain[1][0].any(), plain[1]
    want = run(mem, script, 6, c["sampleIndex"], False, way, None)
    got = run(mem, script, 6, c["sampleIndex"], False, way, meter)
    same_delivery(got, want, way)
    same_as_rule(got, ruled(plain[0], 6, meter), way)
    first = np.concatenate(got["records"][1])[0]
    assert not first.any() and np.concatenate(got["records"][1])[1:, :, 0].any(), "the unlearnt stream's frame is not silent, or what follows it is"
    assert got["refusals"] == plain[2]


@pytest.mark.parametrize("setup", ["mix-and-resampler", "carry-window-shape", "plan-mode-1"])
def test_beside_the_other_options(setup):
    """the meter reads the TRANSFORM's PCM whatever leaves: with a mix to mono and a resampler to 16 kHz behind it the PCM is the
    unmetered run's and the records are the rule over the plain pipeline's stereo 48 kHz PCM; with carry_window_shape; with device plans"""
    kw, plain_kw, mode, way, i16 = {}, {}, False, "host", False
    if setup == "mix-and-resampler":
        kw, way, i16 = dict(mix=mix_kit.hostile_matrix(1, 2), resample=aacgpu.resample_design(48000, 16000, 32)), "packed", True
    elif setup == "carry-window-shape":
        kw = plain_kw = dict(carry_window_shape=True)
        way = "planar"
    else:
        mode = True
    P = plain_run("stereo48", i16, mode, **plain_kw)
    meter = bs1770(48000, 4800) if setup == "plan-mode-1" else hostile(33, 1000)
    want = run(P["mem"], P["script"], 2, P["si"], mode, way, None, i16=i16, **kw)
    got = run(P["mem"], P["script"], 2, P["si"], mode, way, meter, i16=i16, **kw)
    same_delivery(got, want, setup)
    same_as_rule(got, expected(P, meter), setup)
    if setup == "mix-and-resampler":
        assert got["raw"][0].dtype == np.int16 and sum(len(r) for r in got["records"][0]) == 12
    if mode:
        assert got["counts"]["shaped"] == len(P["script"])


def test_refusals_leave_the_pipeline_as_it_was():
    """aacg_pipeline_set_loudness: a null config, a hop outside its limits, a coefficient that is not finite, a second call, a call after
    the first batch; aacg_pipeline_loudness_out on a pipeline without a meter; a submission with no destination named, and one whose
    destination is too small: each is refused with a reason, nothing is enqueued, no ticket is taken, no clock moves, the destination stays
    armed — and the pipeline decodes its next batch exactly as one that never saw the call"""
    data, table, _ = load(CASE["stereo48"])
    fr = [packed([table] * 2, [0, 0], [a, a], [3, 3]) for a in (0, 3)]
    slots, cnt = np.arange(2, dtype=np.uint32), np.full(2, 3, np.uint32)
    fresh = aacgpu.Pipeline(channels=2, max_streams=2, max_frames=3)
    want = [fresh.decode(data, f, slots, 3)[0].copy() for f in fr]
    launches = fresh.launch_counts()
    fresh.close()
    meter = hostile(5, 1000)

    def cfg(hop, coeffs):
        c = aacgpu.LoudnessConfig(hop)
        k = np.ascontiguousarray(coeffs, np.float32)
        C.memmove(c.coeffs, k.ctypes.data, 40)
        return c

    def refused(p, c, code=ERR_INVALID_ARG):
        rc = p.lib.aacg_pipeline_set_loudness(p.handle, None if c is None else C.byref(c))
        assert rc == code, rc
        reason = p.lib.aacg_pipeline_last_error(p.handle).decode()
        assert reason.startswith("aacg_pipeline_set_loudness: ") and len(reason) > 30, reason
        return reason

    nan, inf = meter["coeffs"].copy(), meter["coeffs"].copy()
    nan[1, 3], inf[0, 0] = np.nan, np.inf
    p = aacgpu.Pipeline(channels=2, max_streams=2, max_frames=3)
    reasons = [refused(p, None), refused(p, cfg(0, meter["coeffs"])), refused(p, cfg(2 ** 20 + 1, meter["coeffs"])), refused(p, cfg(1000, nan)), refused(p, cfg(1000, inf))]
    assert len(set(reasons)) == 4
    buf = np.zeros(64, np.float32)
    assert p.lib.aacg_pipeline_loudness_out(p.handle, buf.ctypes.data, buf.size, None) == ERR_INVALID_ARG, "no meter"
    assert p.lib.aacg_pipeline_loudness_counts(p.handle, slots.ctypes.data, cnt.ctypes.data, 2, cnt.copy().ctypes.data) == ERR_INVALID_ARG
    assert same_bits(p.decode(data, fr[0], slots, 3)[0], want[0])
    assert "submitted" in refused(p, cfg(1000, meter["coeffs"]))        # after the first batch
    assert same_bits(p.decode(data, fr[1], slots, 3)[0], want[1]) and p.launch_counts() == launches
    p.close()

    def raw_submit(p, f, pcm):
        res, n_ref, t = np.zeros(len(f), aacgpu.PARSE_RESULT_DTYPE), C.c_uint32(0), C.c_uint64(0)
        rc = p.lib.aacg_pipeline_submit_ragged(p.handle, data.ctypes.data, data.size, f.ctypes.data, slots.ctypes.data, 2, cnt.ctypes.data, pcm.ctypes.data,
                                               res.ctypes.data, C.byref(n_ref), C.byref(t))
        return rc, int(t.value), (res, n_ref)

    ref = aacgpu.Pipeline(channels=2, max_streams=2, max_frames=3, loudness=meter)
    ref_recs = []
    for f in fr:
        ref.decode(data, f, slots, 3)
        ref_recs.append(ref.take_loudness())
    ref.close()

    p = aacgpu.Pipeline(channels=2, max_streams=2, max_frames=3, loudness=meter)
    assert "already" in refused(p, cfg(1000, meter["coeffs"]))          # a second call
    pcm = np.zeros(2 * 3 * 2048, np.float32)
    rc, t, _ = raw_submit(p, fr[0], pcm)                                # no destination named
    assert rc == ERR_INVALID_ARG and t == 0 and "aacg_pipeline_loudness_out" in p.lib.aacg_pipeline_last_error(p.handle).decode()
    need = 2 * 3 * 2 * 2                                                # two streams x three records x two channels x two floats
    assert p.loudness_counts(slots, cnt).tolist() == [3, 3]
    small, n_of = np.full(need + 8, np.nan, np.float32), np.full(2, 77, np.uint32)
    assert p.lib.aacg_pipeline_loudness_out(p.handle, small.ctypes.data, need - 1, n_of.ctypes.data) == 0
    rc, t, _ = raw_submit(p, fr[0], pcm)                                # too small by one float
    assert rc == ERR_CAPACITY and t == 0 and n_of.tolist() == [77, 77] and np.isnan(small).all() and not pcm.any()
    assert p.loudness_counts(slots, cnt).tolist() == [3, 3], "a refused submission moved the clocks"
    with pytest.raises(aacgpu.AacgError):
        p.collect(1)                                                    # no ticket was taken
    assert p.lib.aacg_pipeline_loudness_out(p.handle, small.ctypes.data, need, n_of.ctypes.data) == 0
    bad = fr[0].copy()
    bad["byte_offset"][0] = data.size                                   # a submission refused for a reason of its own
    rc, t, _ = raw_submit(p, bad, pcm)
    assert rc == ERR_INVALID_ARG and t == 0
    rc, t, keep = raw_submit(p, fr[0], pcm)                             # ... and the destination is still armed
    assert rc == 0 and t == 1 and n_of.tolist() == [3, 3]
    assert p.lib.aacg_pipeline_collect(p.handle, t) == 0
    assert same_bits(pcm, want[0]) and np.isnan(small[need:]).all()
    assert same_bits(small[:need], np.concatenate([r.reshape(-1) for r in ref_recs[0]]))
    rc, t2, _ = raw_submit(p, fr[1], pcm)                               # one call arms one submission
    assert rc == ERR_INVALID_ARG and t2 == 0
    got = p.decode(data, fr[1], slots, 3)[0]
    assert same_bits(got, want[1])
    for x, y in zip(p.take_loudness(), ref_recs[1]):
        assert same_bits(x, y)
    assert p.launch_counts() == launches
    p.close()
