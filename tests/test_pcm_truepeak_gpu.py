"""The true-peak stage on the resident route (aacg_pipeline_set_true_peak, aacgpu.Pipeline(loudness=..., true_peak=...)) on a real MI355X.
Every configuration runs twice on a METERED pipeline, with and without the stage: with it, everything the pipeline delivered without it —
every byte of every destination buffer, poison behind the batch included, statuses, refusal counts, plan builds, launch counts and the
meter's own records — is bit-identical; and the true-peak records equal, BIT FOR BIT (a NaN for a NaN), the rule of include/aacgpu.h in
numpy float32 (truepeak_kit.rule) over the transform PCM that a plain pipeline delivers for the same script (resident_kit.run_script),
per slot across the batches.  Hops of 37, 1000 and 4800, batches of at most 3 frames, at most 3 streams."""
import ctypes as C

import numpy as np
import pytest

import aacgpu
import features_kit
import loudness_kit
import mix_kit
import truepeak_kit as kit
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


def run(members, script, C_, si, device_plans, way, meter, stage, i16=False, ahead=True, reset=None, lanes=2, **kw):
    """the script on a metered pipeline with or without the stage, the PCM (or the feature frames) delivered `way`; ahead: every batch is
    submitted before the first is collected; reset: {batch index: slots reset in front of it} -> dict(raw: every batch's whole
    destination buffer, status, refusals, builds, counts, records: the meter's per stream, peaks: per stream (n, C) or None)"""
    S = len(members)
    data = np.concatenate([m[0] for m in members])
    bases = np.cumsum([0] + [len(m[0]) for m in members])[:-1]
    tables = [m[1] for m in members]
    if i16:
        kw["output_kind"] = aacgpu.OUTPUT_I16
    p = aacgpu.Pipeline(channels=C_, max_streams=S, max_frames=3, sample_index=si, device_plans=device_plans, lanes=lanes, loudness=meter, true_peak=stage, **kw)
    O = p.features["n_mels"] if p.features else p.channels
    dtype = np.int16 if i16 and not p.features else np.float32
    out = dict(raw=[], status=[[] for _ in range(S)], refusals=0, records=[[] for _ in range(S)], peaks=[[] for _ in range(S)] if stage else None)
    clock, pending = [0] * S, []

    def finish(item):
        b, ticket, live, counts, buf, n_rec = item
        # the three calls in every order: each finishes the batch if it is the first, and none takes what another returns
        order = [["tp", "pcm", "ld"], ["ld", "tp", "pcm"], ["pcm", "ld", "tp"]][b % 3]
        for what in order:
            if what == "tp" and stage:
                peaks = p.take_true_peak(ticket)
            elif what == "ld":
                recs = p.take_loudness(ticket)
            elif what == "pcm":
                back, res, refused, *_ = p.collect(ticket)
        assert back is buf
        out["raw"].append(buf.copy() if way == "host" else buf.cpu().numpy())
        out["refusals"] += refused
        first = np.concatenate([[0], np.cumsum(counts)])
        for k, s in enumerate(live):
            out["status"][s].append(res["status"][first[k]:first[k + 1]].copy())
            assert recs[k].shape == (n_rec[k], C_, 2)
            out["records"][s].append(recs[k])
            if stage:
                assert peaks[k].shape == (n_rec[k], C_) and peaks[k].dtype == np.float32
                out["peaks"][s].append(peaks[k])

    for b, (live, counts, at) in enumerate(script):
        for s in (reset or {}).get(b, []):
            for item in pending:
                finish(item)
            pending = []
            p.reset_stream(s)
            clock[s] = 0
        fr = packed([tables[s] for s in live], [bases[s] for s in live], at, counts)
        slots, cnt = np.array(live, np.uint32), np.array(counts, np.uint32)
        n_out = [int(v) for v in (p.out_samples(slots, cnt) if p.resample or p.features else cnt.astype(np.int64) * 1024)]
        n_rec = [(clock[s] + 1024 * c) // meter["hop"] - clock[s] // meter["hop"] for s, c in zip(live, counts)]
        total = sum(n_out)
        if way == "host":
            buf = poison_host(np.empty((total + 64) * O, dtype))
            t = p.submit(data, fr, slots, cnt, pcm=buf)
        else:
            planar = way == "planar"
            stride = (max(n_out) + 1023) // 1024
            buf = poisoned_device((len(live) + 1, O, stride * 1024) if planar else ((total + 64) * O,), dtype == np.int16)
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
    """with the stage everything else is what it was without: the destination buffers whole, statuses, refusals, builds, launch counts
    (the stage's own launch is not among the transform's) and the meter's records"""
    assert len(got["raw"]) == len(want["raw"]), what
    for b, (x, y) in enumerate(zip(got["raw"], want["raw"])):
        assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(raw_bits(x), raw_bits(y)), "%s: batch %d's destination differs with the stage" % (what, b)
    for x, y in zip(got["status"], want["status"]):
        assert np.array_equal(np.concatenate(x), np.concatenate(y)), what
    assert got["refusals"] == want["refusals"] and got["builds"] == want["builds"] and got["counts"] == want["counts"], what
    for s, (x, y) in enumerate(zip(got["records"], want["records"])):
        assert len(x) == len(y) and all(same_bits(a, b) for a, b in zip(x, y)), "%s: stream %d's meter records differ with the stage" % (what, s)


def ruled(plain_pcm, C_, hop, table, cuts=None):
    """per stream: the rule over the plain pipeline's transform PCM; cuts: {stream: samples at which its slot was reset}"""
    out = []
    for s, x in enumerate(plain_pcm):
        pieces = np.split(x.reshape(-1, C_), (cuts or {}).get(s, []))
        out.append(np.concatenate([kit.rule(piece, hop, table, kit.State(C_, table.shape[1])) for piece in pieces]))
    return out


def same_as_rule(got, want, what):
    for s, (parts, y) in enumerate(zip(got["peaks"], want)):
        kit.same_records(np.concatenate(parts), y, "%s, stream %d over the plain pipeline's PCM" % (what, s))


def committed(name, copies, frames=12):
    """`frames` frames of a committed stream, its own in rotation where it has fewer (any sequence of a stream's frames decodes)"""
    c = CASE[name]
    data, table, _ = load(c)
    return [(data, table[np.arange(frames) % len(table)])] * copies, c["channels"], c["sampleIndex"]


def meter_of(hop, seed=3):
    return {"hop": hop, "coeffs": loudness_kit.hostile_coeffs(seed)}


def stage_of(Lp, T, kind):
    if kind == "designed":
        return aacgpu.true_peak_design(Lp, T)
    return {"phases": Lp, "taps": T, "table": kit.mixed_table(Lp, T)}


# stream, int16, hop, the table
SETUPS = {"stereo48-f32-hop1000-L4T12-mixed": ("stereo48", False, 1000, (4, 12, "mixed")),
          "stereo48-i16-hop4800-L4T24-designed": ("stereo48", True, 4800, (4, 24, "designed")),
          "stereo48-f32-hop37-L1T4-mixed": ("stereo48", False, 37, (1, 4, "mixed")),
          "surround48-f32-hop4800-L8T64-mixed": ("surround48", False, 4800, (8, 64, "mixed")),
          "surround48-i16-hop1000-L4T24-designed": ("surround48", True, 1000, (4, 24, "designed")),
          "mono22-f32-hop1000-L4T24-designed": ("mono22", False, 1000, (4, 24, "designed")),
          "mono22-i16-hop4800-L8T64-mixed": ("mono22", True, 4800, (8, 64, "mixed"))}
_plain = {}


def plain_run(name, i16, mode=False, **kw):
    """the yardstick, once per stream, element type and options: two slots, seeded ragged batches of at most 3 frames, decoded by a pipeline
    without meter, mix or resampler; the ways and the tests share it (and leave it unchanged), and the rule over it per stage"""
    key = (name, i16, mode, tuple(sorted(kw)))
    if key not in _plain:
        mem, C_, si = committed(name, 2)
        script = ragged_script([m[1] for m in mem], 3, np.random.default_rng(11))
        assert len(script) >= 3, "three or more submissions on two lanes: lanes are reused"
        opts = dict(kw, **(dict(output_kind=aacgpu.OUTPUT_I16) if i16 else {}))
        _plain[key] = dict(mem=mem, C=C_, si=si, script=script, pcm=run_script(mem, script, C_, si, 3, mode, **opts)[0], ruled={})
    return _plain[key]


def expected(P, hop, stage):
    key = (hop, stage["table"].tobytes(), stage["table"].shape)
    if key not in P["ruled"]:
        P["ruled"][key] = ruled(P["pcm"], P["C"], hop, stage["table"])
    return P["ruled"][key]


@pytest.mark.parametrize("way", WAYS)
@pytest.mark.parametrize("case", sorted(SETUPS))
def test_records_are_the_rule_and_nothing_else_differs(case, way):
    """stereo, mono and 5.1, f32 and int16, tables of mixed signs and designed ones, hops of 37 (dozens of records a frame), 1000 and
    4800 (several batches emit nothing and carry their partial maximum); ragged batches on two lanes, all submitted before the first is
    collected: every launch reads the state the one before it wrote on the other lane's stream.  Host memory, the caller's device
    memory packed, and planar"""
    name, i16, hop, (Lp, T, kind) = SETUPS[case]
    meter, stage, P = meter_of(hop), stage_of(Lp, T, kind), plain_run(name, i16)
    want = run(P["mem"], P["script"], P["C"], P["si"], False, way, meter, None, i16=i16)
    got = run(P["mem"], P["script"], P["C"], P["si"], False, way, meter, stage, i16=i16)
    same_delivery(got, want, "%s, %s" % (case, way))
    same_as_rule(got, expected(P, hop, stage), "%s, %s" % (case, way))
    peaks = np.concatenate(got["peaks"][0])
    assert len(peaks) == 12 * 1024 // hop and peaks.max() > 0, "the streams are music"
    if hop == 4800:
        assert any(len(r) == 0 for r in got["peaks"][0]), "a hop that spans batches: some emit nothing"
    assert got["counts"]["launches"] == len(P["script"])


def test_the_python_surface_end_to_end():
    """design, Pipeline(loudness=, true_peak=), decode, take_true_peak() and take_loudness() of the last decode; with the default design
    over music the true peak lies within a few dB of the sample peak, hop for hop"""
    P = plain_run("stereo48", False)
    data, table = P["mem"][0]
    stage = aacgpu.true_peak_design()
    assert (stage["phases"], stage["taps"]) == (4, 24) and stage["table"].shape == (4, 24)
    p = aacgpu.Pipeline(channels=2, max_streams=1, max_frames=3, loudness=aacgpu.loudness_design(48000, hop=1000), true_peak=stage)
    tps, recs = [], []
    for a in range(0, 12, 3):
        p.decode(data, table[a:a + 3], [0], 3)
        tps += p.take_true_peak()
        recs += p.take_loudness()
    with pytest.raises(aacgpu.AacgError):
        p.take_true_peak(99)                                             # no such ticket
    p.close()
    bare = aacgpu.Pipeline(channels=2, max_streams=1, max_frames=3, loudness=aacgpu.loudness_design(48000))
    bare.decode(data, table[:3], [0], 3)
    with pytest.raises(ValueError):
        bare.take_true_peak()                                            # no stage: nothing is held
    bare.close()
    tp, rec = np.concatenate(tps), np.concatenate(recs)
    assert tp.shape == (12, 2) and rec.shape == (12, 2, 2)
    kit.same_records(tp, kit.rule_whole(P["pcm"][0].reshape(-1, 2), 1000, stage["table"])[0], "decode + take_true_peak")
    loud = rec[:, :, 1] > 1e-3
    assert loud.any() and np.isfinite(tp).all() and np.median(np.abs(20 * np.log10(tp[loud] / rec[:, :, 1][loud]))) < 3.0


@pytest.mark.parametrize("way", ["host", "packed"])
def test_a_reset_in_mid_run(way):
    """two lanes, two slots, the seeded script with aacg_pipeline_reset_stream(0) in front of the third batch, in the middle of a hop of
    4800: from there on slot 0's records are the rule over the frames since the reset from nothing — no history, no partial maximum —
    while slot 1 goes on"""
    P = plain_run("stereo48", False)
    script, meter, stage = P["script"], meter_of(4800, 8), stage_of(4, 12, "mixed")
    cut = sum(c for live, counts, at in script[:2] for s, c in zip(live, counts) if s == 0) * 1024
    assert cut % 4800 != 0, "the reset falls in mid-hop"

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

    want = run(P["mem"], script, 2, P["si"], False, way, meter, None, reset={2: [0]})
    got = run(P["mem"], script, 2, P["si"], False, way, meter, stage, reset={2: [0]})
    same_delivery(got, want, way)
    same_as_rule(got, ruled(plain(), 2, 4800, stage["table"], cuts={0: [cut]}), way)
    assert sum(len(r) for r in got["peaks"][0]) == cut // 4800 + (12 * 1024 - cut) // 4800


@pytest.mark.parametrize("way", ["host", "planar"])
def test_a_refused_frame_and_an_unlearnt_stream(way):
    """three 5.1 streams — one clean, one whose first frame is malformed (no layout is learnt in the first batch: its frames there are
    1024 zeros each), one with a malformed frame behind a learnt layout (a refused frame: silence between music).  The zeros advance the
    clock and pass through the filter like any other"""
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
    meter, stage = meter_of(1000, 21), stage_of(4, 24, "designed")
    plain = run_script(mem, script, 6, c["sampleIndex"], 3, False)
    assert plain[2] >= 2 and plain[1][1][0] != 0 and plain[1][2][2] != 0 and not plain[1][0].any(), plain[1]
    want = run(mem, script, 6, c["sampleIndex"], False, way, meter, None)
    got = run(mem, script, 6, c["sampleIndex"], False, way, meter, stage)
    same_delivery(got, want, way)
    same_as_rule(got, ruled(plain[0], 6, 1000, stage["table"]), way)
    peaks = np.concatenate(got["peaks"][1])
    assert not peaks[0].any() and peaks[1:].any(), "the unlearnt stream's frame is not silent, or what follows it is"
    assert got["refusals"] == plain[2]


@pytest.mark.parametrize("setup", ["mix-limiter-resampler", "mix-resampler-features", "carry-window-shape", "plan-mode-1"])
def test_beside_the_other_options(setup):
    """the stage reads the TRANSFORM's PCM whatever leaves: with a mix to mono, a limiter and a resampler to 16 kHz behind it, or with a
    feature stage at the end, what leaves is the run's without the stage and the records are the rule over the plain pipeline's stereo
    48 kHz PCM; with carry_window_shape; with device plans"""
    kw, plain_kw, mode, way, i16 = {}, {}, False, "host", False
    if setup == "mix-limiter-resampler":
        kw, way, i16 = dict(mix=mix_kit.hostile_matrix(1, 2), limiter=(0.25, 0.5), resample=aacgpu.resample_design(48000, 16000, 32)), "packed", True
    elif setup == "mix-resampler-features":
        basis, fb = features_kit.hostile_tables(64, 33, 5)
        kw = dict(mix=aacgpu.mix_standard(2, 1), resample=aacgpu.resample_design(48000, 16000, 32),
                  features=dict(frame_length=64, hop=24, pad_left=17, basis=basis, fb=fb, floor=1e-3, log=False))
    elif setup == "carry-window-shape":
        kw = plain_kw = dict(carry_window_shape=True)
        way = "planar"
    else:
        mode = True
    P = plain_run("stereo48", i16, mode, **plain_kw)
    hop = 4800 if setup == "plan-mode-1" else 1000
    meter, stage = meter_of(hop, 33), stage_of(4, 24, "designed" if mode else "mixed")
    want = run(P["mem"], P["script"], 2, P["si"], mode, way, meter, None, i16=i16, **kw)
    got = run(P["mem"], P["script"], 2, P["si"], mode, way, meter, stage, i16=i16, **kw)
    same_delivery(got, want, setup)
    same_as_rule(got, expected(P, hop, stage), setup)
    if mode:
        assert got["counts"]["shaped"] == len(P["script"])


def test_refusals_leave_the_pipeline_as_it_was():
    """aacg_pipeline_set_true_peak: no meter, a null config, a null table, phases or taps outside their limits, an entry that is not
    finite, a second call, a call after the first batch; aacg_pipeline_true_peak_out on a pipeline without the stage; a submission with no
    destination named, and one whose destination is too small — behind the meter's own two, which come first: each is refused with a
    reason, nothing is enqueued, no ticket is taken, no clock moves, both destinations stay armed — and the pipeline decodes its next
    batch exactly as one that never saw the call"""
    data, table, _ = load(CASE["stereo48"])
    fr = [packed([table] * 2, [0, 0], [a, a], [3, 3]) for a in (0, 3)]
    slots, cnt = np.arange(2, dtype=np.uint32), np.full(2, 3, np.uint32)
    meter, stage = meter_of(1000, 5), stage_of(4, 12, "mixed")
    ref = aacgpu.Pipeline(channels=2, max_streams=2, max_frames=3, loudness=meter)
    want, want_recs = [], []
    for f in fr:
        want.append(ref.decode(data, f, slots, 3)[0].copy())
        want_recs.append(ref.take_loudness())
    launches = ref.launch_counts()
    ref.close()

    def cfg(Lp, T, h):
        h = None if h is None else np.ascontiguousarray(h, np.float32)
        c = aacgpu.TruePeakConfig(Lp, T, None if h is None else h.ctypes.data)
        c.keep = h
        return c

    def refused(p, c, code=ERR_INVALID_ARG):
        rc = p.lib.aacg_pipeline_set_true_peak(p.handle, None if c is None else C.byref(c))
        assert rc == code, rc
        reason = p.lib.aacg_pipeline_last_error(p.handle).decode()
        assert reason.startswith("aacg_pipeline_set_true_peak: ") and len(reason) > 32, reason
        return reason

    h = stage["table"]
    bare = aacgpu.Pipeline(channels=2, max_streams=2, max_frames=3)
    assert "no meter" in refused(bare, cfg(4, 12, h))
    buf = np.zeros(64, np.float32)
    assert bare.lib.aacg_pipeline_true_peak_out(bare.handle, buf.ctypes.data, buf.size) == ERR_INVALID_ARG
    bare.close()

    nan, inf = h.copy(), h.copy()
    nan[3, 11], inf[0, 0] = np.nan, -np.inf
    big = np.zeros((9, 68), np.float32)
    p = aacgpu.Pipeline(channels=2, max_streams=2, max_frames=3, loudness=meter)
    reasons = [refused(p, None), refused(p, cfg(4, 12, None)), refused(p, cfg(0, 12, big)), refused(p, cfg(9, 12, big)), refused(p, cfg(4, 0, big)),
               refused(p, cfg(4, 10, big)), refused(p, cfg(4, 68, big)), refused(p, cfg(4, 12, nan)), refused(p, cfg(4, 12, inf))]
    assert len(set(reasons)) == 6, reasons
    assert p.lib.aacg_pipeline_true_peak_out(p.handle, buf.ctypes.data, buf.size) == ERR_INVALID_ARG, "no stage"
    assert same_bits(p.decode(data, fr[0], slots, 3)[0], want[0]) and all(same_bits(x, y) for x, y in zip(p.take_loudness(), want_recs[0]))
    assert "submitted" in refused(p, cfg(4, 12, h))                      # after the first batch
    assert same_bits(p.decode(data, fr[1], slots, 3)[0], want[1]) and all(same_bits(x, y) for x, y in zip(p.take_loudness(), want_recs[1]))
    assert p.launch_counts() == launches
    p.close()

    def raw_submit(p, f, pcm):
        res, n_ref, t = np.zeros(len(f), aacgpu.PARSE_RESULT_DTYPE), C.c_uint32(0), C.c_uint64(0)
        rc = p.lib.aacg_pipeline_submit_ragged(p.handle, data.ctypes.data, data.size, f.ctypes.data, slots.ctypes.data, 2, cnt.ctypes.data, pcm.ctypes.data,
                                               res.ctypes.data, C.byref(n_ref), C.byref(t))
        return rc, int(t.value), (res, n_ref)

    full = aacgpu.Pipeline(channels=2, max_streams=2, max_frames=3, loudness=meter, true_peak=stage)
    ref_tp = []
    for f in fr:
        full.decode(data, f, slots, 3)
        ref_tp.append(full.take_true_peak())
    full.close()

    p = aacgpu.Pipeline(channels=2, max_streams=2, max_frames=3, loudness=meter, true_peak=stage)
    assert "already" in refused(p, cfg(4, 12, h))                        # a second call
    pcm = np.zeros(2 * 3 * 2048, np.float32)
    need = 2 * 3 * 2                                                     # two streams x three records x two channels
    rec, small = np.full(2 * need, np.nan, np.float32), np.full(need + 8, np.nan, np.float32)
    last = lambda: p.lib.aacg_pipeline_last_error(p.handle).decode()
    rc, t, _ = raw_submit(p, fr[0], pcm)                                 # neither destination named: the meter's refusal comes first
    assert rc == ERR_INVALID_ARG and t == 0 and "aacg_pipeline_loudness_out" in last()
    assert p.lib.aacg_pipeline_true_peak_out(p.handle, small.ctypes.data, need) == 0
    assert p.lib.aacg_pipeline_loudness_out(p.handle, rec.ctypes.data, 2 * need - 1, None) == 0
    rc, t, _ = raw_submit(p, fr[0], pcm)                                 # the meter's is too small: its refusal, again first
    assert rc == ERR_CAPACITY and t == 0 and "loudness" in last()
    p2 = aacgpu.Pipeline(channels=2, max_streams=2, max_frames=3, loudness=meter, true_peak=stage)
    assert p2.lib.aacg_pipeline_loudness_out(p2.handle, rec.ctypes.data, rec.size, None) == 0
    res, n_ref, tk = np.zeros(len(fr[0]), aacgpu.PARSE_RESULT_DTYPE), C.c_uint32(0), C.c_uint64(0)
    rc = p2.lib.aacg_pipeline_submit_ragged(p2.handle, data.ctypes.data, data.size, fr[0].ctypes.data, slots.ctypes.data, 2, cnt.ctypes.data, pcm.ctypes.data,
                                            res.ctypes.data, C.byref(n_ref), C.byref(tk))
    assert rc == ERR_INVALID_ARG and tk.value == 0 and "aacg_pipeline_true_peak_out" in p2.lib.aacg_pipeline_last_error(p2.handle).decode()      # the meter's named, the stage's not
    p2.close()
    assert p.lib.aacg_pipeline_loudness_out(p.handle, rec.ctypes.data, rec.size, None) == 0
    assert p.lib.aacg_pipeline_true_peak_out(p.handle, small.ctypes.data, need - 1) == 0
    rc, t, _ = raw_submit(p, fr[0], pcm)                                 # the stage's is too small by one float
    assert rc == ERR_CAPACITY and t == 0 and "true-peak" in last() and np.isnan(small).all() and np.isnan(rec).all() and not pcm.any()
    assert p.loudness_counts(slots, cnt).tolist() == [3, 3], "a refused submission moved the clocks"
    with pytest.raises(aacgpu.AacgError):
        p.collect(1)                                                     # no ticket was taken
    assert p.lib.aacg_pipeline_true_peak_out(p.handle, small.ctypes.data, need) == 0
    rc, t, keep = raw_submit(p, fr[0], pcm)                              # ... and the meter's destination is still armed
    assert rc == 0 and t == 1
    assert p.lib.aacg_pipeline_collect(p.handle, t) == 0
    assert same_bits(pcm, want[0]) and np.isnan(small[need:]).all()
    kit.same_records(small[:need], np.concatenate([r.reshape(-1) for r in ref_tp[0]]), "the records through the C ABI")
    assert same_bits(rec, np.concatenate([r.reshape(-1) for r in want_recs[0]]))
    assert p.lib.aacg_pipeline_loudness_out(p.handle, rec.ctypes.data, rec.size, None) == 0
    rc, t2, _ = raw_submit(p, fr[1], pcm)                                # one call arms one submission
    assert rc == ERR_INVALID_ARG and t2 == 0 and "aacg_pipeline_true_peak_out" in last()
    got = p.decode(data, fr[1], slots, 3)[0]
    assert same_bits(got, want[1])
    for x, y in zip(p.take_true_peak(), ref_tp[1]):
        kit.same_records(x, y, "the second batch")
    assert p.launch_counts() == launches
    p.close()
