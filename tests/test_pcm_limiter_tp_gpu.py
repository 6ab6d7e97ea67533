"""The limiter's true-peak detector on the resident route (aacg_pipeline_set_limiter_true_peak, aacg_pipeline_limiter_delay,
aacgpu.Pipeline(limiter=..., limiter_true_peak=...)) on a real MI355X.  A script of ragged batches is decoded by a pipeline WITHOUT the
limiter; the rule of include/aacgpu.h in numpy float32 (limiter_tp_kit.rule) is applied to that PCM per slot, batch after batch, with the
gains as they stood when each batch was enqueued; the same script on a pipeline WITH the limiter and the detector must deliver those
bits, and the results, refusal counts and launch counts of the pipeline with the plain limiter.  The ceiling is taken from the unlimited
decode itself, half its largest sample, so that the stage demonstrably engages — asserted on the kit's result.
Five streams of six frames, ragged batches of 1..3 frames, five lanes with device plans, four batches in flight; host memory and device
memory packed and planar; f32 and int16; stereo and 5.1 through the standard downmix; a reset in mid-run, gains set with batches in
flight, a refused frame and an unlearnt stream; in front of the resampler and the trim, and of the feature stage; the refusals."""
import ctypes as C

import numpy as np
import pytest

import aacgpu
import features_kit
import limiter_tp_kit as kit
import resample_kit
import truepeak_kit
from resident_kit import CASES, ERR_INVALID_ARG, load, packed, ragged_script, same_bits

pytestmark = pytest.mark.gpu
CASE = {c["name"]: c for c in CASES}
F = np.float32
RELEASE = 0.0625
I16_POISON = 0x7F7F
TABLE = truepeak_kit.design(4, 24)                       # aacg_true_peak_design's defaults, restated
TP = (4, 24, TABLE)
LATE = 64 + 12


def committed(name, copies, frames=6):
    """`frames` frames of a committed stream, its own in rotation where it has fewer; each copy starts a frame later"""
    c = CASE[name]
    data, table, _ = load(c)
    return [(data, table[(np.arange(frames) + k) % len(table)]) for k in range(copies)], c["channels"], c["sampleIndex"]


def run(mem, script, C_, si, way="pageable", i16=False, limiter=None, tp=None, gains=None, gain_at=None, reset=None, mix=None, resample=None,
        features=None, trim=None, windows=None, lanes=5, in_flight=4, max_frames=3):
    """the script on a pipeline -> dict(out: per stream (rows, width) of what left, status, refusals, counts, delay).  gains: {slot: G}
    set before the first batch; gain_at: {batch: {slot: G}} set in front of that batch while those before it are in flight; reset:
    {batch: slots reset in front of it}; windows: slot -> (skip_in, keep_in) in the stream's own samples, converted by
    trim_design(delay=limiter_delay()) on the pipeline itself"""
    import torch
    S = len(mem)
    data = np.concatenate([m[0] for m in mem])
    bases = np.cumsum([0] + [len(m[0]) for m in mem])[:-1]
    tables = [m[1] for m in mem]
    kw = dict(output_kind=aacgpu.OUTPUT_I16) if i16 else {}
    p = aacgpu.Pipeline(channels=C_, max_streams=S, max_frames=max_frames, sample_index=si, mix=mix, resample=resample, features=features,
                        limiter=limiter, limiter_true_peak=tp, lanes=lanes, device_plans=True, trim=trim, **kw)
    width = p.features["n_mels"] if features else p.channels
    dtype = np.float32 if features or not i16 else np.int16
    ragged = bool(resample or features or trim)
    out = dict(out=[[] for _ in range(S)], status=[[] for _ in range(S)], refusals=0, delay=p.limiter_delay() if limiter else 0, windows={})
    for slot, g in (gains or {}).items():
        p.set_gain(slot, g)
    for slot, (skip_in, keep_in) in (windows or {}).items():
        w = aacgpu.trim_design(skip_in, keep_in, resample=resample, delay=out["delay"])
        p.set_trim(slot, w[0], w[1])
        out["windows"][slot] = w
    pending = []

    def finish(item):
        ticket, live, counts, n_out, buf = item
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

    for b, (live, counts, at) in enumerate(script):
        for s in (reset or {}).get(b, []):
            for item in pending:
                finish(item)
            pending = []
            p.reset_stream(s)
        for slot, g in (gain_at or {}).get(b, {}).items():
            p.set_gain(slot, g)                                   # (the batches before are in flight: their gains went up with them)
        fr = packed([tables[s] for s in live], [bases[s] for s in live], at, counts)
        slots, cnt = np.array(live, np.uint32), np.array(counts, np.uint32)
        n_out = [int(v) for v in (p.out_samples(slots, cnt) if ragged else cnt.astype(np.int64) * 1024)]
        total = sum(n_out)
        if way in ("pinned", "pageable"):
            buf = p.pinned(((total + 64) * width,), dtype) if way == "pinned" else np.empty((total + 64) * width, dtype)
            buf[:] = np.nan if dtype == np.float32 else I16_POISON
            t = p.submit(data, fr, slots, cnt, pcm=buf)
        else:
            planar = way == "planar"
            stride = max(max(n_out), 1) if features else (max(n_out) + 1023) // 1024
            shape = (len(live), width, max(max(n_out), 1) if features else stride * 1024) if planar else ((total + 64) * width,)
            buf = torch.full(shape, I16_POISON, dtype=torch.int16, device="cuda") if dtype == np.int16 else torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()                              # the fill is torch's stream's, the batch a lane's
            t = p.submit_device(data, fr, slots, cnt, buf, planar=planar, stride_frames=stride if planar else None)
        pending.append((t, live, counts, n_out, buf))
        if len(pending) > in_flight:
            finish(pending.pop(0))
    for item in pending:
        finish(item)
    out["counts"] = p.launch_counts()
    p.close()
    out["out"] = [np.concatenate(g) for g in out["out"]]
    out["status"] = [np.concatenate(g) for g in out["status"]]
    return out


def ruled(plain, script, c, gains, gain_at=None, reset=None, table=TABLE):
    """per stream: the rule over the unlimited run's PCM, batch after batch as the script cuts it, with the gains as they stood when each
    batch was enqueued and the slots reset where the script says -> (what must leave per stream, the kit's states)"""
    S, width, T = len(plain), plain[0].shape[1], table.shape[1]
    G = [F(1.0)] * S
    for slot, g in gains.items():
        G[slot] = F(g)
    states, done, out, seen = [kit.State(width, T) for _ in range(S)], [0] * S, [[] for _ in range(S)], []
    for b, (live, counts, at) in enumerate(script):
        for s in (reset or {}).get(b, []):
            seen.append(states[s])
            states[s] = kit.State(width, T)
        for slot, g in (gain_at or {}).get(b, {}).items():
            G[slot] = F(g)
        for s, n in zip(live, counts):
            out[s].append(kit.rule(plain[s][done[s]:done[s] + 1024 * n], G[s], c, RELEASE, table, states[s]))
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


SETUPS = {"stereo": ("stereo48", None), "surround-to-stereo": ("surround48", lambda: aacgpu.mix_standard(6, 2))}
GAINS = {0: 1.0, 1: 4.0, 2: 0.5, 3: 2.0, 4: 1.0}
_plain = {}


def plain_run(case, i16):
    """the yardsticks, once per configuration: five slots, seeded ragged batches of 1..3 frames, decoded WITHOUT the limiter and with the
    PLAIN limiter; the tests share them and leave them unchanged"""
    key = (case, i16)
    if key not in _plain:
        name, make_mix = SETUPS[case]
        mem, C_, si = committed(name, 5)
        script = ragged_script([m[1] for m in mem], 3, np.random.default_rng(17))
        assert len(script) >= 5 and any(len(set(counts)) > 1 for live, counts, at in script), "five or more ragged submissions: every lane is used"
        mix = make_mix() if make_mix else None
        plain = run(mem, script, C_, si, i16=i16, mix=mix)
        c = ceiling_of(plain["out"])
        limited = run(mem, script, C_, si, i16=i16, mix=mix, limiter=(c, RELEASE), gains=GAINS)
        assert limited["delay"] == 64
        _plain[key] = dict(mem=mem, C=C_, si=si, script=script, mix=mix, plain=plain, limited=limited, c=c)
    return _plain[key]


@pytest.mark.parametrize("way", ["pinned", "packed", "planar"])
@pytest.mark.parametrize("i16", [False, True], ids=["f32", "i16"])
@pytest.mark.parametrize("case", sorted(SETUPS))
def test_the_rule_through_the_abi(case, i16, way):
    """five gains, the ceiling half the unlimited decode's peak, four batches in flight on five lanes: bit for bit the kit over the
    unlimited PCM, and everything else the plain limiter's pipeline's"""
    P = plain_run(case, i16)
    want, states = ruled(P["plain"]["out"], P["script"], P["c"], GAINS)
    engaged(states)
    got = run(P["mem"], P["script"], P["C"], P["si"], way=way, i16=i16, mix=P["mix"], limiter=(P["c"], RELEASE), tp=TP, gains=GAINS)
    same_out(got["out"], want, "%s, %s, %s" % (case, "i16" if i16 else "f32", way))
    assert got["delay"] == LATE
    for x, y in zip(got["status"], P["limited"]["status"]):
        assert np.array_equal(x, y)
    assert got["refusals"] == P["limited"]["refusals"] and got["counts"] == P["limited"]["counts"]
    assert not same_bits(got["out"][1], P["limited"]["out"][1]), "the detector changes what leaves"
    if not i16:
        lim = float(P["c"]) * (1 + 2.0 ** -21)
        assert max(float(np.abs(x.astype(np.float64)).max()) for x in got["out"]) <= lim, "consequence (a) of the rule"


def test_true_as_the_table_is_the_design_s(tmp_path):
    """limiter_true_peak=True takes aacg_true_peak_design's defaults: the bits of the same table given as such"""
    P = plain_run("stereo", False)
    want, _ = ruled(P["plain"]["out"], P["script"], P["c"], GAINS, table=np.ascontiguousarray(aacgpu.true_peak_design()["table"], F))
    got = run(P["mem"], P["script"], 2, P["si"], way="pageable", limiter=(P["c"], RELEASE), tp=True, gains=GAINS)
    same_out(got["out"], want, "the default table")


def test_a_reset_and_gains_with_batches_in_flight():
    """aacg_pipeline_reset_stream(0) in front of the third batch: from there on slot 0 leaves as a new stream does — 64 + T / 2 zeros
    first, a0 = th = G — while the others go on; set_gain with batches in flight: those keep the gain they were enqueued with"""
    P = plain_run("stereo", False)
    assert len(P["script"]) >= 4
    reset, gain_at = {2: [0]}, {1: {1: 6.0}, 2: {2: 0.25}, 3: {3: 0.0}}
    plain = run(P["mem"], P["script"], 2, P["si"], reset=reset)
    want, states = ruled(plain["out"], P["script"], P["c"], GAINS, gain_at=gain_at, reset=reset)
    engaged(states)
    got = run(P["mem"], P["script"], 2, P["si"], way="packed", limiter=(P["c"], RELEASE), tp=TP, gains=GAINS, gain_at=gain_at, reset=reset)
    same_out(got["out"], want, "a reset and gains in flight")
    cut = sum(n for live, counts, at in P["script"][:2] for s, n in zip(live, counts) if s == 0) * 1024
    assert plain["out"][0][cut - LATE:cut].any(), "what was held at the reset was music: it must not leave"
    assert not got["out"][0][cut:cut + LATE].any() and got["out"][0][cut + LATE:].any()


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
    mix = aacgpu.mix_standard(6, 2)
    plain = run(mem, script, 6, c["sampleIndex"], mix=mix)
    assert plain["refusals"] >= 2 and plain["status"][1][0] != 0 and plain["status"][2][2] != 0 and not plain["status"][0].any(), plain["status"]
    assert not plain["out"][1][:1024].any() and plain["out"][2][:2048].any()
    ceil, gains = ceiling_of(plain["out"]), {0: 1.0, 1: 2.0, 2: 4.0}
    want, states = ruled(plain["out"], script, ceil, gains)
    engaged(states)
    got = run(mem, script, 6, c["sampleIndex"], way=way, mix=mix, limiter=(ceil, RELEASE), tp=TP, gains=gains)
    same_out(got["out"], want, way)
    assert got["refusals"] == plain["refusals"] and not got["out"][1][:1024 + LATE].any()
    for x, y in zip(got["status"], plain["status"]):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("way", ["pageable", "packed"])
def test_in_front_of_the_trim_the_programme_range_is_exact(way):
    """no resampler, a ceiling far above the music and G = 1: the stage is a pure delay of limiter_delay() samples, and windows from
    trim_design(delay=limiter_delay()) keep exactly the samples [skip_in, skip_in + keep_in) of the unlimited pipeline's PCM"""
    P = plain_run("stereo", False)
    ranges = {0: (2112, None), 1: (1024, 3000), 2: (2113, 1), 3: (0, 6 * 1024 - LATE), 4: (5000, 0)}
    got = run(P["mem"], P["script"], 2, P["si"], way=way, limiter=(1e6, RELEASE), tp=TP, trim=True, windows=ranges)
    assert got["delay"] == LATE and got["windows"][1][:2] == (1024 + LATE, 3000)
    for s, (skip_in, keep_in) in ranges.items():
        x = P["plain"]["out"][s]
        want = x[skip_in:len(x) - LATE if keep_in is None else skip_in + keep_in]
        assert got["out"][s].shape == want.shape and same_bits(got["out"][s], want), "slot %d: not the programme's range" % s
    assert P["plain"]["out"][0][2112:].any()


@pytest.mark.parametrize("i16", [False, True], ids=["f32", "i16"])
def test_in_front_of_the_resampler_and_the_trim(i16):
    """5.1 -> stereo, limited with the detector, resampled by 160 / 441, trimmed by windows from trim_design(delay=limiter_delay()): the
    resampler's rule over the kit over the mixed PCM, sliced at those windows — which are exact integer arithmetic on delay 76"""
    P = plain_run("surround-to-stereo", i16)
    rs = aacgpu.resample_design(44100, 16000, 32)
    assert rs[:2] == (160, 441)
    ranges = {0: (2112, None), 1: (1024, 3000), 2: (2113, 1), 3: (0, 100), 4: (3000, 2000)}
    limited, states = ruled(P["plain"]["out"], P["script"], P["c"], GAINS)
    engaged(states)
    got = run(P["mem"], P["script"], P["C"], P["si"], way="packed", i16=i16, mix=P["mix"], limiter=(P["c"], RELEASE), tp=TP, gains=GAINS,
              resample=rs, trim=True, windows=ranges)
    for s, (skip_in, keep_in) in ranges.items():
        A = lambda t: 2 * 160 * t + 2 * 160 * LATE + 160 * 32 - 1
        skip = -((-A(skip_in)) // 882)
        keep = None if keep_in is None else -((-A(skip_in + keep_in)) // 882) - skip
        assert got["windows"][s][:2] == (skip, keep)
        whole = resample_kit.resample_rule(limited[s], rs[0], rs[1], rs[2])
        want = whole[skip:None if keep is None else skip + keep]
        assert len(want) == (len(whole) - skip if keep is None else keep)
        same_out([got["out"][s]], [want], "slot %d behind the resampler and the trim" % s)


def test_in_front_of_the_feature_stage(tmp_path_factory):
    """mix(-> 1) + limiter with the detector + features: the feature rule over the kit over the mixed mono PCM (linear output: bit for bit)"""
    lib = features_kit.driver(tmp_path_factory.mktemp("features_emu_limit_tp"))
    P = plain_run("stereo", False)
    mix = aacgpu.mix_standard(2, 1)
    basis, fb = features_kit.hostile_tables(64, 33, 5)
    features = dict(frame_length=64, hop=24, pad_left=17, basis=basis, fb=fb, floor=1e-3, log=False)
    mixed = run(P["mem"], P["script"], 2, P["si"], mix=mix)
    ceil = ceiling_of(mixed["out"])
    limited, states = ruled(mixed["out"], P["script"], ceil, GAINS)
    engaged(states)
    want = [features_kit.rule(lib, x[:, 0], 64, 24, 17, basis, fb) for x in limited]
    for way in ("pageable", "planar"):
        got = run(P["mem"], P["script"], 2, P["si"], way=way, mix=mix, features=features, limiter=(ceil, RELEASE), tp=TP, gains=GAINS)
        same_out(got["out"], want, "mix + limiter with the detector + features, %s" % way)


def test_refusals_leave_the_pipeline_as_it_was():
    """aacg_pipeline_set_limiter_true_peak: no limiter, a null config or table, phases or taps outside the limits, an entry that is not
    finite, a second call, a call behind the trim, a call after the first batch; aacg_pipeline_limiter_delay: no limiter, a null pointer.
    Each is refused with a reason, and a pipeline whose call was refused delivers the bits of one that never made it"""
    data, table, _ = load(CASE["stereo48"])
    fr = [packed([table] * 2, [0, 0], [a, a], [3, 3]) for a in (0, 3)]
    slots = np.arange(2, dtype=np.uint32)
    bare = aacgpu.Pipeline(channels=2, max_streams=2, max_frames=3)
    peak = float(np.abs(bare.decode(data, fr[0], slots, 3)[0]).max())
    bare.close()
    lim = (F(4.0 * peak), 0.5)                                          # far above the decode's own peak: gain 1, the stage is a pure delay
    fresh = aacgpu.Pipeline(channels=2, max_streams=2, max_frames=3, limiter=lim)
    want = [fresh.decode(data, f, slots, 3)[0].copy() for f in fr]
    launches = fresh.launch_counts()
    fresh.close()
    good = np.ascontiguousarray(TABLE, F)

    def refused(p, phases, taps, h, null_cfg=False):
        keep = None if h is None else np.ascontiguousarray(h, F)
        cfg = aacgpu.TruePeakConfig(phases, taps, None if keep is None else keep.ctypes.data)
        rc = p.lib.aacg_pipeline_set_limiter_true_peak(p.handle, None if null_cfg else C.byref(cfg))
        assert rc == ERR_INVALID_ARG, (phases, taps, rc)
        reason = p.lib.aacg_pipeline_last_error(p.handle).decode()
        assert reason.startswith("aacg_pipeline_set_limiter_true_peak: ") and len(reason) > len("aacg_pipeline_set_limiter_true_peak: "), reason
        return reason

    n = C.c_uint32(7)
    p = aacgpu.Pipeline(channels=2, max_streams=2, max_frames=3)
    assert "no limiter" in refused(p, 4, 24, good)
    assert p.lib.aacg_pipeline_limiter_delay(p.handle, C.byref(n)) == ERR_INVALID_ARG and n.value == 7
    p.close()

    p = aacgpu.Pipeline(channels=2, max_streams=2, max_frames=3, limiter=lim)
    bad_nan, bad_inf = good.copy(), good.copy()
    bad_nan[3, 23], bad_inf[0, 0] = np.nan, np.inf
    big = np.zeros((9, 64), F)
    reasons = [refused(p, 4, 24, good, null_cfg=True), refused(p, 4, 24, None)]
    reasons += [refused(p, L, 24, big) for L in (0, 9)] + [refused(p, 4, T, big) for T in (0, 2, 6, 68)]
    reasons += [refused(p, 4, 24, bad_nan), refused(p, 4, 24, bad_inf)]
    assert len(set(reasons)) == 6 and "95" in reasons[-2] and "coefficient 0 " in reasons[-1], reasons
    assert p.lib.aacg_pipeline_limiter_delay(p.handle, None) == ERR_INVALID_ARG
    assert p.limiter_delay() == 64 and p.limiter_true_peak is None
    assert same_bits(p.decode(data, fr[0], slots, 3)[0], want[0])
    assert "submitted" in refused(p, 4, 24, good)                       # after the first batch
    assert same_bits(p.decode(data, fr[1], slots, 3)[0], want[1]) and p.launch_counts() == launches and p.limiter_delay() == 64
    p.close()

    p = aacgpu.Pipeline(channels=2, max_streams=2, max_frames=3, limiter=lim, limiter_true_peak=(1, 4, [[0, 0, 1, 0]]))
    assert p.limiter_delay() == 66 and p.limiter_true_peak["taps"] == 4
    assert "already" in refused(p, 4, 24, good)                         # a second call
    # one phase that is the delayed path itself (acc = x[j - 2] exactly, so pt = ps), below the ceiling: the plain limiter's bits, two samples later
    got = p.decode(data, fr[0], slots, 3)[0].reshape(2, 3 * 1024, 2)
    plain = want[0].reshape(2, 3 * 1024, 2)
    assert not got[:, :2].any() and same_bits(got[:, 2:], plain[:, :-2]) and plain.any() and peak > 0
    p.close()
    p = aacgpu.Pipeline(channels=2, max_streams=2, max_frames=3, limiter=lim, trim=True)
    assert "a trim" in refused(p, 4, 24, good)                          # the detector is set in front of the trim, like the limiter
    assert same_bits(p.decode(data, fr[0], slots, 3)[0].reshape(-1)[:want[0].size], want[0].reshape(-1))
    p.close()
    with pytest.raises(aacgpu.AacgError, match="no limiter"):
        aacgpu.Pipeline(channels=2, max_streams=2, max_frames=3, limiter_true_peak=True)
