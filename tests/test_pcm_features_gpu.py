"""The feature stage on the resident route (aacg_pipeline_set_features, aacgpu.Pipeline(features=...)) on a real MI355X: the feature frames
a pipeline with the stage delivers equal the rule of include/aacgpu.h — emu_features_rule, the straight C loop of tests/emu/features_emu.cpp,
on the CPU — applied to the PCM that the SAME configuration delivers WITHOUT the stage, concatenated per slot across the batches: bit for
bit linear, to 4 ulp with log (OpenCL's 3-ulp bound for log10, which the device library follows, plus the reference's own rounding).
Host packed with two lanes in flight and device planar through decode_tensor; a reset in mid-script, a refused frame and a stream learnt
late; the refusals; and the ledger — statuses, refusal counts, launch counts — unchanged.  Every buffer is poisoned first and is larger
than the batch needs."""
import numpy as np
import pytest

import aacgpu
import features_kit as kit
import mix_kit
import resample_kit
from resident_kit import CASES, ERR_INVALID_ARG, load, packed, same_bits

pytestmark = pytest.mark.gpu
CASE = {c["name"]: c for c in CASES}
FLOOR = 1e-3
# three streams over four batches, 1..3 frames each, the third stream absent from the second batch: 7 frames a stream
COUNTS = [[2, 1, 3], [1, 3, 0], [3, 2, 2], [1, 1, 2]]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return kit.driver(tmp_path_factory.mktemp("features_emu"))


def script_of(counts):
    at, out = [0] * len(counts[0]), []
    for row in counts:
        live = [s for s, c in enumerate(row) if c]
        out.append((live, [row[s] for s in live], [at[s] for s in live]))
        for s in live:
            at[s] += row[s]
    return out


def run(members, script, C_, si, max_frames, way="host", mix=None, resample=None, features=None, i16=False, reset=None, lanes=2):
    """the script on a pipeline with or without the stage -> (per-stream (rows, width) arrays, per-stream statuses, refusals in all, launch
    counts).  way "host": pageable host memory, every batch submitted while the one before is in flight (two lanes); "planar": decode_tensor"""
    S = len(members)
    data = np.concatenate([m[0] for m in members])
    bases = np.cumsum([0] + [len(m[0]) for m in members])[:-1]
    tables = [m[1] for m in members]
    kw = dict(output_kind=aacgpu.OUTPUT_I16) if i16 else {}
    p = aacgpu.Pipeline(channels=C_, max_streams=S, max_frames=max_frames, sample_index=si, mix=mix, resample=resample, features=features, lanes=lanes, **kw)
    width = p.features["n_mels"] if features else p.channels
    dtype = np.float32 if features or not i16 else np.int16
    got, status, refusals, pending = [[] for _ in range(S)], [[] for _ in range(S)], 0, []
    rs_clock, ft_clock = [0] * S, [0] * S                     # the test's own count of what each slot's stages have consumed

    def finish(item):
        nonlocal refusals
        ticket, live, counts, n_out, buf = item
        back, res, refused, *lengths = p.collect(ticket)
        assert back is buf and (not lengths or lengths[0].tolist() == n_out)
        total, first = sum(n_out), np.concatenate([[0], np.cumsum(counts)])
        assert np.isnan(buf[total * width:]).all() if dtype == np.float32 else (buf[total * width:] == 0x7F7F).all(), "the elements behind the batch were written"
        parts = np.split(buf[:total * width].copy(), np.cumsum(n_out)[:-1] * width)
        refusals += refused
        for k, s in enumerate(live):
            got[s].append(parts[k].reshape(-1, width))
            status[s].append(res["status"][first[k]:first[k + 1]].copy())

    for b, (live, counts, at) in enumerate(script):
        for s in (reset or {}).get(b, []):
            for item in pending:
                finish(item)
            pending = []
            p.reset_stream(s)
            rs_clock[s] = ft_clock[s] = 0
        fr = packed([tables[s] for s in live], [bases[s] for s in live], at, counts)
        slots, cnt = np.array(live, np.uint32), np.array(counts, np.uint32)
        n_out = [resample_kit.n_out(rs_clock[s], rs_clock[s] + 1024 * c, resample[0], resample[1]) if resample else 1024 * c for s, c in zip(live, counts)]
        for s, c in zip(live, counts):
            rs_clock[s] += 1024 * c
        if features:
            n_in, K, H, P = n_out, p.features["frame_length"], p.features["hop"], p.features["pad_left"]
            n_out = [kit.count(ft_clock[s] + n, K, H, P) - kit.count(ft_clock[s], K, H, P) for s, n in zip(live, n_in)]
            assert p.out_samples(slots, cnt).tolist() == n_out, "aacg_pipeline_out_samples against the formula, in feature frames"
            for s, n in zip(live, n_in):
                ft_clock[s] += n
        total = sum(n_out)
        if way == "host":
            buf = np.empty((total + 64) * width, dtype)
            buf[:] = np.nan if dtype == np.float32 else 0x7F7F
            pending.append((p.submit(data, fr, slots, cnt, pcm=buf), live, counts, n_out, buf))
            if len(pending) == 2:
                finish(pending.pop(0))
        else:
            assert features
            out, lengths, res, refused = p.decode_tensor(data, fr, slots, cnt)
            dev = out.cpu().numpy()
            assert dev.dtype == np.float32 and dev.shape == (len(live), width, max(max(n_out), 1)) and lengths.tolist() == n_out
            refusals += refused
            first = np.concatenate([[0], np.cumsum(counts)])
            for k, s in enumerate(live):
                got[s].append(np.ascontiguousarray(dev[k, :, :n_out[k]].T))
                status[s].append(res["status"][first[k]:first[k + 1]].copy())
                padding = dev[k, :, n_out[k]:]
                if p.features["log"]:
                    want = np.full_like(padding, np.float32(np.log10(np.float64(np.float32(p.features["floor"])))))
                    assert (kit.ulps(padding, want) <= 4).all() and (padding.size == 0 or (padding == padding.flat[0]).all()), "the padding is not log10f(floor)"
                else:
                    assert not padding.view(np.uint32).any(), "the padding is not exactly +0"
    for item in pending:
        finish(item)
    counts_ = p.launch_counts()
    p.close()
    return [np.concatenate(g) for g in got], [np.concatenate(x) for x in status], refusals, counts_


def check(lib, got, plain, features, what, cuts=None):
    """got: a run with the stage; plain: the same configuration's run without it.  The rule over each stream's plain PCM (cut where its
    slot was reset) is what the stage must have delivered; statuses, refusal counts and launch counts are the plain run's"""
    K, H, P = features["frame_length"], features["hop"], features.get("pad_left", 0)
    for s, (y, x) in enumerate(zip(got[0], plain[0])):
        assert x.shape[1] == 1
        pieces = np.split(kit.as_float(x[:, 0]), (cuts or {}).get(s, []))
        mel = np.concatenate([kit.rule(lib, piece, K, H, P, features["basis"], features["fb"]) for piece in pieces])
        assert y.shape == mel.shape and len(mel) > 0, (what, s, y.shape, mel.shape)
        if features.get("log", True):
            worst = int(kit.ulps(y, kit.log_reference(mel, features["floor"])).max())
            print("%s, stream %d: log output within %d ulp of the reference" % (what, s, worst))
            assert worst <= 4, (what, s, worst)
        else:
            kit.same_bits(y, mel, "%s, stream %d" % (what, s))
    for x, y in zip(got[1], plain[1]):
        assert np.array_equal(x, y), what
    assert got[2] == plain[2] and got[3] == plain[3], (what, got[2:], plain[2:])


def committed(name, copies, frames=7):
    c = CASE[name]
    data, table, _ = load(c)
    step = 1 if len(table) >= frames + copies - 1 else 0     # (where the stream is long enough each copy starts a frame later: three different streams)
    return [(data, table[k * step:k * step + frames]) for k in range(copies)], c["channels"], c["sampleIndex"]


def whisper(**kw):
    return dict(aacgpu.features_design(16000, 400, 160, 201, 80), pad_left=200, floor=FLOOR, **kw)


def hostile(K, H, P, B, n_mels, **kw):
    basis, fb = kit.hostile_tables(K, B, n_mels)
    return dict(frame_length=K, hop=H, pad_left=P, basis=basis, fb=fb, floor=FLOOR, **kw)


# (stream, mix to mono, resampler, int16 PCM, the stage's tables)
SETUPS = {"stereo-mono-16k-whisper": ("stereo48", lambda: aacgpu.mix_standard(2, 1), lambda: aacgpu.resample_design(48000, 16000, 32), False, whisper),
          "mono-hostile": ("mono22", None, None, False, lambda **kw: hostile(128, 50, 64, 65, 20, **kw)),
          "int16-mono-hostile": ("stereo48", lambda: mix_kit.hostile_matrix(1, 2) * np.float32(0.25), None, True, lambda **kw: hostile(64, 24, 17, 33, 5, **kw))}
_plain = {}


def plain_run(case):
    """the yardstick, once per configuration: the ways and the log flag share it (and leave it unchanged)"""
    if case not in _plain:
        name, make_mix, make_rs, i16, _ = SETUPS[case]
        mem, C_, si = committed(name, 3)
        mix, rs = make_mix() if make_mix else None, make_rs() if make_rs else None
        _plain[case] = (mem, C_, si, mix, rs, i16, run(mem, script_of(COUNTS), C_, si, 3, mix=mix, resample=rs, i16=i16))
    return _plain[case]


@pytest.mark.parametrize("way", ["host", "planar"])
@pytest.mark.parametrize("case", sorted(SETUPS))
def test_features_are_the_rule_over_the_plain_pipeline(lib, case, way):
    """three streams, ragged batches of 1..3 frames over four batches, two lanes: linear bit for bit, log to 4 ulp"""
    mem, C_, si, mix, rs, i16, want = plain_run(case)
    assert np.abs(want[0][0].astype(np.float64)).max() > (100 if i16 else 1e-3), "the streams are music"
    for log in (False, True):
        features = SETUPS[case][4](log=log)
        got = run(mem, script_of(COUNTS), C_, si, 3, way=way, mix=mix, resample=rs, features=features, i16=i16)
        check(lib, got, want, features, "%s, %s, log %d" % (case, way, log))
        assert got[2] == 0 and all(np.isfinite(g).all() for g in got[0])


def test_a_reset_starts_clock_and_history_again(lib):
    """aacg_pipeline_reset_stream of the second slot in front of the third batch, at 4 frames: from there on its features are the rule over
    the samples since the reset, with zeros in front of them"""
    mem, C_, si = committed("stereo48", 3)
    mix, rs = aacgpu.mix_standard(2, 1), aacgpu.resample_design(48000, 16000, 32)
    features = whisper(log=False)
    want = run(mem, script_of(COUNTS), C_, si, 3, mix=mix, resample=rs, reset={2: [1]})
    got = run(mem, script_of(COUNTS), C_, si, 3, mix=mix, resample=rs, features=features, reset={2: [1]})
    cut = resample_kit.n_out(0, 4 * 1024, rs[0], rs[1])
    check(lib, got, want, features, "reset", cuts={1: [cut]})
    assert len(got[0][1]) == kit.count(cut, 400, 160, 200) + kit.count(len(want[0][1]) - cut, 400, 160, 200)


def test_silence_flows_through_the_stage(lib):
    """three 5.1 streams mixed to one channel — one clean, one whose first frame is malformed (no layout is learnt in the first batch: the
    stream is learnt late), one with a malformed frame behind a learnt layout (a refused frame).  The frames of zeros advance the clock
    and are framed like any other: the rule on zeros"""
    c = CASE["surround48"]
    data, table, _ = load(c)

    def broken(at):
        bad = data.copy()
        off, length = int(table[at]["byte_offset"]), int(table[at]["byte_length"])
        bad[off + 7: off + length] = 0xFF                      # a raw_data_block with none of the stream's elements in it
        return bad

    mem = [(data, table), (broken(0), table), (broken(2), table)]
    script = [([0, 1, 2], [2, 1, 3], [0, 0, 0]), ([0, 1, 2], [3, 4, 2], [2, 1, 3])]
    mix = mix_kit.hostile_matrix(1, 6)
    features = hostile(128, 50, 64, 65, 20, log=False)
    want = run(mem, script, 6, c["sampleIndex"], 4, mix=mix)
    assert want[2] >= 2 and want[1][1][0] != 0 and want[1][2][2] != 0 and not want[1][0].any(), want[1]
    assert not want[0][1][:1024].any() and want[0][1][1024:].any()      # (a refused frame behind music still carries the overlap of the frame before it)
    for way in ("host", "planar"):
        got = run(mem, script, 6, c["sampleIndex"], 4, way=way, mix=mix, features=features)
        check(lib, got, want, features, "silence, %s" % way)
        assert not got[0][1][:kit.count(1024, 128, 50, 64)].any(), "frames over nothing but zeros are not zero"


def test_set_features_refusals_leave_the_pipeline_as_it_was():
    """a limit broken, a null or non-finite table, a floor that is not positive and finite, more than one output channel, a second call, a
    call after the first batch, a mix or a resampler behind the stage; on a pipeline with the stage a planar stride below a stream's count:
    each is refused with a reason before anything is enqueued"""
    import ctypes as C
    import torch
    data, table, _ = load(CASE["mono22"])
    good = hostile(64, 24, 17, 33, 5, log=False)

    def refused(p, **change):
        f = dict(good, **change)
        basis, fb = f["basis"], f["fb"]
        cfg = aacgpu.FeaturesConfig(f["frame_length"], f["hop"], f["pad_left"], f.get("n_rows", 66), f.get("n_mels", 5), 0, f["floor"],
                                    None if basis is None else basis.ctypes.data, None if fb is None else fb.ctypes.data)
        rc = p.lib.aacg_pipeline_set_features(p.handle, C.byref(cfg))
        assert rc == ERR_INVALID_ARG, (change.keys(), rc)
        reason = p.lib.aacg_pipeline_last_error(p.handle).decode()
        assert reason.startswith("aacg_pipeline_set_features: ") and len(reason) > len("aacg_pipeline_set_features: "), reason
        return reason

    big, nan_b, nan_f = np.ones((1028, 1028), np.float32), good["basis"].copy(), good["fb"].copy()
    nan_b[3, 7], nan_f[1, 2] = np.nan, np.inf
    p = aacgpu.Pipeline(channels=1, max_streams=1, max_frames=3, sample_index=7)
    want = [p.decode(data, table[a:a + 3], [0], 3)[0].copy() for a in (0, 3)]
    p.close()
    p = aacgpu.Pipeline(channels=1, max_streams=1, max_frames=3, sample_index=7)
    reasons = [refused(p, frame_length=62, basis=big), refused(p, frame_length=28, basis=big), refused(p, frame_length=1028, basis=big), refused(p, hop=0), refused(p, hop=65),
               refused(p, pad_left=64), refused(p, n_rows=65, basis=big), refused(p, n_rows=0), refused(p, n_rows=1028, basis=big, fb=big), refused(p, n_mels=0),
               refused(p, n_mels=129, fb=big), refused(p, floor=0.0), refused(p, floor=-1.0), refused(p, floor=float("nan")), refused(p, floor=float("inf")),
               refused(p, basis=None), refused(p, fb=None), refused(p, basis=nan_b), refused(p, fb=nan_f)]
    assert len(set(reasons)) == 9, sorted(set(reasons))
    assert p.lib.aacg_pipeline_set_features(p.handle, None) == ERR_INVALID_ARG
    assert p.features is None and p.out_samples([0], 3).tolist() == [3072]
    assert same_bits(p.decode(data, table[:3], [0], 3)[0], want[0])
    assert "submitted" in refused(p)                           # after the first batch
    assert same_bits(p.decode(data, table[3:6], [0], 3)[0], want[1])
    p.close()

    stereo = aacgpu.Pipeline(channels=2, max_streams=1, max_frames=3)
    assert "ONE channel" in refused(stereo)
    stereo.close()
    huge = aacgpu.Pipeline(channels=1, max_streams=128, max_frames=128, sample_index=7, lanes=1)      # 2^14 frames x 1024 / 1 x 128 floats = 2^31
    assert "2^31" in refused(huge, hop=1, n_mels=128, fb=big)
    huge.close()

    p = aacgpu.Pipeline(channels=1, max_streams=1, max_frames=3, sample_index=7, features=good)
    assert "already" in refused(p)                             # a second call
    with pytest.raises(aacgpu.AacgError):
        p.set_mix(np.ones((1, 1), np.float32))                 # the mix comes first
    with pytest.raises(aacgpu.AacgError):
        p.set_resample(*aacgpu.resample_design(22050, 16000, 16))      # ... and the resampler
    n = int(p.out_samples([0], 3)[0])
    assert n == kit.count(3072, 64, 24, 17)
    out = torch.zeros(5 * n, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(aacgpu.AacgError) as e:                 # rows of n - 1 feature frames do not hold the stream's n
        p.submit_device(data, table[:3], [0], 3, out, planar=True, stride_frames=n - 1)
    assert e.value.code == ERR_INVALID_ARG and "stride_frames" in str(e.value)
    with pytest.raises(aacgpu.AacgError) as e:
        p.submit_device(data, table[:3], [0], 3, (out.data_ptr(), 5 * n * 4 - 4))
    assert "d_pcm_bytes" in str(e.value)
    assert int(p.out_samples([0], 3)[0]) == n, "a refused submission moved the clock"
    assert not out.cpu().numpy().any(), "a refused submission wrote the caller's memory"
    p.close()
