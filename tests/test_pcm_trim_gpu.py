"""The trim on the device (aacg_pipeline_set_trim, include/aacgpu.h; aacg_pcm_trim_*): the expected PCM is always the output of the SAME
pipeline WITHOUT the trim — resident_kit.run_script's where that pipeline is not ragged, this file's runner with trim=None where it has a
resampler — concatenated per slot and sliced in numpy by the rule in Python integers (trim_kit).  Every comparison is equality of bits
and of counts.  Every buffer is poisoned and oversized, as tests/test_pcm_resample_gpu.py's are."""
import ctypes as C

import numpy as np
import pytest

import aacgpu
import features_kit
import resample_kit
import trim_kit
from resident_kit import CASES, ERR_CAPACITY, ERR_INVALID_ARG, NODE, OPTIONS, load, members_of, packed, ragged_script, rect_script, run_script, same_bits
from resident_kit import stage_streams          # noqa: F401  (fixture: tests/js/stage_cases.js)
from test_pcm_resample_gpu import is_poison, poison_host, poisoned_device

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not present")]
WAYS = ["pinned", "pageable", "packed", "planar"]
SPEC = dict(tns_spec=True, pns_spec=True, parse_options=OPTIONS)


def stage_kw(i16):
    """how the streams of tests/js/stage_cases.js are decoded: with the spec-correct stages, every frame; int16 PCM does not go with those,
    so there the frames with noise bands are refused and silent — and count their samples like any other"""
    return dict(parse_options=OPTIONS) if i16 else dict(SPEC)


def members(streams, names, copies):
    """resident_kit.members_of over the streams of tests/js/stage_cases.js and, by their names, the committed ones (twelve frames of each):
    without the spec stages every frame of five1_48 and split48 is refused, so int16 PCM of 5.1 that is not silence comes from surround48"""
    committed = {c["name"]: c for c in CASES}
    out = []
    for n in names:
        if n in streams:
            out += members_of(streams, [n], copies)
        else:
            data, table, _ = load(committed[n])
            out += [(data, np.resize(table, 12))] * copies     # (surround48 has five frames: round and round, which decodes like any other order)
    return out


def is_music(x, i16):
    return float(np.abs(x.astype(np.float64)).max()) > (100 if i16 else 1e-3)


class Model:
    """the test's own account of what each slot's stages count: the resampler's clock, the trim's window and position, the feature
    stage's clock, and where in the slot's received samples the position was restarted"""

    def __init__(self, S, resample, trim, features):
        self.rs, self.ft = resample, features
        self.clock, self.Q, self.N, self.received = [0] * S, [0] * S, [0] * S, [0] * S
        self.window = [tuple(trim) if trim else None for _ in range(S)]
        self.cuts = [[(0,) + tuple(trim)] if trim else [] for _ in range(S)]

    def set(self, s, skip, keep):
        self.window[s], self.Q[s] = (skip, keep), 0
        self.cuts[s].append((self.received[s], skip, keep))

    def reset(self, s):
        self.clock[s] = self.Q[s] = self.N[s] = 0
        if self.window[s]:
            self.cuts[s].append((self.received[s],) + self.window[s])

    def batch(self, s, frames):
        """-> what the slot's stream emits for `frames` frames (kept samples, or the feature frames that follow), and the counts move on"""
        n = 1024 * frames
        if self.rs:
            n, self.clock[s] = resample_kit.n_out(self.clock[s], self.clock[s] + n, self.rs[0], self.rs[1]), self.clock[s] + n
        self.received[s] += n
        if self.window[s]:
            n, self.Q[s] = trim_kit.span(self.Q[s], self.window[s][0], self.window[s][1], n)[1], self.Q[s] + n
        if self.ft:
            K, H, P = self.ft["frame_length"], self.ft["hop"], self.ft.get("pad_left", 0)
            n, self.N[s] = features_kit.count(self.N[s] + n, K, H, P) - features_kit.count(self.N[s], K, H, P), self.N[s] + n
        return n


def trim_run(members, script, C_, si, max_frames, way="pageable", trim=None, windows=None, i16=False, ahead=False, actions=None, device_plans=True, **kw):
    """a script of batches on a pipeline with (or, trim None, without) the trim, the output delivered `way`.  trim: (skip, keep) every slot
    starts with; windows: {slot: (skip, keep)} set before the first batch; actions: {batch index: [("set", slot, skip, keep) | ("reset",
    slot)]} in front of that batch; ahead: every batch is submitted before the first is collected.
    -> (per-stream [n x width] arrays, per-stream statuses, refusals in all, launch counts, per-batch {slot: count}, the model's cuts)"""
    S = len(members)
    data = np.concatenate([m[0] for m in members])
    bases = np.cumsum([0] + [len(m[0]) for m in members])[:-1]
    tables = [m[1] for m in members]
    if i16:
        kw["output_kind"] = aacgpu.OUTPUT_I16
    p = aacgpu.Pipeline(channels=C_, max_streams=S, max_frames=max_frames, sample_index=si, device_plans=device_plans, trim=trim, **kw)
    ft = p.features
    width, dtype, unit = (ft["n_mels"], np.float32, 1) if ft else (p.channels, np.int16 if i16 else np.float32, 1024)
    ragged = bool(p.trim or p.resample or ft)
    model = Model(S, p.resample, trim, ft)
    if trim is not None:
        assert p.trim == tuple(trim) and all(p.stream_trim(s) == tuple(trim) + (0,) for s in range(S))
    for s, w in (windows or {}).items():
        p.set_trim(s, *w)
        model.set(s, *w)
        assert p.stream_trim(s) == tuple(w) + (0,)
    got, status, lengths_of, pending, refusals = [[] for _ in range(S)], [[] for _ in range(S)], [], [], [0]

    def finish(item):
        ticket, live, counts, n_out, buf = item
        back, res, refused, *lengths = p.collect(ticket)
        assert back is buf and (not ragged or lengths[0].tolist() == n_out)
        total, first = sum(n_out), np.concatenate([[0], np.cumsum(counts)])
        if way in ("pinned", "pageable"):
            assert is_poison(buf[total * width:]), "the elements behind the batch were written"
            parts = np.split(buf[:total * width].copy(), np.cumsum(n_out)[:-1] * width)
        else:
            dev = buf.cpu().numpy()
            if way == "planar":
                assert is_poison(dev[len(live)]), "the row behind the last stream was written"
                parts = []
                for k in range(len(live)):
                    parts.append(np.ascontiguousarray(dev[k, :, :n_out[k]].T).reshape(-1))
                    assert not dev[k, :, n_out[k]:].view(np.uint16 if dtype == np.int16 else np.uint32).any(), "the padding behind a stream's samples is not exactly zero"
            else:
                assert is_poison(dev[total * width:]), "the elements behind the batch were written"
                parts = np.split(dev[:total * width], np.cumsum(n_out)[:-1] * width)
        refusals[0] += refused
        for k, s in enumerate(live):
            got[s].append(parts[k].reshape(-1, width))
            status[s].append(res["status"][first[k]:first[k + 1]].copy())

    for b, (live, counts, at) in enumerate(script):
        for act in (actions or {}).get(b, []):
            if act[0] == "set":                              # at once, whatever is in flight
                p.set_trim(*act[1:])
                model.set(*act[1:])
                assert p.stream_trim(act[1]) == tuple(act[2:]) + (0,)
            else:
                for item in pending:
                    finish(item)
                pending = []
                p.reset_stream(act[1])
                model.reset(act[1])
                if p.trim:
                    assert p.stream_trim(act[1]) == model.window[act[1]] + (0,), "a reset leaves the window and restarts the position"
        fr = packed([tables[s] for s in live], [bases[s] for s in live], at, counts)
        slots, cnt = np.array(live, np.uint32), np.array(counts, np.uint32)
        n_out = [model.batch(s, c) for s, c in zip(live, counts)]
        assert p.out_samples(slots, cnt).tolist() == n_out, "aacg_pipeline_out_samples against the formula"
        lengths_of.append(dict(zip(live, n_out)))
        total = sum(n_out)
        if way in ("pinned", "pageable"):
            buf = poison_host(p.pinned((total + 64) * width, dtype) if way == "pinned" else np.empty((total + 64) * width, dtype))
            t = p.submit(data, fr, slots, cnt, pcm=buf)
        else:
            planar = way == "planar"
            stride = max((max(n_out) + unit - 1) // unit, 1) + (b % 2)       # (every other batch a row longer than it need be)
            buf = poisoned_device((len(live) + 1, width, stride * unit) if planar else ((total + 64) * width,), dtype == np.int16)
            t = p.submit_device(data, fr, slots, cnt, buf, planar=planar, stride_frames=stride if planar else None)
        if p.trim:
            for s in live:
                assert p.stream_trim(s)[2] == model.Q[s], "the position advances when the batch has been enqueued"
        pending.append((t, live, counts, n_out, buf))
        if not ahead:
            finish(pending.pop())
    for item in pending:
        finish(item)
    counts_ = p.launch_counts()
    p.close()
    return [np.concatenate(g) for g in got], [np.concatenate(x) for x in status], refusals[0], counts_, lengths_of, model.cuts


def expect(got, plain_pcm, plain_status, plain_refusals, what):
    """got: a trim_run; plain_pcm: per slot what the pipeline delivers without the trim, (samples, O)"""
    for s, (y, x) in enumerate(zip(got[0], plain_pcm)):
        want = trim_kit.sliced(x, got[5][s])
        assert same_bits(y, want), "%s: slot %d's trimmed PCM %s differs from the slice %s of the untrimmed pipeline's" % (what, s, y.shape, want.shape)
    for x, y in zip(got[1], plain_status):
        assert np.array_equal(x, y), what
    assert got[2] == plain_refusals, what


_plain = {}


def plain(streams, names, copies, C_, script_key, script, i16, **kw):
    """the yardstick once per configuration: resident_kit.run_script on the same pipeline without the trim; the tests leave it unchanged"""
    key = (tuple(names), copies, script_key, i16, tuple(sorted(kw)))
    if key not in _plain:
        mem = members(streams, names, copies)
        out = run_script(mem, script, C_, 3, 4, True, **dict(kw, **stage_kw(i16), **(dict(output_kind=aacgpu.OUTPUT_I16) if i16 else {})))
        _plain[key] = ([x.reshape(-1, C_) for x in out[0]], out[1], out[2], out[4])
        print("%s x %d, int16 %d: %d refusals, music %s" % (names, copies, i16, out[2], [is_music(x, i16) for x in out[0]]))
    return _plain[key]


WINDOWS = {0: (2112, None), 1: (1, 5000), 2: (0, 0)}          # slot 3 keeps the default


@pytest.mark.parametrize("i16", [False, True], ids=["f32", "i16"])
@pytest.mark.parametrize("way", WAYS)
def test_windows_one_frame_a_batch(stage_streams, way, i16):
    """four stereo slots with the windows (2112, ALL), (1, 5000), (0, 0) and the default, one frame per batch: the first slot's batches 1
    and 2 emit nothing and the third emits 960; the third slot never emits; the second ends in its fifth frame"""
    names = ["stereo48", "split48"]
    script = rect_script(4, 1, 12)
    want = plain(stage_streams, names, 2, 2, "rect1", script, i16)
    got = trim_run(members_of(stage_streams, names, 2), script, 2, 3, 4, way, trim=(0, None), windows=WINDOWS, i16=i16, **stage_kw(i16))
    expect(got, want[0], want[1], want[2], "%s, int16 %d" % (way, i16))
    assert is_music(want[0][0], i16) and is_music(want[0][1], i16), "the slots that keep something hold music"
    per_batch = got[4]
    assert [b[0] for b in per_batch[:4]] == [0, 0, 960, 1024] and all(b[2] == 0 for b in per_batch)
    assert [b[1] for b in per_batch[:6]] == [1023, 1024, 1024, 1024, 905, 0] and all(b[3] == 1024 for b in per_batch)
    assert [len(x) for x in got[0]] == [12 * 1024 - 2112, 5000, 0, 12 * 1024]
    assert got[3] == want[3], "the transform's launches are the untrimmed pipeline's"


@pytest.mark.parametrize("way,i16", [("pinned", True), ("pageable", False), ("packed", False), ("planar", True)])
def test_windows_ragged_batches(stage_streams, way, i16):
    """the same windows over a ragged script, submitted ahead: any split of a stream's frames into batches gives the same bits"""
    names = ["stereo48", "split48"]
    mem = members_of(stage_streams, names, 2)
    script = ragged_script([m[1] for m in mem], 4, np.random.default_rng(11))
    want = plain(stage_streams, names, 2, 2, "ragged11", script, i16)
    got = trim_run(mem, script, 2, 3, 4, way, trim=(0, None), windows=WINDOWS, i16=i16, ahead=True, **stage_kw(i16))
    expect(got, want[0], want[1], want[2], "%s, int16 %d" % (way, i16))
    assert [len(x) for x in got[0]] == [12 * 1024 - 2112, 5000, 0, 12 * 1024]


@pytest.mark.parametrize("way", ["pageable", "packed", "planar"])
@pytest.mark.parametrize("name,channels,skips", [("mono48", 1, (1, 2113)), ("five1_48", 6, (3, 3)), ("surround48", 6, (3, 1025)), ("stereo48", 2, (5, 2112))],
                         ids=["mono", "five1", "surround", "stereo"])
def test_odd_element_alignments(stage_streams, name, channels, skips, way):
    """int16 with odd skips: mono's source begins 2-byte aligned and its neighbour's output at an odd element; 5.1 with skip 3 (five1_48:
    every frame refused, silence that counts its samples like any other; surround48: music)"""
    mem = members(stage_streams, [name], 2)
    script = ragged_script([m[1] for m in mem], 3, np.random.default_rng(5))
    want = plain(stage_streams, [name], 2, channels, "ragged5", [(l, c, a) for l, c, a in script], True)
    windows = {0: (skips[0], 4097), 1: (skips[1], None)}
    got = trim_run(mem, script, channels, 3, 4, way, trim=(0, None), windows=windows, i16=True, **stage_kw(True))
    expect(got, want[0], want[1], want[2], "%s %s" % (name, way))
    assert is_music(want[0][0], True) == (name != "five1_48") and (name == "surround48" or want[2] > 0), "music with refused frames in it; five1_48 all refused"
    assert len(got[0][0]) == 4097 and len(got[0][1]) == 12 * 1024 - skips[1]


@pytest.mark.parametrize("way,i16", [("pageable", False), ("planar", False), ("packed", True), ("pinned", True)])
@pytest.mark.parametrize("rates", [(48000, 16000), (44100, 16000)], ids=["1-3", "160-441"])
def test_behind_mix_limiter_and_resampler(stage_streams, rates, way, i16):
    """5.1 mixed to stereo, gained and limited, resampled by 1 / 3 and by 160 / 441, then trimmed by windows from trim_design: the slice of
    the same pipeline's output without the trim, and aacg_pipeline_out_samples against the formula batch by batch (trim_run)"""
    resample = aacgpu.resample_design(rates[0], rates[1], 32)
    assert resample[:2] == ((1, 3) if rates[0] == 48000 else (160, 441))
    kw = dict(mix=aacgpu.mix_standard(6, 2), limiter=aacgpu.limiter_design(48000, -3.0, 50.0), resample=resample, **stage_kw(i16))
    mem = members(stage_streams, ["surround48" if i16 else "five1_48"], 3)       # (int16 PCM does not go with the spec stages, without which five1_48 is refused)
    script = ragged_script([m[1] for m in mem], 4, np.random.default_rng(3))
    windows = {0: aacgpu.trim_design(2112, None, True, resample)[:2], 1: aacgpu.trim_design(1024, 6000, True, resample)[:2], 2: aacgpu.trim_design(2113, 1, True, resample)[:2]}
    assert windows[0] == trim_kit.design(2112, None, True, resample[0], resample[1], 32)[:2] and windows[0][0] > 0 and windows[1][1] in (6000 * resample[0] // resample[1], 6000 * resample[0] // resample[1] + 1)
    bare = trim_run(mem, script, 6, 3, 4, "pageable", trim=None, i16=i16, **kw)
    got = trim_run(mem, script, 6, 3, 4, way, trim=(0, None), windows=windows, i16=i16, ahead=True, **kw)
    expect(got, bare[0], bare[1], bare[2], "%s %s" % (rates, way))
    assert got[3] == bare[3] and [len(x) for x in got[0]][1:] == [windows[1][1], windows[2][1]]
    assert is_music(bare[0][0], i16), "the streams are music"


@pytest.mark.parametrize("way", ["pageable", "packed", "planar"])
@pytest.mark.parametrize("resampled", [False, True], ids=["48k", "16k"])
def test_features_take_the_kept_range(stage_streams, tmp_path_factory, resampled, way):
    """a feature stage behind the trim: equal to features_kit's rule over the sliced PCM of the same pipeline without trim and features,
    batches that bring the stage no sample included (the first slot's first two, all of the third's); the trim launches nothing"""
    lib = features_kit.driver(tmp_path_factory.mktemp("features_emu_trim_gpu"))
    K, H, P, B, NM = 128, 50, 64, 65, 20
    basis, fb = features_kit.hostile_tables(K, B, NM)
    features = dict(frame_length=K, hop=H, pad_left=P, basis=basis, fb=fb, floor=1e-3, log=False)
    kw = dict(mix=aacgpu.mix_standard(2, 1), **SPEC)
    if resampled:
        kw["resample"] = aacgpu.resample_design(48000, 16000, 16)
    mem = members_of(stage_streams, ["stereo48", "split48"], 2)
    script = rect_script(4, 1, 12) if way == "planar" else ragged_script([m[1] for m in mem], 3, np.random.default_rng(8))
    windows = {0: (2112 // (3 if resampled else 1), None), 1: (1, 1500), 2: (0, 0)}
    bare = trim_run(mem, script, 2, 3, 4, "pageable", trim=None, **kw)
    got = trim_run(mem, script, 2, 3, 4, way, trim=(0, None), windows=windows, features=features, **kw)
    assert any(0 in b.values() for b in got[4]), "some batch emits no feature frame for a stream"
    for s in range(4):
        x = trim_kit.sliced(bare[0][s], got[5][s])
        mel = features_kit.rule(lib, features_kit.as_float(x[:, 0]), K, H, P, basis, fb)
        features_kit.same_bits(got[0][s], mel, "slot %d, %s" % (s, way))
        assert np.array_equal(got[1][s], bare[1][s])
    assert len(got[0][2]) == 0 and len(got[0][3]) > 0 and got[2] == bare[2] and got[3] == bare[3]


@pytest.mark.parametrize("way,i16", [("pinned", False), ("planar", True)])
def test_windows_changed_in_mid_stream(stage_streams, way, i16):
    """one frame per batch, all submitted ahead on five lanes; in front of batch 6 one slot's window is replaced (set_trim: at once,
    whatever is in flight) and another slot is reset (the window stays): both positions restart there"""
    names = ["stereo48", "split48"]
    script = rect_script(4, 1, 12)
    want = plain(stage_streams, names, 2, 2, "rect1", script, i16)
    actions = {6: [("set", 1, 100, 3000), ("reset", 3)]}
    got = trim_run(members_of(stage_streams, names, 2), script, 2, 3, 4, way, trim=(0, None), windows={1: (1, 5000), 3: (700, 2000)}, i16=i16, ahead=True, actions=actions, lanes=5, **stage_kw(i16))
    assert got[5][1] == [(0, 0, None), (0, 1, 5000), (6 * 1024, 100, 3000)] and got[5][3] == [(0, 0, None), (0, 700, 2000), (6 * 1024, 700, 2000)]
    # the reset slot's stream starts again for the transform too: its reference is the plain pipeline with the same reset
    mem = members_of(stage_streams, names, 2)
    data, bases = np.concatenate([m[0] for m in mem]), np.cumsum([0] + [len(m[0]) for m in mem])[:-1]
    p = aacgpu.Pipeline(channels=2, max_streams=4, max_frames=4, device_plans=True, **stage_kw(i16), **(dict(output_kind=aacgpu.OUTPUT_I16) if i16 else {}))
    ref3 = []
    for b, (live, counts, at) in enumerate(script):
        if b == 6:
            p.reset_stream(3)
        pcm = p.decode(data, packed([mem[s][1] for s in live], [bases[s] for s in live], at, counts), np.array(live, np.uint32), np.array(counts, np.uint32))[0]
        ref3.append(pcm.reshape(4, 1024, 2)[3].copy())
    p.close()
    expect(got, want[0][:3] + [np.concatenate(ref3)], want[1], want[2], way)
    assert [len(x) for x in got[0]] == [12 * 1024, 5000 + 3000, 12 * 1024, 2000 + 2000]


def test_default_windows_and_no_stage_change_nothing(stage_streams):
    """the stage with every window at its default delivers, bit for bit and count for count, what the pipeline delivers without it, every
    way; and a pipeline without the stage has the launch counts it had"""
    names = ["stereo48", "split48"]
    mem = members_of(stage_streams, names, 2)
    script = ragged_script([m[1] for m in mem], 4, np.random.default_rng(11))
    for i16, way in ((False, "pinned"), (True, "pageable"), (False, "packed"), (True, "planar")):
        want = plain(stage_streams, names, 2, 2, "ragged11", script, i16)
        got = trim_run(mem, script, 2, 3, 4, way, trim=(0, None), i16=i16, **stage_kw(i16))
        for x, y in zip(got[0], want[0]):
            assert same_bits(x, y)
        assert all(list(b.values()) == [1024 * c for c in counts] for b, (_, counts, _) in zip(got[4], script))
        assert got[2] == want[2] and got[3] == want[3]
        off = trim_run(mem, script, 2, 3, 4, way, trim=None, i16=i16, **stage_kw(i16))
        assert off[3] == want[3] and all(same_bits(x, y) for x, y in zip(off[0], want[0]))


@pytest.mark.parametrize("i16", [False, True], ids=["f32", "i16"])
def test_a_batch_that_keeps_nothing(stage_streams, i16):
    """host and packed buffers are untouched, planar rows are zeros, lengths are zeros (trim_run checks each); the next batch is right"""
    names = ["stereo48", "split48"]
    script = rect_script(4, 2, 12)
    want = plain(stage_streams, names, 2, 2, "rect2", script, i16)
    for way in WAYS:
        got = trim_run(members_of(stage_streams, names, 2), script, 2, 3, 4, way, trim=(4096, 3000), i16=i16, **stage_kw(i16))
        assert [sum(b.values()) for b in got[4]] == [0, 0, 4 * 2048, 4 * 952, 0, 0]
        expect(got, want[0], want[1], want[2], way)


def test_refusals_leave_the_pipeline_as_it_was(stage_streams):
    names = ["stereo48", "split48"]
    mem = members_of(stage_streams, names, 1)
    script = rect_script(2, 2, 12)
    want = plain(stage_streams, names, 1, 2, "rect2x2", script, False)
    data, bases = np.concatenate([m[0] for m in mem]), np.cumsum([0] + [len(m[0]) for m in mem])[:-1]
    lib = aacgpu.load_library()
    ALL = aacgpu.TRIM_ALL

    def refused(p, rc, fragment, code=ERR_INVALID_ARG):
        assert rc == code and fragment in lib.aacg_pipeline_last_error(p.handle).decode(), (rc, lib.aacg_pipeline_last_error(p.handle))

    def batch(p, b):
        live, counts, at = script[b]
        return p.decode(data, packed([mem[s][1] for s in live], [bases[s] for s in live], at, counts), np.array(live, np.uint32), np.array(counts, np.uint32))

    p = aacgpu.Pipeline(channels=2, max_streams=2, max_frames=4, device_plans=True, **SPEC)
    # no stage yet: the per-stream calls say so
    refused(p, lib.aacg_pipeline_set_stream_trim(p.handle, 0, 0, ALL), "the pipeline has no trim")
    with pytest.raises(aacgpu.AacgError):
        p.stream_trim(0)
    refused(p, lib.aacg_pipeline_set_trim(p.handle, None), "no configuration")
    for skip, keep in ((2 ** 40, ALL), (0, 2 ** 40), (2 ** 63, 5), (0, ALL - 1)):
        refused(p, lib.aacg_pipeline_set_trim(p.handle, C.byref(aacgpu.TrimConfig(skip, keep))), "2^40")
    assert p.trim is None and len(batch(p, 0)) == 3, "the pipeline is as it was: no trim, a plain batch"
    refused(p, lib.aacg_pipeline_set_trim(p.handle, C.byref(aacgpu.TrimConfig(0, ALL))), "a batch has been submitted")
    assert same_bits(batch(p, 1)[0].reshape(2, 2048, 2)[1], want[0][1][2048:4096])
    p.close()

    p = aacgpu.Pipeline(channels=2, max_streams=2, max_frames=4, device_plans=True, trim=(2112, None), **SPEC)
    refused(p, lib.aacg_pipeline_set_trim(p.handle, C.byref(aacgpu.TrimConfig(0, ALL))), "has a trim already")
    refused(p, lib.aacg_pipeline_set_mix(p.handle, 1, aacgpu.mix_standard(2, 1).ctypes.data), "has a trim already")
    refused(p, lib.aacg_pipeline_set_limiter(p.handle, C.byref(aacgpu.LimiterConfig(0.5, 0.5))), "has a trim already")
    L, M, table = aacgpu.resample_design(48000, 16000, 8)
    refused(p, lib.aacg_pipeline_set_resample(p.handle, L, M, 8, table.ctypes.data), "has a trim already")
    refused(p, lib.aacg_pipeline_set_stream_trim(p.handle, 2, 0, ALL), "slot out of range")
    refused(p, lib.aacg_pipeline_set_stream_trim(p.handle, 0, 2 ** 40, ALL), "2^40")
    refused(p, lib.aacg_pipeline_set_stream_trim(p.handle, 0, 0, 2 ** 40), "2^40")
    assert lib.aacg_pipeline_stream_trim(p.handle, 2, None, None, None) == ERR_INVALID_ARG
    assert p.stream_trim(0) == (2112, None, 0) and p.stream_trim(1) == (2112, None, 0) and p.channels == 2
    # a planar batch whose rows are too short for what a stream keeps, a stride outside 1..2^21, a buffer too small: refused, positions unmoved
    import torch
    live, counts, at = script[0]
    fr, slots, cnt = packed([mem[s][1] for s in live], [bases[s] for s in live], at, counts), np.array(live, np.uint32), np.array(counts, np.uint32)
    p.set_trim(1, 0, None)
    assert p.out_samples(slots, cnt).tolist() == [0, 2048]
    out = torch.zeros((2, 2, 2048), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for stride, fragment, code in ((1, "below a stream's trimmed count", ERR_INVALID_ARG), (0, "not in 1..2^21", ERR_INVALID_ARG), ((1 << 21) + 1, "not in 1..2^21", ERR_INVALID_ARG),
                                   (3, "smaller than the batch needs", ERR_CAPACITY)):
        with pytest.raises(aacgpu.AacgError) as e:
            p.submit_device(data, fr, slots, cnt, out, planar=True, stride_frames=stride)
        assert e.value.code == code and fragment in str(e.value), (stride, str(e.value))
    assert p.stream_trim(0)[2] == 0 and p.stream_trim(1)[2] == 0 and not out.cpu().numpy().any(), "a refused submission leaves the positions alone and writes nothing"
    # ... and then good batches that are right: slot 0 keeps from 2112 on, slot 1 everything
    parts = [[], []]
    for b in range(len(script)):
        pcm, res, n_refused, lengths = batch(p, b)
        ends = np.cumsum(lengths) * 2
        parts[0].append(pcm[:ends[0]].reshape(-1, 2))
        parts[1].append(pcm[ends[0]:ends[1]].reshape(-1, 2))
    assert same_bits(np.concatenate(parts[0]), want[0][0][2112:]) and same_bits(np.concatenate(parts[1]), want[0][1])
    assert p.stream_trim(0) == (2112, None, 12 * 1024)
    p.close()


def test_decode_tensor_follows_the_trimmed_counts(stage_streams):
    names = ["stereo48", "split48"]
    mem = members_of(stage_streams, names, 1)
    script = rect_script(2, 3, 12)
    want = plain(stage_streams, names, 1, 2, "rect3x2", script, False)
    data, bases = np.concatenate([m[0] for m in mem]), np.cumsum([0] + [len(m[0]) for m in mem])[:-1]
    p = aacgpu.Pipeline(channels=2, max_streams=2, max_frames=4, device_plans=True, trim=True, **SPEC)
    p.set_trim(0, 2112)
    p.set_trim(1, 5000, 10)
    live, counts, at = script[0]
    fr = packed([mem[s][1] for s in live], [bases[s] for s in live], at, counts)
    t, lengths, res, n_refused = p.decode_tensor(data, fr, np.array(live, np.uint32), np.array(counts, np.uint32))
    assert tuple(t.shape) == (2, 2, 1024) and lengths.tolist() == [960, 0]
    got = t.cpu().numpy()
    assert same_bits(np.ascontiguousarray(got[0, :, :960].T), want[0][0][2112:3072]) and not got[0, :, 960:].any() and not got[1].any()
    live, counts, at = script[1]
    fr = packed([mem[s][1] for s in live], [bases[s] for s in live], at, counts)
    t, lengths, res, n_refused = p.decode_tensor(data, fr, np.array(live, np.uint32), np.array(counts, np.uint32), planar=False)
    assert tuple(t.shape) == (3072 + 10, 2) and lengths.tolist() == [3072, 10]
    assert same_bits(t.cpu().numpy(), np.concatenate([want[0][0][3072:6144], want[0][1][5000:5010]]))
    p.close()
