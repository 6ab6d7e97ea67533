"""Every PCM stage of the resident route at a product-sized batch, past its grid cap, on a real MI355X: the batch of product_batch_kit.py —
stereo48 in 320 slots of twelve classes of (first frame, count), 4640 frames in the first batch, a ragged second batch with gaps in the
slot list submitted while the first is in flight — through the mix, the planar tail, the limiter, the resampler, the trim, the meter with
the true-peak stage, the feature stage, the concealment, and all that compose in one chain.

The yardstick shares no code with the kernels: the twelve classes' plain PCM from a pipeline of twelve slots without any stage (held to
the committed oracle PCM by resident_kit.close_to), the kits' rules over it — continued across the two batches, which the rules do by
being causal: a class's expected output is the rule over all the class receives — and every one of the 320 slots compared with its
class's expected output by the stage's own comparison: bit for bit; log feature frames to the project's 4 ulp against
features_kit.log_reference and bit-identical within a class.  Counts are held to the formulas batch by batch (product_batch_kit.Counts).
Every destination is poisoned and larger than the batch needs.  No tolerance is introduced here.

Each test first asserts, from the numbers, that its launch passes the stage's cap on workgroups (AACG_*_MAX_BLOCKS, restated below next
to the header each comes from), so that a workgroup makes more than one trip through its grid-stride loop.  The limiter (groups of 4
streams under a cap of 4096) and the meter (groups of 64 / C streams under 4096) cannot reach theirs from the API — nor can
aacg_units_carry_shape —: they run here at 80 and 10 workgroups where the small tests run 1 or 2, and their second trip stays with the
lane emulator."""
import numpy as np
import pytest

import aacgpu
import conceal_kit
import features_kit
import limiter_kit
import loudness_kit
import mix_kit
import product_batch_kit as kit
import resample_kit
import trim_kit
import truepeak_kit
from product_batch_kit import CLASSES, S, every_slot, first_count, second_count

pytestmark = pytest.mark.gpu
F = np.float32

# the caps, and what a workgroup takes per trip
MIX_MAX_BLOCKS, MIX_THREADS = 2048, 256                     # aacg_pcm_mix.h: AACG_MIX_MAX_BLOCKS, AACG_MIX_THREADS; an item is 16 bytes of every channel
PLANAR_MAX_BLOCKS, PLANAR_THREADS = 2048, 256               # aacg_pcm_planar.h: AACG_PLANAR_MAX_BLOCKS, AACG_PLANAR_THREADS
CONCEAL_MAX_BLOCKS, CONCEAL_WAVES = 2048, 4                 # aacg_units_conceal.h: AACG_CONCEAL_MAX_BLOCKS, AACG_CONCEAL_THREADS / 64; a job per wave
RESAMPLE_MAX_BLOCKS = 4096                                  # aacg_pcm_resample.h: AACG_RESAMPLE_MAX_BLOCKS; a frame per workgroup
TRUEPEAK_MAX_BLOCKS = 4096                                  # aacg_pcm_truepeak.h: AACG_TRUEPEAK_MAX_BLOCKS; a frame per workgroup
TRIM_MAX_BLOCKS, TRIM_TILE = 4096, 512                      # aacg_pcm_trim.h: AACG_TRIM_MAX_BLOCKS, AACG_TRIM_TILE; an item per workgroup
FEATURES_MAX_BLOCKS, FEATURES_TILE = 4096, 16               # aacg_pcm_features.h: AACG_FEATURES_MAX_BLOCKS, AACG_FEATURES_TILE; an item per workgroup
LIMIT_MAX_BLOCKS, LIMIT_WAVES = 4096, 4                     # aacg_pcm_limit.h: AACG_LIMIT_MAX_BLOCKS, AACG_LIMIT_WAVES; a stream per wave
LOUDNESS_MAX_BLOCKS = 4096                                  # aacg_pcm_loudness.h: AACG_LOUDNESS_MAX_BLOCKS; 64 / C streams per workgroup
N1 = kit.first_batch_frames()                               # 4640

GAINS = [1.0, 4.0, 2.5, 0.5, 6.0, 1.5, 3.0, 8.0, 0.75, 2.0, 5.0, 1.25]      # by class: neighbouring slots differ
RELEASE = 0.0625
METER = {"hop": 1000, "coeffs": loudness_kit.hostile_coeffs(3)}           # a hop that straddles frames and batches


def by_slot(per_class):
    return {s: per_class[s % CLASSES] for s in range(S)}


def mix_items(frames, i16):
    return frames * (1024 // (8 if i16 else 4))


def ceiling_of(pcm):
    """half the largest sample of the unlimited PCM, in full-scale units: the limiter demonstrably engages"""
    peak = max(float(np.abs(x.astype(np.float64)).max()) for x in pcm)
    return F(0.5 * peak / (32768.0 if pcm[0].dtype == np.int16 else 1.0))


def limited(pcm, ceiling):
    """limiter_kit.rule per class with the class's gain over all the class receives, cut where its batches meet (the state carries)"""
    out, under, at = [], 0, 0
    for c, x in enumerate(pcm):
        state, n1 = limiter_kit.State(x.shape[1]), 1024 * first_count(c)
        out.append(np.concatenate([limiter_kit.rule(x[:n1], GAINS[c], ceiling, RELEASE, state), limiter_kit.rule(x[n1:], GAINS[c], ceiling, RELEASE, state)]))
        under, at = under + state.engaged()[0], at + state.engaged()[1]
    assert under > 0 and at > 0, "the kit never limited, or always: the case does not test what it is for"
    return out


_meter = {}


def metered():
    """(loudness_kit.rule's records, truepeak_kit.rule's) per class over the plain float PCM.  The meter's rule is a loop over samples
    whose channels run side by side: the twelve classes go through it as 24 channels of one evaluation, each padded with zeros behind
    its end, and a class takes the records its own samples complete"""
    if not _meter:
        pcm = kit.plain()
        n = max(len(x) for x in pcm)
        side = np.concatenate([np.concatenate([x, np.zeros((n - len(x), 2), F)]) for x in pcm], axis=1)
        rec = loudness_kit.rule(side, METER["hop"], METER["coeffs"], loudness_kit.State(2 * CLASSES))
        _meter["records"] = [np.ascontiguousarray(rec[:len(x) // METER["hop"], 2 * c:2 * c + 2]) for c, x in enumerate(pcm)]
        table = truepeak_kit.mixed_table(4, 12)
        _meter["stage"] = {"phases": 4, "taps": 12, "table": table}
        _meter["peaks"] = []
        for c, x in enumerate(pcm):
            state, n1 = truepeak_kit.State(2, 12), 1024 * first_count(c)
            _meter["peaks"].append(np.concatenate([truepeak_kit.rule(x[:n1], METER["hop"], table, state), truepeak_kit.rule(x[n1:], METER["hop"], table, state)]))
    return _meter


def clean(got):
    assert got["refusals"] == 0 and not any(x.any() for x in got["status"]), "every frame of the committed stream decodes"
    assert got["launches"]["shaped"] == 2, "both batches' plans were shaped on the device"


# ---- 1. the mix ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_channels,i16,way", [(2, False, "pageable"), (2, True, "packed"), (1, False, "packed"), (1, True, "pageable")],
                         ids=["stereo-f32-pageable", "stereo-i16-packed", "mono-f32-packed", "mono-i16-pageable"])
def test_mix(out_channels, i16, way):
    """stereo through mix_kit.hostile_matrix(2, 2), and to mono: mix_kit.mix_rule over the class's plain PCM, every slot"""
    assert mix_items(N1, i16) > MIX_MAX_BLOCKS * MIX_THREADS, "the mix's workgroups make one trip"
    mix = mix_kit.hostile_matrix(out_channels, 2)
    want = [mix_kit.mix_rule(x, mix) for x in kit.plain(i16)]
    got = kit.run(S, way, i16, mix=mix)
    clean(got)
    every_slot(got["out"], want, "mix to %d, %s" % (out_channels, way))
    assert [len(x) for x in got["out"][:CLASSES]] == [1024 * (first_count(c) + second_count(c)) for c in range(CLASSES)]


# ---- 2. the planar tail -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i16", [False, True], ids=["f32", "i16"])
def test_planar_tail(i16):
    """the plain pipeline into [stream][channel][16 * 1024] on the device (submit_device, planar, stride_frames 16): the class's plain
    PCM, exact zeros behind every short stream's samples (kit.run checks them), the row behind the last stream untouched; and, f32,
    decode_tensor's tensors and lengths for the same two batches"""
    rows = S * kit.MAX_FRAMES
    want_blocks = rows * mix_items(1, i16) // PLANAR_THREADS
    assert want_blocks > PLANAR_MAX_BLOCKS and rows > (4096 if i16 else 2048), "the planar tail's workgroups make one trip"
    want = kit.plain(i16)
    got = kit.run(S, "planar", i16)
    clean(got)
    every_slot(got["out"], want, "planar, stride 16")
    if i16:
        return
    data, table, _ = kit.stream()
    p = aacgpu.Pipeline(channels=2, max_streams=S, max_frames=kit.MAX_FRAMES, sample_index=3, device_plans=True, lanes=2)
    parts = [[] for _ in range(S)]
    for live, counts, at in kit.script(S):
        t, lengths, res, refused = p.decode_tensor(data, kit.packed([table] * len(live), [0] * len(live), at, counts), np.array(live, np.uint32), np.array(counts, np.uint32))
        assert tuple(t.shape) == (len(live), 2, 1024 * max(counts)) and lengths.tolist() == [1024 * c for c in counts] and refused == 0
        host = t.cpu().numpy()
        for k, s in enumerate(live):
            parts[s].append(np.ascontiguousarray(host[k, :, :1024 * counts[k]].T))
            assert not host[k, :, 1024 * counts[k]:].view(np.uint32).any(), "decode_tensor: the padding behind slot %d's samples is not exactly zero" % s
    p.close()
    every_slot([np.concatenate(x) for x in parts], want, "decode_tensor")


# ---- 3. the limiter -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i16,way", [(False, "pageable"), (True, "packed"), (False, "planar")], ids=["f32-pageable", "i16-packed", "f32-planar"])
def test_limiter(i16, way):
    """a gain per slot that differs between neighbours (GAINS by class, up to 8) under a ceiling of half the plain PCM's peak:
    limiter_kit.rule over the class's plain PCM.  The limiter's cap cannot be reached — a workgroup takes 4 streams, the cap is 4096
    workgroups — so this is 80 workgroups in one trip where the small tests run 1; the emulator alone covers its second trip"""
    groups = (S + LIMIT_WAVES - 1) // LIMIT_WAVES
    assert groups == 80 and groups < LIMIT_MAX_BLOCKS
    pcm = kit.plain(i16)
    ceiling = ceiling_of(pcm)
    want = limited(pcm, ceiling)
    got = kit.run(S, way, i16, gains=by_slot(GAINS), limiter=(ceiling, RELEASE))
    clean(got)
    every_slot(got["out"], want, "limiter, %s" % way)


# ---- 4. the resampler ---------------------------------------------------------------------------------------------------------------
RESAMPLERS = {"1-3": lambda: aacgpu.resample_design(48000, 16000, 32), "160-147": lambda: (160, 147, resample_kit.hostile_table(160, 8))}


@pytest.mark.parametrize("way,i16", [("packed", False), ("planar", True)], ids=["packed-f32", "planar-i16"])
@pytest.mark.parametrize("ratio", sorted(RESAMPLERS))
def test_resampler(ratio, way, i16):
    """1 : 3 with the designed table of 32 taps, and up by 160 / 147 with a hostile table of 8: resample_kit.resample_rule over all the
    class receives — the second batch continues from the history that the first batch's workgroups wrote, the late trips' among them"""
    assert N1 > RESAMPLE_MAX_BLOCKS, "the resampler's workgroups make one trip"
    L, M, table = rs = RESAMPLERS[ratio]()
    assert (L, M, table.shape[1]) == ((1, 3, 32) if ratio == "1-3" else (160, 147, 8))
    want = [resample_kit.resample_rule(x, L, M, table) for x in kit.plain(i16)]
    got = kit.run(S, way, i16, resample=rs)
    clean(got)
    every_slot(got["out"], want, "resampler %s, %s" % (ratio, way))
    assert all(got["lengths"][1].get(s, 0) > 0 for s in kit.script(S)[1][0])


# ---- 5. the trim --------------------------------------------------------------------------------------------------------------------
def windows(scale=1, first_of=lambda c: 1024 * first_count(c)):
    """a window per class, in samples of what the stage receives (scale: how many source samples make one): one keeps nothing, one begins
    inside the second batch (class 3 has one), the rest keep most of what comes, with odd skips and ends inside either batch"""
    w = [(2112, None), (1, 5000), (0, 0), None, (5, None), (3, 15000), (1025, None), (0, None), (700, 12001), (2113, None), (1, None), (4097, 9000)]
    w = [None if x is None else (x[0] // scale, None if x[1] is None else x[1] // scale) for x in w]
    w[3] = (first_of(3) + 33, None)
    assert second_count(3) > 0
    return w


def trimmed(pcm, w):
    return [trim_kit.sliced(x, [(0,) + w[c]]) for c, x in enumerate(pcm)]


def trim_lengths(got, w, n_in_of):
    """trim_kit.counts and aacg_trim_counts against what each batch delivered, per slot"""
    for s in range(S):
        c = s % CLASSES
        n_in = n_in_of(c)
        first, kept = trim_kit.counts(0, w[c][0], w[c][1], n_in)
        lib_first, lib_kept = aacgpu.trim_counts(0, w[c][0], w[c][1], n_in)
        assert lib_first.tolist() == first and lib_kept.tolist() == kept
        assert [got["lengths"][b][s] for b in range(len(n_in))] == kept, "slot %d's batches keep other counts than the rule's" % s


@pytest.mark.parametrize("way,i16", [("packed", False), ("planar", True), ("planar", False)], ids=["packed-f32", "planar-i16", "planar-f32"])
def test_trim_at_the_source_rate(way, i16):
    """no resampler, most samples kept: the items of 512 kept samples pass the cap.  trim_kit.sliced over the class's plain PCM"""
    w = windows()
    items = sum(-(-trim_kit.span(0, w[s % CLASSES][0], w[s % CLASSES][1], 1024 * first_count(s))[1] // TRIM_TILE) for s in range(S))
    assert items > TRIM_MAX_BLOCKS, "the trim's workgroups make one trip"
    want = trimmed(kit.plain(i16), w)
    got = kit.run(S, way, i16, windows=by_slot(w), trim=True)
    clean(got)
    every_slot(got["out"], want, "trim, %s" % way)
    trim_lengths(got, w, lambda c: [1024 * first_count(c)] + [1024 * second_count(c)] * (second_count(c) > 0))
    assert len(want[2]) == 0 and got["lengths"][0][3] == 0 and got["lengths"][1][3] == 2048 - 33, "a window that keeps nothing, and one that begins inside the second batch"


def test_trim_behind_the_resampler():
    """behind the 1 : 3 resampler the items stay under the cap: this is the per-stream records of 320 streams, the resampler's and the
    trim's side by side in one staging block"""
    L, M, table = rs = RESAMPLERS["1-3"]()
    n1 = lambda c: resample_kit.n_out(0, 1024 * first_count(c), L, M)
    n2 = lambda c: resample_kit.n_out(1024 * first_count(c), 1024 * (first_count(c) + second_count(c)), L, M)
    w = windows(3, n1)
    want = trimmed([resample_kit.resample_rule(x, L, M, table) for x in kit.plain()], w)
    got = kit.run(S, "packed", False, windows=by_slot(w), resample=rs, trim=True)
    clean(got)
    every_slot(got["out"], want, "trim behind the resampler")
    trim_lengths(got, w, lambda c: [n1(c)] + [n2(c)] * (second_count(c) > 0))
    assert got["lengths"][0][3] == 0 and got["lengths"][1][3] == n2(3) - 33


# ---- 6. the meter with the true-peak stage ------------------------------------------------------------------------------------------
def test_loudness_and_true_peak():
    """a hop of 1000 samples straddles frames, so the per-hop maxima go through the atomic-maximum path, and 16 - s % 4 frames are no
    whole number of hops, so the partial energy, peak and true peak carry into the second batch: every slot's records of both batches
    against loudness_kit.rule and truepeak_kit.rule over the class's plain PCM, the counts against the formula (kit.run), and the PCM
    that leaves beside them untouched.  The true-peak stage passes its cap (a frame per workgroup); the meter cannot reach its own — a
    workgroup takes 64 / C = 32 streams, the cap is 4096 workgroups —: 10 workgroups in one trip where the small tests run 1, and the
    emulator alone covers its second trip"""
    assert N1 > TRUEPEAK_MAX_BLOCKS, "the true-peak stage's workgroups make one trip"
    groups = (S + 64 // 2 - 1) // (64 // 2)
    assert groups == 10 and groups < LOUDNESS_MAX_BLOCKS
    assert all((1024 * first_count(c)) % METER["hop"] for c in range(CLASSES)), "every class carries a partial hop across the batches"
    want = metered()
    got = kit.run(S, "packed", False, loudness=METER, true_peak=want["stage"])
    clean(got)
    every_slot(got["out"], kit.plain(), "the PCM beside the meter")
    every_slot(got["records"], want["records"], "the meter's records")
    every_slot(got["peaks"], want["peaks"], "the true-peak records", same=truepeak_kit.same_records)
    assert [len(x) for x in got["records"][:CLASSES]] == [1024 * (first_count(c) + second_count(c)) // METER["hop"] for c in range(CLASSES)]
    assert got["records"][0][:, :, 0].max() > 0 and got["peaks"][0].max() > 0, "the streams are music"


# ---- 7. the feature stage -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return features_kit.driver(tmp_path_factory.mktemp("features_emu_product"))


def check_features(lib, got, mono, features, what):
    """linear: features_kit.rule over the class's mono PCM, bit for bit.  log: within the project's 4 ulp of features_kit.log_reference
    over that, and the slots of a class bit-identical to one another"""
    K, H, P = features["frame_length"], features["hop"], features["pad_left"]
    mel = [features_kit.rule(lib, np.ascontiguousarray(x[:, 0]), K, H, P, features["basis"], features["fb"], features["floor"]) for x in mono]
    assert all(len(m) > 0 for m in mel)
    if not features["log"]:
        every_slot(got["out"], mel, what)
        return
    ref = [features_kit.log_reference(m, features["floor"]) for m in mel]

    def near(x, y, where):
        worst = int(features_kit.ulps(x, y).max())
        assert worst <= 4, "%s: log output %d ulp from the reference" % (where, worst)

    every_slot(got["out"], ref, what, same=near)
    every_slot(got["out"], got["out"][:CLASSES], what + ", a class's slots against its first")


@pytest.mark.parametrize("log,way", [(False, "packed"), (True, "planar"), (False, "planar"), (True, "pageable")], ids=["linear-packed", "log-planar", "linear-planar", "log-pageable"])
def test_features_with_a_small_hop(lib, log, way):
    """a hostile stage of K = 32, H = 8, pad 5, 17 bins and 3 mel bands over the mono mix: some 2000 feature frames a stream, about 128
    items of 16, so the items pass the cap tenfold"""
    basis, fb = features_kit.hostile_tables(32, 17, 3)
    features = dict(frame_length=32, hop=8, pad_left=5, basis=basis, fb=fb, floor=1e-3, log=log)
    items = sum(-(-features_kit.count(1024 * first_count(s), 32, 8, 5) // FEATURES_TILE) for s in range(S))
    assert items > FEATURES_MAX_BLOCKS, "the feature stage's workgroups make one trip"
    mix = aacgpu.mix_standard(2, 1)
    mono = [mix_kit.mix_rule(x, mix) for x in kit.plain()]
    got = kit.run(S, way, False, mix=mix, features=features)
    clean(got)
    check_features(lib, got, mono, features, "small hop, log %d, %s" % (log, way))


@pytest.mark.parametrize("log,way", [(True, "pageable"), (False, "planar")], ids=["log-pageable", "linear-planar"])
def test_features_whisper_behind_mix_and_resampler(lib, log, way):
    """the Whisper design (400 / 160 at 16 kHz, 80 mel bands) behind the mono mix and the 1 : 3 resampler: some 34 feature frames a
    stream, a few items each — the per-stream records of 320 streams rather than the cap"""
    features = dict(aacgpu.features_design(16000, 400, 160, 201, 80), pad_left=200, floor=1e-3, log=log)
    mix, (L, M, table) = aacgpu.mix_standard(2, 1), RESAMPLERS["1-3"]()
    mono = [resample_kit.resample_rule(mix_kit.mix_rule(x, mix), L, M, table) for x in kit.plain()]
    got = kit.run(S, way, False, mix=mix, resample=(L, M, table), features=features)
    clean(got)
    check_features(lib, got, mono, features, "whisper, log %d, %s" % (log, way))


# ---- 8. the concealment -------------------------------------------------------------------------------------------------------------
FADE, HOLD, PERIOD = 2, 3, 60                               # the drops repeat with the classes and with every fifth slot


def drops_of(s):
    """every fifth slot loses one frame of its first batch, at a place that differs by class and never the first, and — if it has one —
    the first frame of its second batch: the state that conceals that one was written by the first batch's job of the slot's last
    frame, a late-trip job for the slots in the back"""
    if s % 5:
        return []
    at = 2 + (s % CLASSES) % 11
    assert 0 < at < first_count(s)
    return [kit.start(s) + at] + ([kit.start(s) + first_count(s)] if second_count(s) else [])


@pytest.mark.parametrize("i16,way", [(False, "pageable"), (True, "planar")], ids=["f32-pageable", "i16-planar"])
def test_concealment(i16, way):
    """device plans, a fade of 2 steps and a hold of 3.  The PCM of every slot against conceal_kit's host route (parse on the host, the
    numpy rule over the records, a plan per batch, decode_pipelined) over the same tables in 60 slots — the period of classes and drops —,
    bit for bit; statuses, flags, refusal and concealed counts as tests/test_units_conceal_gpu.py holds them"""
    Cp, longest = 2, max(first_count(s) for s in range(S))
    jobs = S * longest * Cp
    assert jobs // CONCEAL_WAVES > CONCEAL_MAX_BLOCKS, "the concealment's workgroups make one trip"
    late = [s for s in range(S) if drops_of(s) and second_count(s) and (s * longest + first_count(s) - 1) * Cp >= CONCEAL_MAX_BLOCKS * CONCEAL_WAVES]
    assert late, "a slot whose state a late-trip job wrote conceals a frame of the second batch"
    data, table, _ = kit.stream()
    tables = [conceal_kit.dropped(table, drops_of(s)) for s in range(S)]
    assert all(drops_of(s) == drops_of(s % PERIOD) and s % CLASSES == (s % PERIOD) % CLASSES for s in range(S))
    host = conceal_kit.ConcealRoute(PERIOD, 2, 3, FADE, HOLD, None, carry=False, i16=i16)
    want = [[] for _ in range(PERIOD)]
    for live, counts, at in kit.script(PERIOD):
        pcm, _, _ = host.decode(data, kit.packed([tables[s] for s in live], [0] * len(live), at, counts), live, counts)
        first = np.concatenate([[0], np.cumsum(counts)]) * 2048
        for k, s in enumerate(live):
            want[s].append(pcm[first[k]:first[k + 1]].reshape(-1, 2))
    host.close()
    want = [np.concatenate(x) for x in want]
    got = kit.run(S, way, i16, tables=tables, conceal=dict(fade_steps=FADE, hold_frames=HOLD))
    n_drops = sum(len(drops_of(s)) for s in range(S))
    assert host.refused == host.concealed == sum(len(drops_of(s)) for s in range(PERIOD))
    assert got["refusals"] == n_drops and got["concealed"] == n_drops, "every dropped frame has a good frame in front of it, within the hold"
    for s in range(S):
        h = s % PERIOD
        local = [d - kit.start(s) for d in drops_of(s)]
        assert np.flatnonzero(got["status"][s]).tolist() == local, "slot %d's refused frames are not exactly the dropped ones" % s
        assert np.array_equal(got["status"][s], np.concatenate(host.statuses[h])), "slot %d" % s
        marked = np.flatnonzero(got["flags"][s] & aacgpu.PARSE_CONCEALED).tolist()
        assert marked == local == np.flatnonzero(np.concatenate(host.flags[h]) & aacgpu.PARSE_CONCEALED).tolist(), "slot %d" % s
        x, y = got["out"][s], want[h]
        assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(kit.bits(x), kit.bits(y)), \
            "slot %d: the device's concealed frames decode to other bits than the host route's" % s
    clean_pcm = kit.plain(i16)
    for s in range(S):
        if not drops_of(s):
            assert np.array_equal(kit.bits(got["out"][s]), kit.bits(clean_pcm[s % CLASSES])), "slot %d lost no frame and is not the plain PCM" % s
        elif not i16:                                           # (the stream has passages below half an int16 step)
            f = drops_of(s)[0] - kit.start(s)
            assert got["out"][s][1024 * f:1024 * (f + 1)].any(), "slot %d's dropped frame went silent" % s


# ---- 9. one chain -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("way", ["packed", "planar"])
def test_one_chain(way):
    """mix -> limiter -> resampler -> trim with the meter and the true-peak stage, the combination tests/test_pcm_truepeak_gpu.py and
    tests/test_pcm_trim_gpu.py build small, composed from the same rules: the staging block carries every stage's records for 320
    streams at once.  The meter and the true-peak stage tap the transform's PCM in front of all of it"""
    assert mix_items(N1, False) > MIX_MAX_BLOCKS * MIX_THREADS and N1 > RESAMPLE_MAX_BLOCKS and N1 > TRUEPEAK_MAX_BLOCKS
    mix, (L, M, table) = mix_kit.hostile_matrix(2, 2), RESAMPLERS["1-3"]()
    mixed = [mix_kit.mix_rule(x, mix) for x in kit.plain()]
    ceiling = ceiling_of(mixed)
    n1 = lambda c: resample_kit.n_out(0, 1024 * first_count(c), L, M)
    w = windows(3, n1)
    want = trimmed([resample_kit.resample_rule(x, L, M, table) for x in limited(mixed, ceiling)], w)
    meter = metered()
    got = kit.run(S, way, False, gains=by_slot(GAINS), windows=by_slot(w), mix=mix, limiter=(ceiling, RELEASE), resample=(L, M, table), trim=True,
                  loudness=METER, true_peak=meter["stage"])
    clean(got)
    every_slot(got["out"], want, "the chain, %s" % way)
    every_slot(got["records"], meter["records"], "the chain's meter records")
    every_slot(got["peaks"], meter["peaks"], "the chain's true-peak records", same=truepeak_kit.same_records)
