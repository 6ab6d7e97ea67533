"""What tests/test_pcm_product_batch_gpu.py shares: the product-sized batch, the pipeline that runs it, the test's own account of every
stage's counts, and the comparison of 320 slots with the expected output of their twelve classes.  A plain module like resident_kit.py;
torch is imported where a GPU is used.

The batch: the committed stream stereo48 (18 frames) in S = 320 slots.  Slot s starts at frame s % 3 and brings 16 - s % 4 frames in the
first batch — twelve classes of (start, count), s % 12 names the class, 4640 frames in all at max_frames 16 — and what it has left, at most
2 frames, in the second, from which the slots with nothing left are absent.  Both are submitted before the first is collected (two lanes).
Whatever else differs between slots (a gain, a window, a dropped frame) is a function of the slot that repeats with the classes, so that
twelve evaluations of a rule give every slot's expected output."""
import numpy as np

import aacgpu
import features_kit
import resample_kit
import trim_kit
from resident_kit import CASES, close_to, load, packed

S, MAX_FRAMES, CLASSES, FRAMES, CHANNELS, SAMPLE_INDEX = 320, 16, 12, 18, 2, 3
I16_POISON = 0x7F7F
_stream = []


def stream():
    """(bytes, frame table, the oracle's PCM) of stereo48"""
    if not _stream:
        case = {c["name"]: c for c in CASES}["stereo48"]
        assert case["frames"] == FRAMES and case["channels"] == CHANNELS and case["sampleIndex"] == SAMPLE_INDEX
        _stream.append(load(case))
    return _stream[0]


def start(s):
    return s % 3


def first_count(s):
    return 16 - s % 4


def second_count(s):
    return min(2, FRAMES - start(s) - first_count(s))


def script(n_slots):
    """the two batches of the slots 0 .. n_slots - 1: [(live slots, counts, first frames)]"""
    slots = list(range(n_slots))
    live = [s for s in slots if second_count(s)]
    return [(slots, [first_count(s) for s in slots], [start(s) for s in slots]),
            (live, [second_count(s) for s in live], [start(s) + first_count(s) for s in live])]


def first_batch_frames(n_slots=S):
    return sum(first_count(s) for s in range(n_slots))


assert first_batch_frames() == 4640 and len({(start(s), first_count(s)) for s in range(S)}) == CLASSES
assert all((start(s), first_count(s)) == (start(s % CLASSES), first_count(s % CLASSES)) for s in range(S))
assert len(script(S)[1][0]) < S and max(script(S)[1][1]) == 2 and min(script(S)[1][1]) == 1, "the second batch is ragged, with gaps in the slot list"


class Counts:
    """the test's own account of what each slot's stages count, from the kits' formulas: the resampler's clock, the trim's window and
    position, the feature stage's clock and the meter's"""

    def __init__(self, n_slots, resample, windows, features, hop):
        self.rs, self.windows, self.ft, self.hop = resample, windows, features, hop
        self.clock, self.Q, self.N, self.received = [0] * n_slots, [0] * n_slots, [0] * n_slots, [0] * n_slots

    def batch(self, s, frames):
        """-> (what leaves for the slot's `frames` frames: samples, or feature frames; the meter's records), and the counts move on"""
        n = 1024 * frames
        n_rec = (self.received[s] + n) // self.hop - self.received[s] // self.hop if self.hop else 0
        self.received[s] += n
        if self.rs:
            n, self.clock[s] = resample_kit.n_out(self.clock[s], self.clock[s] + n, self.rs[0], self.rs[1]), self.clock[s] + n
        if self.windows is not None:
            n, self.Q[s] = trim_kit.span(self.Q[s], self.windows[s][0], self.windows[s][1], n)[1], self.Q[s] + n
        if self.ft:
            K, H, P = self.ft["frame_length"], self.ft["hop"], self.ft["pad_left"]
            n, self.N[s] = features_kit.count(self.N[s] + n, K, H, P) - features_kit.count(self.N[s], K, H, P), self.N[s] + n
        return n, n_rec


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


def run(n_slots, way="pageable", i16=False, gains=None, windows=None, tables=None, **kw):
    """the two batches of the slots 0 .. n_slots - 1 on a pipeline with device plans and two lanes, the second submitted while the first
    is in flight, what leaves delivered `way` (pageable, packed or planar) into a poisoned destination larger than the batch needs.
    gains: {slot: G} and windows: {slot: (skip, keep)}, set before the first batch; tables: a frame table per slot in the place of the
    stream's own (a dropped frame); kw: the pipeline's stages.
    -> dict(out: per slot (rows, width) of what left, status, flags, refusals, concealed, lengths: per batch {slot: count}, records and
    peaks: per slot per batch or None, launches)"""
    data, table, _ = stream()
    tables = tables if tables is not None else [table] * n_slots
    if i16:
        kw["output_kind"] = aacgpu.OUTPUT_I16
    p = aacgpu.Pipeline(channels=CHANNELS, max_streams=n_slots, max_frames=MAX_FRAMES, sample_index=SAMPLE_INDEX, device_plans=True, lanes=2, **kw)
    ft = p.features
    width, dtype, unit = (ft["n_mels"], np.float32, 1) if ft else (p.channels, np.int16 if i16 else np.float32, 1024)
    ragged = bool(p.trim or p.resample or ft)
    for s, g in (gains or {}).items():
        p.set_gain(s, g)
    if p.trim:
        windows = {s: (windows or {}).get(s, p.trim) for s in range(n_slots)}
        for s, w in windows.items():
            p.set_trim(s, *w)
            assert p.stream_trim(s) == tuple(w) + (0,)
    model = Counts(n_slots, p.resample, windows if p.trim else None, ft, p.loudness["hop"] if p.loudness else 0)
    out = dict(out=[[] for _ in range(n_slots)], status=[[] for _ in range(n_slots)], flags=[[] for _ in range(n_slots)], refusals=0, lengths=[],
               records=[[] for _ in range(n_slots)] if p.loudness else None, peaks=[[] for _ in range(n_slots)] if p.true_peak else None)
    pending = []
    for b, (live, counts, at) in enumerate(script(n_slots)):
        fr = packed([tables[s] for s in live], [0] * len(live), at, counts)
        slots, cnt = np.array(live, np.uint32), np.array(counts, np.uint32)
        n_out, n_rec = [list(v) for v in zip(*[model.batch(s, c) for s, c in zip(live, counts)])]
        assert p.out_samples(slots, cnt).tolist() == n_out, "aacg_pipeline_out_samples against the formula, batch %d" % b
        if p.loudness:
            assert p.loudness_counts(slots, cnt).tolist() == n_rec, "aacg_pipeline_loudness_counts against the formula, batch %d" % b
        out["lengths"].append(dict(zip(live, n_out)))
        total = sum(n_out)
        if way == "pageable":
            buf = poison_host(np.empty((total + 64) * width, dtype))
            t = p.submit(data, fr, slots, cnt, pcm=buf)
        else:
            planar = way == "planar"
            stride = max((max(n_out) + unit - 1) // unit, 1) if ragged else MAX_FRAMES
            buf = poisoned_device((len(live) + 1, width, stride * unit) if planar else ((total + 64) * width,), dtype == np.int16)
            t = p.submit_device(data, fr, slots, cnt, buf, planar=planar, stride_frames=stride if planar else None)
        pending.append((t, live, counts, n_out, n_rec, buf))
    for t, live, counts, n_out, n_rec, buf in pending:
        recs = p.take_loudness(t) if p.loudness else None
        peaks = p.take_true_peak(t) if p.true_peak else None
        back, res, refused, *lengths = p.collect(t)
        assert back is buf and (not ragged or lengths[0].tolist() == n_out)
        total, first = sum(n_out), np.concatenate([[0], np.cumsum(counts)])
        if way == "pageable":
            assert is_poison(buf[total * width:]), "the elements behind the batch were written"
            parts = np.split(buf[:total * width].copy(), np.cumsum(n_out)[:-1] * width)
        else:
            dev = buf.cpu().numpy()
            if way == "planar":
                assert is_poison(dev[len(live)]), "the row behind the last stream was written"
                parts = []
                for k in range(len(live)):
                    parts.append(np.ascontiguousarray(dev[k, :, :n_out[k]].T).reshape(-1))
                    padding = dev[k, :, n_out[k]:]
                    if ft and ft["log"]:
                        want = np.full_like(padding, np.float32(np.log10(np.float64(np.float32(ft["floor"])))))
                        assert (features_kit.ulps(padding, want) <= 4).all() and (padding.size == 0 or (padding == padding.flat[0]).all()), "the padding is not log10f(floor)"
                    else:
                        assert not padding.view(np.uint16 if dtype == np.int16 else np.uint32).any(), "the padding behind slot %d's samples is not exactly zero" % live[k]
            else:
                assert is_poison(dev[total * width:]), "the elements behind the batch were written"
                parts = np.split(dev[:total * width], np.cumsum(n_out)[:-1] * width)
        out["refusals"] += refused
        for k, s in enumerate(live):
            out["out"][s].append(parts[k].reshape(-1, width))
            out["status"][s].append(res["status"][first[k]:first[k + 1]].copy())
            out["flags"][s].append(res["flags"][first[k]:first[k + 1]].copy())
            if p.loudness:
                assert recs[k].shape == (n_rec[k], CHANNELS, 2)
                out["records"][s].append(recs[k])
            if p.true_peak:
                assert peaks[k].shape == (n_rec[k], CHANNELS)
                out["peaks"][s].append(peaks[k])
    out["concealed"] = p.concealed() if p.conceal else 0
    out["launches"] = p.launch_counts()
    p.close()
    for key in ("out", "status", "flags", "records", "peaks"):
        if out[key] is not None:
            out[key] = [np.concatenate(x) for x in out[key]]
    return out


_plain = {}


def plain(i16=False):
    """the yardstick's input, once per element type: the twelve classes' PCM, (samples, 2) each, from a pipeline of twelve slots without
    any stage — the shape the existing tests use — fed the same two batches; the tests leave it unchanged.  The float PCM is held to the
    committed oracle PCM by the project's tolerances (a class that starts behind frame 0 from its second frame on: its first frame overlaps
    nothing)"""
    if i16 not in _plain:
        got = run(CLASSES, i16=i16)
        assert got["refusals"] == 0 and not any(x.any() for x in got["status"])
        pcm = got["out"]
        for c, x in enumerate(pcm):
            assert len(x) == 1024 * (first_count(c) + second_count(c))
        if not i16:
            ref = stream()[2].reshape(FRAMES, 1024, CHANNELS)
            skip = [1 if start(c) else 0 for c in range(CLASSES)]
            close_to(np.concatenate([x[1024 * k:] for x, k in zip(pcm, skip)]),
                     np.concatenate([ref[start(c) + k:start(c) + len(x) // 1024].reshape(-1, CHANNELS) for c, (x, k) in enumerate(zip(pcm, skip))]))
        _plain[i16] = pcm
    return _plain[i16]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint16 if a.dtype.itemsize == 2 else np.uint32)


def every_slot(got, want, what, same=None):
    """got: per slot what left; want: per class what must have — bit for bit (or by `same(x, y, what)`), every one of the slots"""
    assert len(got) == S and len(want) == CLASSES
    for s, x in enumerate(got):
        y = np.ascontiguousarray(want[s % CLASSES])
        assert x.shape == y.shape and x.dtype == y.dtype, "%s: slot %d delivered %s %s, its class expects %s %s" % (what, s, x.shape, x.dtype, y.shape, y.dtype)
        if same is not None:
            same(x, y, "%s, slot %d" % (what, s))
            continue
        wrong = np.argwhere(bits(x) != bits(y))
        assert wrong.size == 0, "%s: slot %d (class %d) differs from its class's expected output at %d of %d values, first at %s: %r against %r" % (
            what, s, s % CLASSES, len(wrong), y.size, wrong[0], x[tuple(wrong[0])], y[tuple(wrong[0])])
