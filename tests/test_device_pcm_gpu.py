"""PCM left on the device on the resident route (aacg_pipeline_submit_device / aacg_pipeline_wait_device, aacgpu.Pipeline.submit_device,
wait_device, decode_tensor), on a real MI355X: the same batches as the host call's, the PCM into a torch tensor — packed, where the
transform writes the caller's memory, or planar, (stream, channel, stride_frames * 1024) with the padding written by aacg_pcm_planar.

The yardstick is the host route (resident_kit.run_script: aacg_pipeline_decode_ragged into host memory) on the same script with the
same options.  Every comparison is bit for bit — the PCM is the same kernels' output — and every tensor is poisoned first and is
larger than the batch needs, so that an element nobody wrote and an element written outside the batch's block both show."""
import numpy as np
import pytest

import aacgpu
from resident_kit import CASES, ERR_CAPACITY, ERR_INVALID_ARG, NODE, OPTIONS, load, members_of, packed, ragged_script, run_script
from resident_kit import same_bits, steady
from resident_kit import shape_streams, stage_streams          # noqa: F401  (fixtures: tests/js/shape_cases.js, stage_cases.js)

pytestmark = pytest.mark.gpu
CASE = {c["name"]: c for c in CASES}
I16_POISON = 0x7F7F


def poisoned(shape, i16):
    import torch
    t = torch.full(shape, I16_POISON, dtype=torch.int16, device="cuda") if i16 else torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()                                  # the fill is torch's stream's, the batch a lane's
    return t


def is_poison(a):
    return bool((a == I16_POISON).all()) if a.dtype == np.int16 else bool(np.isnan(a).all())


def no_poison(a):
    return not (a == I16_POISON).any() if a.dtype == np.int16 else bool(np.isfinite(a).all())


def unpack(pcm, live, counts, C_, planar, max_frames, got, pads):
    """one collected batch (a numpy copy of its tensor, poison rows included) -> per-stream interleaved PCM appended to got; checks
    the poison behind the batch's block, and for planar collects the padding"""
    first = np.concatenate([[0], np.cumsum(counts)])
    per = 1024 * C_
    if planar:
        assert pcm.shape == (len(live) + 1, C_, max_frames * 1024)
        assert is_poison(pcm[len(live)]), "the row behind the last stream was written"
        for k, s in enumerate(live):
            n = counts[k] * 1024
            got[s].append(np.ascontiguousarray(pcm[k, :, :n].T).reshape(-1))      # [sample][channel], as the host call's
            pads.append(pcm[k, :, n:])
    else:
        n = int(first[-1])
        assert pcm.shape == ((n + 1) * per,)
        assert is_poison(pcm[n * per:]), "the frame behind the batch was written"
        for k, s in enumerate(live):
            got[s].append(pcm[first[k] * per:first[k + 1] * per])


def device_run(members, script, C_, si, max_frames, device_plans, planar, i16=False, **kw):
    """run_script with the PCM left on the device -> (per-stream PCM, per-stream statuses, refusals in all, plan builds, launch counts)"""
    S = len(members)
    data = np.concatenate([m[0] for m in members])
    bases = np.cumsum([0] + [len(m[0]) for m in members])[:-1]
    tables = [m[1] for m in members]
    if i16:
        kw["output_kind"] = aacgpu.OUTPUT_I16
    p = aacgpu.Pipeline(channels=C_, max_streams=S, max_frames=max_frames, sample_index=si, device_plans=device_plans, **kw)
    got, status, refusals, pads = [[] for _ in range(S)], [[] for _ in range(S)], 0, []
    for live, counts, at in script:
        fr = packed([tables[s] for s in live], [bases[s] for s in live], at, counts)
        n = int(sum(counts))
        out = poisoned((len(live) + 1, C_, max_frames * 1024) if planar else ((n + 1) * 1024 * C_,), i16)
        t = p.submit_device(data, fr, np.array(live, np.uint32), np.array(counts, np.uint32), out, planar=planar, stride_frames=max_frames if planar else None)
        back, res, refused = p.collect(t)
        assert back is out
        refusals += refused
        unpack(out.cpu().numpy(), live, counts, C_, planar, max_frames, got, pads)
        first = np.concatenate([[0], np.cumsum(counts)])
        for k, s in enumerate(live):
            status[s].append(res["status"][first[k]:first[k + 1]].copy())
    for pad in pads:
        assert pad.size == 0 or not pad.view(np.uint16 if i16 else np.uint32).any(), "the padding behind a stream's samples is not exactly zero"
    builds, counts_ = p.plan_builds(), p.launch_counts()
    p.close()
    return [np.concatenate(g) for g in got], [np.concatenate(x) for x in status], refusals, builds, counts_


def committed(name, copies):
    c = CASE[name]
    data, table, _ = load(c)
    return [(data, table[:12])] * copies, c["channels"], c["sampleIndex"]


def same_run(a, b, what):
    for s, (x, y) in enumerate(zip(a[0], b[0])):
        assert same_bits(x, y), "%s: stream %d's PCM differs from the host route's" % (what, s)
    for x, y in zip(a[1], b[1]):
        assert np.array_equal(x, y), what
    assert a[2] == b[2], what


@pytest.mark.parametrize("planar", [False, True], ids=["packed", "planar"])
@pytest.mark.parametrize("name,copies", [("stereo48", 3), ("surround48", 2), ("mono22", 2)])
def test_device_pcm_equals_the_host_route(name, copies, planar):
    """tests 1 and 2: seeded ragged batches of at most 4 frames over the streams' first 12, both plan modes, f32 and int16; packed:
    the batch's frames equal the host route's and the frame behind them is still poison; planar (stride_frames = max_frames):
    tensor[s, c, :len] is the host PCM's channel c, the padding is exactly zero and a row of poison behind the last stream is untouched"""
    mem, C_, si = committed(name, copies)
    script = ragged_script([m[1] for m in mem], 4, np.random.default_rng(11))
    assert len(script) >= 2
    for i16 in (False, True):
        kw = dict(output_kind=aacgpu.OUTPUT_I16) if i16 else {}
        for mode in (False, True):
            want = run_script(mem, script, C_, si, 4, mode, **kw)
            got = device_run(mem, script, C_, si, 4, mode, planar, i16=i16)
            same_run(got, want, "%s, %s, plan mode %d" % (name, "int16" if i16 else "f32", mode))
            assert got[2] == 0 and got[4]["launches"] == want[4]["launches"] and got[4]["shaped"] == want[4]["shaped"]
            assert np.abs(got[0][0].astype(np.float64)).max() > (100 if i16 else 1e-3), "the streams are music"


@pytest.mark.parametrize("planar", [False, True], ids=["packed", "planar"])
def test_silence_and_refusals(planar):
    """test 3: three 5.1 streams — one clean, one whose first frame is malformed (no layout is learnt from it: every frame of the
    stream in that batch is refused with AACG_PARSE_LAYOUT and nothing of them is decoded), one with a malformed frame behind a learnt
    layout (a silent unit: the stream's state moves on through it, so its PCM is the predecessor's tail, as on the host route).
    Statuses and the refusal count equal the host route's, the PCM too; the unlearnt stream's frames are zeros in both layouts, and
    no poison survives inside the batch's block"""
    c = CASE["surround48"]
    data, table, _ = load(c)

    def broken(at):
        bad = data.copy()                                      # the test's own copy
        off, length = int(table[at]["byte_offset"]), int(table[at]["byte_length"])
        bad[off + 7: off + length] = 0xFF                      # a raw_data_block with none of the stream's elements in it
        return bad

    mem = [(data, table), (broken(0), table), (broken(2), table)]
    script = [([0, 1, 2], [2, 1, 3], [0, 0, 0]), ([0, 1, 2], [3, 4, 2], [2, 1, 3])]
    for mode in (False, True):
        want = run_script(mem, script, 6, c["sampleIndex"], 4, mode)
        assert want[2] >= 2 and want[1][1][0] != 0 and not want[1][1][1:].any() and want[1][2][2] != 0 and not want[1][0].any(), want[1]
        got = device_run(mem, script, 6, c["sampleIndex"], 4, mode, planar)
        same_run(got, want, "plan mode %d" % mode)
        assert not got[0][1][:6 * 1024].any(), "the unlearnt stream's frame is not silent"
        assert got[0][1][6 * 1024:].any() and got[0][2].any()
        assert all(no_poison(x) for x in got[0]), "poison survived inside the batch's block"


def test_batches_in_flight_and_the_consumers_stream():
    """test 4: five lanes, eight batches of 4 stereo streams x 2 frames submitted ahead, each into its own tensor; behind
    wait_device(ticket, side stream) a clone of the tensor is enqueued on that torch stream with no host synchronisation in between,
    and only then is anything collected.  The clones are the host route's batches, and as many launches continued their predecessor"""
    import torch
    data, table, _ = load(CASE["stereo48"])
    S, B, period = 4, 8, 16
    for planar in (False, True):
        want_counts, want = steady(data, table, S, B, period, False)
        p = aacgpu.Pipeline(channels=2, max_streams=S, max_frames=2, lanes=5)
        side = torch.cuda.Stream()
        outs = [poisoned((S, 2, 2048) if planar else (S * 2 * 2048,), False) for _ in range(B)]
        tickets, clones = [], []
        for b in range(B):
            fr = packed([table] * S, [0] * S, [(2 * b) % period] * S, [2] * S)
            tickets.append(p.submit_device(data, fr, np.arange(S), 2, outs[b], planar=planar))
            p.wait_device(tickets[-1], side)
            with torch.cuda.stream(side):
                clones.append(outs[b].clone())
        for t in tickets:
            out, res, refused = p.collect(t)
            assert refused == 0 and not res["status"].any()
        with pytest.raises(aacgpu.AacgError) as e:
            p.wait_device(B + 1)                               # never given out
        assert e.value.code == ERR_INVALID_ARG
        p.wait_device(tickets[0])                              # collected: nothing to wait for
        side.synchronize()
        counts = p.launch_counts()
        p.close()
        assert counts["launches"] == B and counts["chained"] == want_counts["chained"] and counts["chained"] > 0
        for b in range(B):
            got = clones[b].cpu().numpy()
            if planar:
                got = np.ascontiguousarray(got.transpose(0, 2, 1)).reshape(-1)
            assert same_bits(got, want[b]), "batch %d's clone on the consumer's stream is not the host route's PCM" % b


@pytest.mark.skipif(NODE is None, reason="node not present")
def test_with_the_other_resident_features(stage_streams, shape_streams):
    """test 5: the spec-correct TNS / noise stages (f32) and the carried window shape (int16), one planar and one packed run each,
    against the host route with the same options"""
    for streams, kw, i16 in ((stage_streams, dict(tns_spec=True, pns_spec=True, parse_options=OPTIONS), False), (shape_streams, dict(carry_window_shape=True), True)):
        mem = members_of(streams, ["stereo48", "split48"], 2)
        script = ragged_script([m[1] for m in mem], 4, np.random.default_rng(5))
        host_kw = dict(kw, output_kind=aacgpu.OUTPUT_I16) if i16 else kw
        want = run_script(mem, script, 2, 3, 4, False, **host_kw)
        for planar in (True, False):
            same_run(device_run(mem, script, 2, 3, 4, False, planar, i16=i16, **kw), want, "%s, %s" % (sorted(kw), "planar" if planar else "packed"))


def test_decode_tensor():
    """test 6: shapes, lengths, device, dtype and values of one stereo and one 5.1 batch, planar and packed"""
    import torch
    for name, counts in (("stereo48", [3, 1, 2]), ("surround48", [2, 4])):
        c = CASE[name]
        data, table, _ = load(c)
        S, C_ = len(counts), c["channels"]
        fr = packed([table] * S, [0] * S, [0] * S, counts)
        host = aacgpu.Pipeline(channels=C_, max_streams=S, max_frames=4, sample_index=c["sampleIndex"])
        want, want_res, _ = host.decode(data, fr, np.arange(S), np.array(counts, np.uint32))
        host.close()
        first = np.concatenate([[0], np.cumsum(counts)]) * 1024 * C_
        for i16 in (False, True):
            if i16:
                host = aacgpu.Pipeline(channels=C_, max_streams=S, max_frames=4, sample_index=c["sampleIndex"], output_kind=aacgpu.OUTPUT_I16)
                want = host.decode(data, fr, np.arange(S), np.array(counts, np.uint32))[0]
                host.close()
            for planar in (True, False):
                p = aacgpu.Pipeline(channels=C_, max_streams=S, max_frames=4, sample_index=c["sampleIndex"], output_kind=aacgpu.OUTPUT_I16 if i16 else aacgpu.OUTPUT_F32)
                t, lengths, res, refused = p.decode_tensor(data, fr, np.arange(S), counts, planar=planar)
                torch.cuda.current_stream().synchronize()      # what decode_tensor put behind the batch
                p.close()
                assert t.is_cuda and t.device.index == 0 and t.dtype == (torch.int16 if i16 else torch.float32) and t.is_contiguous()
                assert list(lengths) == [n * 1024 for n in counts] and refused == 0 and np.array_equal(res["status"], want_res["status"])
                got = t.cpu().numpy()
                if planar:
                    assert tuple(t.shape) == (S, C_, max(counts) * 1024)
                    for s in range(S):
                        n = int(lengths[s])
                        assert same_bits(np.ascontiguousarray(got[s, :, :n].T).reshape(-1), want[first[s]:first[s + 1]]), (name, s)
                        assert not got[s, :, n:].any()
                else:
                    assert tuple(t.shape) == (sum(counts), 1024, C_) and same_bits(got.reshape(-1), want[:first[-1]])


def test_refusals_take_no_ticket_and_leave_the_pipeline_as_it_was():
    """test 7: page-locked host memory as d_pcm, a pointer offset by 4 bytes, stride_frames one below the largest count, d_pcm_bytes one
    byte short (AACG_ERR_CAPACITY), layout 2, PACKED with a stride: each is refused with its code, takes no ticket, and a good batch
    behind them all on the same pipeline is the host route's, bit for bit"""
    data, table, _ = load(CASE["stereo48"])
    S, counts = 3, [2, 4, 3]
    n, per = sum(counts), 2048
    fr = packed([table] * S, [0] * S, [0] * S, counts)
    host = aacgpu.Pipeline(channels=2, max_streams=S, max_frames=4)
    want = host.decode(data, fr, np.arange(S), np.array(counts, np.uint32))[0]
    host.close()
    p = aacgpu.Pipeline(channels=2, max_streams=S, max_frames=4)
    t = poisoned((S * 2 * 4 * 1024 + per,), False)            # room for the planar block of stride 4, and a frame to spare
    addr, packed_bytes, planar_bytes = t.data_ptr(), n * per * 4, S * 2 * 4 * 1024 * 4
    assert planar_bytes <= t.numel() * 4
    pinned = p.pinned(n * per, np.float32)
    pinned[:] = 7.0
    cases = [((pinned.ctypes.data, packed_bytes), dict(), ERR_INVALID_ARG),                      # page-locked host memory
             ((addr + 4, packed_bytes), dict(), ERR_INVALID_ARG),                               # not 16-byte aligned
             ((addr, planar_bytes), dict(planar=True, stride_frames=3), ERR_INVALID_ARG),       # the largest count is 4
             ((addr, packed_bytes - 1), dict(), ERR_CAPACITY),
             ((addr, planar_bytes - 1), dict(planar=True, stride_frames=4), ERR_CAPACITY),
             ((addr, planar_bytes), dict(layout=2, stride_frames=4), ERR_INVALID_ARG),          # no such layout
             ((addr, packed_bytes), dict(stride_frames=4), ERR_INVALID_ARG)]                    # PACKED takes no stride
    for out, kw, code in cases:
        with pytest.raises(aacgpu.AacgError) as e:
            p.submit_device(data, fr, np.arange(S), counts, out, **kw)
        assert e.value.code == code, (kw, out, str(e.value))
        assert "aacg_pipeline_submit_device" in str(e.value)
    import torch
    torch.cuda.synchronize()
    assert is_poison(t.cpu().numpy()) and (pinned == 7.0).all(), "a refused call wrote PCM"
    assert p._keep == {} and p.launch_counts()["launches"] == 0
    ticket = p.submit_device(data, fr, np.arange(S), counts, t)
    assert ticket == 1, "a refused call took a ticket"
    out, res, refused = p.collect(ticket)
    got = t.cpu().numpy()
    p.close()
    assert refused == 0 and same_bits(got[:n * per], want) and is_poison(got[n * per:])


def test_decode_tensor_waits_for_what_torch_has_queued_on_the_block():
    """decode_tensor's tensor comes from torch's allocator on torch's current stream, which hands a freed block out again while that
    stream's work on it is still queued; the lane's stream is ordered behind nothing of torch's.  Here the block's previous life ends
    with a fill of NaN queued behind some milliseconds of other work on the same stream, then the tensor is dropped and decode_tensor
    called at once: the PCM must be the host route's, with no NaN landing in it late"""
    import torch
    c = CASE["stereo48"]
    data, table, _ = load(c)
    S, F = 4, 4
    fr = packed([table] * S, [0] * S, [0] * S, [F] * S)
    host = aacgpu.Pipeline(channels=2, max_streams=S, max_frames=F)
    want = host.decode(data, fr, np.arange(S), F)[0]
    host.close()
    p = aacgpu.Pipeline(channels=2, max_streams=S, max_frames=F)
    for planar in (True, False):
        p.reset_stream(0), p.reset_stream(1), p.reset_stream(2), p.reset_stream(3)
        shape = (S, 2, F * 1024) if planar else (S * F, 1024, 2)
        busy = torch.empty(64 << 20, dtype=torch.float32, device="cuda")
        old = torch.empty(shape, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for _ in range(100):                                   # 100 x 256 MB of fills: milliseconds of work in front of ...
            busy.fill_(1.0)
        old.fill_(float("nan"))                                # ... the last write of the block's previous life
        ptr = old.data_ptr()
        del old
        t, lengths, res, refused = p.decode_tensor(data, fr, np.arange(S), F, planar=planar)
        reused = t.data_ptr() == ptr
        torch.cuda.synchronize()
        got = t.cpu().numpy()
        print("planar %s: the allocator handed the same block out again: %s" % (planar, reused))
        if planar:
            got = np.ascontiguousarray(got.transpose(0, 2, 1))
        assert refused == 0 and same_bits(got.reshape(-1), want), "work queued on the block before decode_tensor landed in the PCM"
    p.close()
