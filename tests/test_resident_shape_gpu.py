"""Each channel's window shape carried on the device on the resident route (aacg_pipeline_config.stages bit 2,
aacgpu.Pipeline(carry_window_shape=True)), on a real MI355X: behind every refresh one launch of aacg_units_carry_shape sets
window_shape_prev of the batch's unit records from the frame before and, across batches, from the engine's per-channel state.

The yardstick is the host-planned path with the same rule applied by the test: Parser.parse_batch -> window_shape_prev per stream and
channel (the stream's first frame of a batch takes what its previous batch left, a refused frame is silent and has shape 0) ->
Engine.plan -> decode_pipelined, bit for bit; the oracle on the same units bounds both with the project's tolerances.

Streams: tests/js/shape_cases.js (plain frames: no TNS, no noise bands, no pulses) and tests/js/stage_cases.js (all three, for the
carried shape together with the spec-correct stages).  The conditions they were chosen for are asserted here from the parser's
records; no frame is left out of any comparison."""
import os
import subprocess

import numpy as np
import pytest

import aacgpu
from resident_kit import ERR_INVALID_ARG, ERR_UNSUPPORTED, EX_RV, GROUPS, NODE, OPTIONS, PLAIN, ROOT, HostRoute, close_to, members_of, packed
from resident_kit import ragged_script, rect_script, same_bits, steady
from resident_kit import oracle, stage_streams          # noqa: F401  (fixtures: the oracle; tests/js/stage_cases.js)
from resident_kit import shape_streams as streams          # noqa: F401  (fixture: tests/js/shape_cases.js)

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not present")]


def host_run(mem, script, C_, si, oracle=None, **kw):
    """the script on the yardstick -> (per-stream PCM, per-stream oracle PCM or None, W after every batch, the route object, closed)"""
    S = len(mem)
    host = HostRoute(S, C_, si, oracle, **kw)
    data = np.concatenate([m[0] for m in mem])
    bases = np.cumsum([0] + [len(m[0]) for m in mem])[:-1]
    want, ref, states = [[] for _ in range(S)], [[] for _ in range(S)], []
    per = 1024 * C_
    for live, counts, at in script:
        fr = packed([mem[s][1] for s in live], [bases[s] for s in live], at, counts)
        pcm, r, _ = host.decode(data, fr, live, counts)
        first = np.concatenate([[0], np.cumsum(counts)])
        for k, s in enumerate(live):
            want[s].append(pcm[first[k] * per:first[k + 1] * per])
            if r is not None:
                ref[s].append(r[first[k] * per:first[k + 1] * per])
        states.append(host.W.copy())
    host.close()
    return [np.concatenate(w) for w in want], [np.concatenate(r) for r in ref] if oracle is not None else None, states, host


def pipe_run(mem, script, C_, si, max_frames, device_plans=False, states=None, lanes=0, ahead=False, **kw):
    """the script on a pipeline -> (per-stream PCM, per-stream statuses, refusals, launch counts).  states: W after every batch, compared
    with stream_window_shape of every slot.  ahead: every batch submitted before the fifth-last is collected (five lanes in flight)."""
    S = len(mem)
    data = np.concatenate([m[0] for m in mem])
    bases = np.cumsum([0] + [len(m[0]) for m in mem])[:-1]
    p = aacgpu.Pipeline(channels=C_, max_streams=S, max_frames=max_frames, sample_index=si, device_plans=device_plans, lanes=lanes, **kw)
    elem = np.int16 if kw.get("output_kind") == aacgpu.OUTPUT_I16 else np.float32
    got, status, refusals = [[] for _ in range(S)], [[] for _ in range(S)], 0
    per = 1024 * C_
    outs, pending = [], []
    for b, (live, counts, at) in enumerate(script):
        fr = packed([mem[s][1] for s in live], [bases[s] for s in live], at, counts)
        if ahead:
            pending.append(p.submit(data, fr, np.array(live, np.uint32), np.array(counts, np.uint32), pcm=p.pinned(int(sum(counts)) * per, elem)))
            if len(pending) == 5:
                outs.append(p.collect(pending.pop(0)))
        else:
            outs.append(p.decode(data, fr, np.array(live, np.uint32), np.array(counts, np.uint32)))
            if states is not None:
                for s in range(S):
                    assert p.stream_window_shape(s) == [int(v) for v in states[b][s]], "batch %d: the state of slot %d" % (b, s)
    outs += [p.collect(t) for t in pending]
    for (live, counts, at), (pcm, res, refused) in zip(script, outs):
        refusals += refused
        first = np.concatenate([[0], np.cumsum(counts)])
        for k, s in enumerate(live):
            got[s].append(pcm[first[k] * per:first[k + 1] * per].copy())
            status[s].append(res["status"][first[k]:first[k + 1]].copy())
    counts_ = p.launch_counts()
    builds = p.plan_builds()
    p.close()
    return [np.concatenate(g) for g in got], [np.concatenate(x) for x in status], refusals, counts_, builds


def kbd_before(host, s):
    """per frame of stream s: did some channel carry KBD into it (the shape_prev the rule gave it)"""
    return np.array([bool(prev.any()) for shape, prev in host.shapes[s]])


def not_carried(frame, other, kbd, what):
    """a frame against the same frame of a pipeline that does not carry the shape: other bits where some channel carries KBD into
    it.  Where none does the windows are the same ones, but not always the bits: a CPE whose channels were given different previous
    shapes leaves the run kernels' packed pair path for this frame, whose tail the next frame adds — the same arithmetic rounded in
    another order, held here to the project's absolute tolerance per sample."""
    if kbd:
        assert not same_bits(frame, other), what + ": KBD carried into it, and yet the samples of a pipeline that always takes sine"
    else:
        assert float(np.abs(frame.astype(np.float64) - other).max()) <= 1e-5, what + ": no KBD carried into it"


@pytest.mark.parametrize("names,C_,si", GROUPS, ids=[g[0] for g in GROUPS])
def test_carried_shapes_equal_the_host_route_bit_for_bit_and_the_oracle(streams, oracle, names, C_, si):
    """stages = 4 alone (REFERENCE modes) on the plain streams, 4 to 8 streams x 4 frames a batch, three batches: the pipeline's PCM
    against the host-planned path with the rule applied by the test (same bits), against the oracle on those units, and NOT the bits
    of a stages = 0 pipeline on any frame that some channel carries KBD into"""
    names = names.split("+")
    copies = 8 // len(names) if C_ == 2 else (4 if C_ == 6 else 6)
    mem = members_of(streams, names, copies)
    S = len(mem)
    assert 4 <= S <= 8
    script = rect_script(S, 4, 12)
    want, ref, states, host = host_run(mem, script, C_, si, oracle)
    assert host.refused == 0 and host.pns_units == 0, "all 12 frames parse, no unit has noise bands"
    assert host.routes <= {"aacg_imdct_run_quant_rv", "aacg_imdct_run_quant_rv_nt"}, "the plain run kernels (the multichannel variant for 5.1)"
    for s in range(S):
        sh = np.array([shape for shape, prev in host.shapes[s]])
        assert sh.shape == (12, C_)
        up, down = (sh[:-1] == 0) & (sh[1:] == 1), (sh[:-1] == 1) & (sh[1:] == 0)
        assert up.any(axis=0).all() and down.any(axis=0).all(), "every channel changes its shape both ways"
        assert sh[3].any() or sh[7].any(), "KBD is carried across a batch boundary"
    got = pipe_run(mem, script, C_, si, 4, states=states, carry_window_shape=True)
    plain = pipe_run(mem, script, C_, si, 4)
    assert got[2] == 0 and plain[2] == 0 and not any(x.any() for x in got[1])
    per = 1024 * C_
    differ = 0
    for s in range(S):
        assert same_bits(got[0][s], want[s]), "stream %d: the device's carried shapes decode to other bits than the rule's" % s
        kbd = kbd_before(host, s)
        a, b = got[0][s].reshape(12, per), plain[0][s].reshape(12, per)
        for f in range(12):
            not_carried(a[f], b[f], kbd[f], "stream %d frame %d" % (s, f))
        differ += int(kbd.sum())
    print("%s: %d of %d frames start from KBD in some channel" % (names, differ, 12 * S))
    assert differ >= 3 * S
    close_to(np.concatenate(got[0]), np.concatenate(ref))


@pytest.mark.parametrize("names,C_,si", GROUPS, ids=[g[0] for g in GROUPS])
def test_with_the_spec_stages(stage_streams, oracle, names, C_, si):
    """stages = 7 on the streams with TNS filters, noise bands and pulses: bit for bit against the SPEC host route with carried shapes,
    every launch aacg_imdct_run_quant_ex_rv, the oracle's tolerances"""
    names = names.split("+")
    copies = 8 // len(names) if C_ == 2 else (4 if C_ == 6 else 6)
    mem = members_of(stage_streams, names, copies)
    S = len(mem)
    script = rect_script(S, 4, 12)
    want, ref, states, host = host_run(mem, script, C_, si, oracle, spec=True, options=OPTIONS)
    assert host.refused == 0 and host.routes == {EX_RV}
    assert aacgpu.debug_route(aacgpu.INPUT_QUANT_I16, aacgpu.OUTPUT_F32, aacgpu.ROUTE_PLAN_STAGES, True) == EX_RV      # the pipeline's plans: one route
    for s in range(S):
        sh = np.array([shape for shape, prev in host.shapes[s]])
        with_kbd_before = int(sh[:-1].sum())                  # channel-frames whose predecessor is KBD
        assert 3 * with_kbd_before >= sh[1:].size and sh[3].any(), (names, s, with_kbd_before)
    got = pipe_run(mem, script, C_, si, 4, states=states, carry_window_shape=True, tns_spec=True, pns_spec=True, parse_options=OPTIONS)
    assert got[2] == 0 and not any(x.any() for x in got[1])
    for s in range(S):
        assert same_bits(got[0][s], want[s]), s
    close_to(np.concatenate(got[0]), np.concatenate(ref))
    # ... and other bits than the same stages without the carried shape, wherever KBD is carried
    spec = pipe_run(mem, script, C_, si, 4, tns_spec=True, pns_spec=True, parse_options=OPTIONS)
    per = 1024 * C_
    for s in range(S):
        kbd = kbd_before(host, s)
        a, b = got[0][s].reshape(12, per), spec[0][s].reshape(12, per)
        for f in range(12):
            not_carried(a[f], b[f], kbd[f], "stream %d frame %d" % (s, f))


def test_plan_modes_ragged_counts_and_five_lanes_in_flight(streams):
    """both plan modes give the same bits; ragged scripts give the bits of the rectangular feed; five lanes in flight (submit / collect,
    a batch per lane) give the bits of one batch at a time; int16 PCM is the f32 result rounded"""
    rng = np.random.default_rng(41)
    mem = members_of(streams, ["stereo48", "split48"], 3)
    S = len(mem)
    rect = pipe_run(mem, rect_script(S, 4, 12), 2, 3, 4, carry_window_shape=True)
    script = ragged_script([m[1] for m in mem], 4, rng)
    assert len(script) > 3 and any(1 in counts for live, counts, at in script)
    kept = pipe_run(mem, script, 2, 3, 4, False, carry_window_shape=True)
    shaped = pipe_run(mem, script, 2, 3, 4, True, carry_window_shape=True)
    flight = pipe_run(mem, script, 2, 3, 4, True, lanes=5, ahead=True, carry_window_shape=True)
    flight0 = pipe_run(mem, script, 2, 3, 4, False, lanes=5, ahead=True, carry_window_shape=True)
    clear = pipe_run(mem, script, 2, 3, 4, False)
    assert kept[2] == shaped[2] == flight[2] == flight0[2] == rect[2] == clear[2] == 0
    assert shaped[4] == 0 and shaped[3]["shaped"] == shaped[3]["launches"] == len(script) and kept[4] > 0 and kept[3]["shaped"] == 0
    assert kept[3]["launches"] == clear[3]["launches"] == len(script) and kept[4] == clear[4], "the launches and plan builds of the bit clear"
    for s in range(S):
        assert same_bits(kept[0][s], rect[0][s]) and same_bits(shaped[0][s], rect[0][s]), s
        assert same_bits(flight[0][s], rect[0][s]) and same_bits(flight0[0][s], rect[0][s]), s
        assert not same_bits(clear[0][s], rect[0][s]) and np.abs(rect[0][s]).max() > 1e-3
    # int16 PCM with stages = 4: the f32 samples rounded to nearest, saturated (tests/test_gpu_parity.py: _pcm16), at most a step off
    # and only at a rounding boundary; bits 0 and 1 with int16 PCM stay unsupported
    for mode in (False, True):
        i16 = pipe_run(mem, script, 2, 3, 4, mode, carry_window_shape=True, output_kind=aacgpu.OUTPUT_I16)
        i16_clear = pipe_run(mem, script, 2, 3, 4, mode, output_kind=aacgpu.OUTPUT_I16)
        assert i16[2] == i16_clear[2] == 0
        assert not all(same_bits(i16_clear[0][s], i16[0][s]) for s in range(S)), "int16 PCM with the carried shape is not the PCM without it"
        for s in range(S):
            assert i16[0][s].dtype == np.int16
            want = np.clip(np.rint(rect[0][s].astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)
            d = i16[0][s].astype(np.int32) - want
            assert np.abs(d).max() <= 1 and np.count_nonzero(d) <= 1e-2 * d.size and np.abs(want).max() > 1000, (np.abs(d).max(), np.count_nonzero(d))
    for kw in (dict(tns_spec=True), dict(pns_spec=True), dict(tns_spec=True, pns_spec=True)):
        with pytest.raises(aacgpu.AacgError) as e:
            aacgpu.Pipeline(channels=2, max_streams=2, max_frames=4, output_kind=aacgpu.OUTPUT_I16, carry_window_shape=True, **kw)
        assert e.value.code == ERR_UNSUPPORTED


def test_the_steady_feed_still_continues_its_predecessor(streams):
    """consecutive batches of one shape still meet in the cross-launch cells with the carry launch between refresh and transform: as
    many launches, and as many of them continued, as with the bit clear; the bits of one batch at a time"""
    c, data, table = streams["stereo48"]
    for mode in (False, True):
        on, pcm = steady(data, table, 6, 24, 12, mode, carry_window_shape=True)
        off, _ = steady(data, table, 6, 24, 12, mode)
        print("device plans %s: %s with the carried shape, %s without" % (mode, on, off))
        assert on["launches"] == off["launches"] == 24 and on["chained"] == off["chained"] > 0 and on["shaped"] == off["shaped"]
    one = aacgpu.Pipeline(channels=2, max_streams=6, max_frames=2, lanes=1, carry_window_shape=True)
    for b in range(24):
        fr = packed([table] * 6, [0] * 6, [(2 * b) % 12] * 6, [2] * 6)
        want, res, refused = one.decode(data, fr, np.arange(6), np.full(6, 2, np.uint32))
        assert refused == 0 and same_bits(want, pcm[b]), b
    one.close()


@pytest.mark.parametrize("mode", [False, True], ids=["kept_plans", "device_plans"])
def test_state_reset_absent_streams_and_a_truncated_frame(streams, oracle, mode):
    """stream_window_shape after every batch is the last frame's shapes; a stream absent from a batch keeps its state; after
    reset_stream the state is 0 and the next frame decodes as a first frame; a truncated frame in the middle of a batch is silent and
    counted once, the frame behind it starts from sine — all against the yardstick with the same rule, bit for bit"""
    c, data, table = streams["stereo48"]
    c2, data2, table2 = streams["split48"]
    bad = data.copy()
    off, length = int(table[6]["byte_offset"]), int(table[6]["byte_length"])
    bad[off + 7: off + length] = 0xFF                           # frame 6: a raw_data_block with no CPE in it
    mem = [(data, table), (bad, table), (data2, table2), (data, table)]
    # batch 1: everybody; batch 2: without slot 2 (and slot 1's frame 6 is the bad one, in the middle); batch 3: everybody, slot 2 continues
    # from frame 4, slot 3 — reset in front of the batch — starts again from frame 8
    script = [([0, 1, 2, 3], [4, 4, 4, 4], [0, 0, 0, 0]), ([3, 1, 0], [4, 4, 4], [4, 4, 4]), ([0, 1, 2, 3], [4, 4, 4, 2], [8, 8, 4, 8])]
    S, per = 4, 2048
    all_data = np.concatenate([m[0] for m in mem])
    bases = np.cumsum([0] + [len(m[0]) for m in mem])[:-1]
    host = HostRoute(S, 2, 3, oracle)
    p = aacgpu.Pipeline(channels=2, max_streams=S, max_frames=4, device_plans=mode, carry_window_shape=True)
    refusals, got, want, ref = 0, [], [], []
    for b, (live, counts, at) in enumerate(script):
        if b == 2:
            before = p.stream_window_shape(3)
            p.reset_stream(3)
            host.reset(3)
            assert p.stream_window_shape(3) == [0, 0] and p.stream_window_shape(0) == [int(v) for v in host.W[0]]
            assert any(before), "slot 3 carried KBD into the reset"
        fr = packed([mem[s][1] for s in live], [bases[s] for s in live], at, counts)
        pcm, res, refused = p.decode(all_data, fr, np.array(live, np.uint32), np.array(counts, np.uint32))
        w, r, _ = host.decode(all_data, fr, live, counts)
        refusals += refused
        if b == 1:
            assert refused == 1 and np.count_nonzero(res["status"]) == 1 and res["status"][4 + 2] != 0, "the truncated frame, counted once"
            assert p.stream_window_shape(2) == [int(v) for v in state_after_first[2]], "a stream absent from the batch keeps its state"
        else:
            assert refused == 0 and not res["status"].any()
        for s in range(S):
            assert p.stream_window_shape(s) == [int(v) for v in host.W[s]], (b, s)
        if b == 0:
            state_after_first = host.W.copy()
        got.append(pcm.copy()); want.append(w); ref.append(r)
    p.close()
    assert refusals == host.refused == 1
    # slot 0 decodes the same stream whole: there frame 6 is KBD in some channel and frame 7 starts from it
    assert host.shapes[0][6][0].any() and host.shapes[0][7][1].any()
    assert not host.shapes[1][6][0].any() and not host.shapes[1][7][1].any(), "the bad frame is silent (shape 0), and the frame after it starts from sine"
    assert not host.shapes[3][8][1].any() and state_after_first.any() and host.shapes[2][4][1].any(), "the reset slot starts from sine; the absent slot continues from KBD"
    for b in range(3):
        assert same_bits(got[b], want[b]), "batch %d" % b
    close_to(np.concatenate(got), np.concatenate(ref))
    host.close()


def test_a_stream_unlearnt_in_its_first_batch(streams):
    """channels > 2: a stream whose first frame does not parse has no layout in its first batch — every frame of it is refused, its
    state stays 0 — and decodes from the next batch on as from a first frame, next to a stream that carries its shapes all along.
    Only the zero case can be reached through the pipeline: a slot's layout is forgotten by aacg_pipeline_reset_stream alone, which
    also clears its state, so an unlearnt slot never holds a carried KBD that a stray write could be seen to destroy.  That a channel
    without a unit keeps a NON-zero state is pinned on the kernel itself (tests/test_shape_carry_emu.py: absent streams, channels beyond
    a narrower stream) and here by the stream absent from a batch (test_state_reset_absent_streams_and_a_truncated_frame)."""
    c, data, table = streams["five1_48"]
    bad = data.copy()
    off, length = int(table[0]["byte_offset"]), int(table[0]["byte_length"])
    bad[off + 7: off + length] = 0xFF
    both = np.concatenate([data, bad])
    p = aacgpu.Pipeline(channels=6, max_streams=2, max_frames=4, carry_window_shape=True)
    q = aacgpu.Pipeline(channels=6, max_streams=2, max_frames=4, carry_window_shape=True)
    fr = packed([table, table], [0, len(data)], [0, 0], [4, 4])
    pcm, res, refused = p.decode(both, fr, np.array([0, 1], np.uint32), 4)
    assert refused == 4 and (res["status"][4:] != 0).all() and not res["status"][:4].any() and not pcm[4 * 6144:].any()
    assert p.stream_window_shape(1) == [0] * 6 and any(p.stream_window_shape(0))
    fr = packed([table, table], [0, len(data)], [4, 4], [4, 4])
    pcm, res, refused = p.decode(both, fr, np.array([0, 1], np.uint32), 4)
    assert refused == 0 and p.stream_window_shape(1) == p.stream_window_shape(0)
    # the yardstick for slot 1: a pipeline that sees frames 4..7 as the stream's first ones
    alone, res, refused = q.decode(data, packed([table], [0], [4], [4]), np.array([1], np.uint32), 4)
    assert refused == 0 and same_bits(pcm[4 * 6144:], alone)
    p.close()
    q.close()


def test_get_and_set_window_shape_and_the_listings_that_are_refused():
    """aacg_get / aacg_set_window_shape round-trip beside the overlap state, reset_stream clears it; aacg_plan_carry_window_shape refuses
    (on the host, with a reason) a plan that does not list each stream's frames one behind the other with the same elements"""
    import torch
    eng = aacgpu.Engine(aacgpu.INPUT_QUANT_I16, max_streams=3, max_channels=2)
    assert [eng.get_window_shape(s, c) for s in range(3) for c in range(2)] == [0] * 6
    eng.set_window_shape(1, 1, 1)
    eng.set_window_shape(2, 0, 1)
    assert [eng.get_window_shape(s, c) for s in range(3) for c in range(2)] == [0, 0, 0, 1, 1, 0]
    eng.set_window_shape(2, 0, 0)
    eng.reset_stream(1)
    assert [eng.get_window_shape(s, c) for s in range(3) for c in range(2)] == [0] * 6
    for bad in (lambda: eng.set_window_shape(3, 0, 1), lambda: eng.get_window_shape(0, 2), lambda: eng.set_window_shape(0, 0, 2)):
        with pytest.raises(aacgpu.AacgError) as e:
            bad()
        assert e.value.code == ERR_INVALID_ARG
    skel = np.zeros(6, aacgpu.UNIT_DTYPE)
    skel["n_out_ch"], skel["n_ch"] = 2, 2
    skel["pcm_offset"] = np.arange(6) * 2048
    skel["coef_offset"] = skel["meta_offset"] = np.arange(6) * 2
    skel["ch"]["group_count"], skel["ch"]["group_len"][:, :, 0] = 1, 1
    d_map = torch.zeros(6 * 2, dtype=torch.int32, device="cuda")
    skel["stream"] = [0, 0, 1, 1, 0, 0]                           # stream 0 in two stretches
    plan = eng.plan(skel)
    with pytest.raises(aacgpu.AacgError) as e:
        eng.carry_window_shape(plan, d_map.data_ptr())
    assert e.value.code == ERR_UNSUPPORTED and "stretch" in str(e.value)
    with pytest.raises(aacgpu.AacgError) as e:
        eng.carry_window_shape(plan, 0)
    assert e.value.code == ERR_INVALID_ARG
    plan.destroy()
    eng.close()
    eng = aacgpu.Engine(aacgpu.INPUT_SPEC_F32, max_streams=2, max_channels=2)
    skel["stream"] = [0, 0, 0, 1, 1, 1]
    plan = eng.plan(skel)
    with pytest.raises(aacgpu.AacgError) as e:
        eng.carry_window_shape(plan, d_map.data_ptr())
    assert e.value.code == ERR_INVALID_ARG
    plan.destroy()
    eng.close()


@pytest.mark.parametrize("spec", [False, True], ids=["stages0", "stages3"])
def test_without_the_bit_the_path_is_as_it_was(streams, stage_streams, oracle, spec):
    """stages = 0 (plain streams) and stages = 3 pipelines (the streams with filters and noise bands) give the bits of the host route with window_shape_prev = 0 (what the
    parser writes and the refresh copies), in both plan modes"""
    mem = members_of(stage_streams if spec else streams, ["stereo16", "split16"], 2)
    script = rect_script(len(mem), 4, 12)
    kw = dict(tns_spec=True, pns_spec=True, parse_options=OPTIONS) if spec else {}
    want, ref, states, host = host_run(mem, script, 2, 8, oracle, carry=False, spec=spec, options=OPTIONS if spec else PLAIN)
    assert host.refused == 0 and host.routes == {EX_RV if spec else "aacg_imdct_run_quant_rv"}
    assert any(prev_w.any() for st in states for prev_w in st), "KBD frames at the batches' ends: the rule would have carried them"
    for mode in (False, True):
        got = pipe_run(mem, script, 2, 8, 4, mode, states=[np.zeros((len(mem), 2), np.uint8)] * len(script), **kw)
        assert got[2] == 0
        for s in range(len(mem)):
            assert same_bits(got[0][s], want[s]), (mode, s)
    close_to(np.concatenate(want), np.concatenate(ref))


def test_behind_the_plugin_surface(tmp_path):
    """SharedEngine({ resident: true, carryWindowShape: true }) under Node: readChunk() of 8 decoders returns the same samples, bit for
    bit, as the same decoders on the parsing route with carryWindowShape — as ADTS streams and as 'mp4a' packets (residentPackets)"""
    d = str(tmp_path)
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "shape_cases.js"), d], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "test_resident_shape.js"), "gpu", d], capture_output=True, text=True, timeout=500)
    print(r.stdout)
    assert r.returncode == 0 and "resident shape gpu tests ok" in r.stdout, r.stdout + r.stderr
