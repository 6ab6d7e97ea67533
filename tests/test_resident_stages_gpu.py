"""The spec-correct optional stages on the resident route (aacg_pipeline_config.stages, aacgpu.Pipeline(tns_spec=, pns_spec=)), on a
real MI355X: the device parser writes TNS side info, aacg_tns_records makes the records and their matrices on the lane's stream, the
refresh keeps TNS flags and noise-band units, and every launch is aacg_imdct_run_quant_ex_rv through aacg_decode_pipelined_stages.

What is new against the host-planned SPEC path is WHERE the TNS records are made, so the first yardstick is that path itself, bit for
bit: Parser.parse_batch(want_tns) -> Engine(TNS_SPEC, PNS_SPEC).plan(units, tns) -> decode_pipelined on the same batches in the same
order (the same run kernel on host-made records).  The oracle bounds both with the project's tolerances.  Then both plan modes,
ragged counts, five lanes in flight, the steady feed's overlap, `stages = 0` as it was, malformed and odd frames.

Streams: tests/js/stage_cases.js (TNS filters, noise bands and pulse data throughout; seeds fixed there).  The conditions they were
chosen for are asserted here from what the device returns."""
import os
import subprocess

import numpy as np
import pytest

import aacgpu
from resident_kit import ERR_INVALID_ARG, ERR_UNSUPPORTED, EX_RV, GROUPS, NODE, OPTIONS, PARSE_TNS_ORDER, ROOT, HostRoute, close_to, members_of, packed
from resident_kit import ragged_script, records_layout, rect_script, run_script, same_bits, silent, steady
from resident_kit import emu_tns, oracle          # noqa: F401  (fixtures: aacg_tns_prepare on the host, built with g++; the oracle)
from resident_kit import stage_streams as streams          # noqa: F401  (fixture: tests/js/stage_cases.js)

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not present")]
SPEC = dict(tns_spec=True, pns_spec=True, parse_options=OPTIONS)
# the yardstick of these tests: the host-planned SPEC path on host-made records, window_shape_prev 0, every frame parses
HOST = dict(carry=False, spec=True, options=OPTIONS, every_frame_parses=True)


@pytest.mark.parametrize("names,C_,si", GROUPS, ids=[g[0] for g in GROUPS])
def test_device_records_equal_host_records_bit_for_bit_and_the_oracle(streams, oracle, emu_tns, names, C_, si):
    """4 to 8 streams x 4 frames a batch, three batches: the pipeline's PCM against the host-planned SPEC path on the same batches
    (same bits) and against the oracle on the host-parsed records; the records the device makes of the device parser's outputs
    against aacg_tns_prepare's, byte for byte; and the conditions the streams were chosen for."""
    import torch
    names = names.split("+")
    copies = 8 // len(names) if C_ == 2 else (4 if C_ == 6 else 6)
    mem = members_of(streams, names, copies)
    S = len(mem)
    assert 4 <= S <= 8
    script = rect_script(S, 4, 12)
    got = run_script(mem, script, C_, si, 4, False, **SPEC)
    assert got[2] == 0 and not any(x.any() for x in got[1]), "every frame parses on the device"
    host = HostRoute(S, C_, si, oracle, **HOST)
    data = np.concatenate([m[0] for m in mem])
    bases = np.cumsum([0] + [len(m[0]) for m in mem])[:-1]
    want, ref = [[] for _ in range(S)], [[] for _ in range(S)]
    filters = 0
    per = 1024 * C_
    for live, counts, at in script:
        fr = packed([mem[s][1] for s in live], [bases[s] for s in live], at, counts)
        pcm, r, out = host.decode(data, fr, live, counts)
        for k, s in enumerate(live):
            want[s].append(pcm[k * 4 * per:(k + 1) * 4 * per])
            ref[s].append(r[k * 4 * per:(k + 1) * 4 * per])
        # the kernel on the GPU against the host function, on this batch's parser outputs
        n, U, Cp = len(fr), host.U, host.Cp
        m_off, total = records_layout(emu_tns, n * Cp)
        assert total == host.eng.tns_records_bytes(n * Cp)
        hbuf = np.zeros(total, np.uint8)
        assert emu_tns.emu_tns_host(si, out["units"].ctypes.data, out["results"].ctypes.data, out["tns"].ctypes.data, n, U, Cp, hbuf.ctypes.data) == 0
        d = [torch.from_numpy(out[k].view(np.uint8).reshape(-1)).cuda() for k in ("units", "results", "tns")]
        d_rec = torch.full((total + 512,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        host.eng.tns_records_from_parse(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), n, U, Cp, d_rec.data_ptr())
        host.eng.synchronize()
        dbuf = d_rec.cpu().numpy()
        assert (dbuf[total:] == 0xA5).all(), "written behind the batch's records and matrices"
        assert dbuf[:n * Cp * 512].tobytes() == hbuf[:n * Cp * 512].tobytes(), "the device's TNS records differ from aacg_tns_prepare's"
        assert dbuf[m_off:total].tobytes() == hbuf[m_off:total].tobytes(), "the device's transition matrices differ"
        batch_filters = int(sum(1 for rec in hbuf[:n * Cp * 512].view(aacgpu.DEV_TNS_DTYPE) if rec["order"].any()))
        assert batch_filters, "every batch holds a filter, so the host plan takes the route of the stages"
        filters += batch_filters
    assert host.routes == {EX_RV}
    print("%s: %d of %d channel-frames end with a filter to run, %d of %d units carry noise bands" % (names, filters, host.channel_frames, host.pns_units, host.units))
    assert 4 * filters >= host.channel_frames and 10 * host.pns_units >= host.units
    for s in range(S):
        assert same_bits(got[0][s], np.concatenate(want[s])), "stream %d: device-made records decode to other bits than host-made ones" % s
    close_to(np.concatenate(got[0]), np.concatenate([np.concatenate(r) for r in ref]))
    host.close()


def test_plans_made_for_the_stages_always_take_the_stages_route():
    """aacg_plan_create_stages and aacg_plan_create_shaped_stages on a SPEC engine: aacg_imdct_run_quant_ex_rv whether or not a batch holds
    a filter, serial or pipelined; the serial and plain pipelined launch calls refuse such a plan; engines the route does not exist on"""
    skel = np.zeros(8, aacgpu.UNIT_DTYPE)
    skel["stream"], skel["n_out_ch"], skel["n_ch"] = np.arange(8) // 4, 2, 2
    skel["pcm_offset"] = np.arange(8) * 2048
    skel["coef_offset"] = skel["meta_offset"] = np.arange(8) * 2
    skel["ch"]["group_count"], skel["ch"]["group_len"][:, :, 0] = 1, 1
    for modes in (dict(tns_mode=aacgpu.TNS_SPEC, pns_mode=aacgpu.PNS_SPEC), dict(tns_mode=aacgpu.TNS_SPEC), dict(pns_mode=aacgpu.PNS_SPEC)):
        eng = aacgpu.Engine(aacgpu.INPUT_QUANT_I16, max_streams=2, max_channels=2, **modes)
        plan = eng.plan_stages(skel)
        assert eng.plan_kernels(plan) == EX_RV and eng.plan_kernels(plan, pipelined=True) == EX_RV
        with pytest.raises(aacgpu.AacgError) as e:
            eng.decode_pipelined(plan, 256, 256, 256)
        assert e.value.code == ERR_UNSUPPORTED
        with pytest.raises(aacgpu.AacgError) as e:
            eng.decode_device(plan, 256, 256, 256)
        assert e.value.code == ERR_UNSUPPORTED
        if "tns_mode" in modes:
            with pytest.raises(aacgpu.AacgError) as e:
                eng.decode_pipelined_stages(plan, 256, 256, 0, 0, 256)          # an AACG_TNS_SPEC engine's launch needs the records
            assert e.value.code == ERR_INVALID_ARG
        shaped = eng.plan_shaped(2, 4, stages=True)
        assert eng.plan_kernels(shaped, pipelined=True) == EX_RV
        with pytest.raises(aacgpu.AacgError) as e:                 # the plain shaped plan stays what it was: none on such an engine
            eng.plan_shaped(2, 4)
        assert e.value.code == ERR_UNSUPPORTED
        plain = eng.plan(skel)
        with pytest.raises(aacgpu.AacgError) as e:
            eng.decode_pipelined_stages(plain, 256, 256, 256, 1, 256)
        assert e.value.code == ERR_INVALID_ARG
        for p in (plan, shaped, plain):
            p.destroy()
        eng.close()
    for kw in (dict(), dict(tns_mode=aacgpu.TNS_SPEC, output_kind=aacgpu.OUTPUT_I16)):
        eng = aacgpu.Engine(aacgpu.INPUT_QUANT_I16, max_streams=2, max_channels=2, **kw)
        for make in (lambda: eng.plan_stages(skel), lambda: eng.plan_shaped(2, 4, stages=True)):
            with pytest.raises(aacgpu.AacgError) as e:
                make()
            assert e.value.code == ERR_UNSUPPORTED
        eng.close()


def test_both_plan_modes_ragged_counts_and_five_lanes_in_flight(streams):
    """stereo and split-window streams at different starting frames, ragged random counts: device plans give the bits of kept plans
    without building a plan per shape; the same batches submitted ahead on five lanes give the bits of one batch at a time"""
    rng = np.random.default_rng(31)
    mem = members_of(streams, ["stereo48", "split48"], 3)
    script = ragged_script([m[1] for m in mem], 4, rng)
    kept = run_script(mem, script, 2, 3, 4, False, **SPEC)
    shaped = run_script(mem, script, 2, 3, 4, True, **SPEC)
    assert kept[2] == 0 and shaped[2] == 0
    assert shaped[3] == 0 and shaped[4]["shaped"] == shaped[4]["launches"] == len(script) and kept[3] > 0 and kept[4]["shaped"] == 0
    for s in range(len(mem)):
        assert same_bits(kept[0][s], shaped[0][s]), s
        assert np.abs(kept[0][s]).max() > 1e-3
    # in flight: every batch of the script submitted before the fifth-last is collected
    data = np.concatenate([m[0] for m in mem])
    bases = np.cumsum([0] + [len(m[0]) for m in mem])[:-1]
    p = aacgpu.Pipeline(channels=2, max_streams=len(mem), max_frames=4, lanes=5, device_plans=True, **SPEC)
    pending, out = [], []
    for live, counts, at in script:
        fr = packed([mem[s][1] for s in live], [bases[s] for s in live], at, counts)
        pending.append(p.submit(data, fr, np.array(live, np.uint32), np.array(counts, np.uint32), pcm=p.pinned(int(sum(counts)) * 2048, np.float32)))
        if len(pending) == 5:
            out.append(p.collect(pending.pop(0)))
    out += [p.collect(t) for t in pending]
    flight = [[] for _ in mem]
    for (live, counts, at), (pcm, res, refused) in zip(script, out):
        assert refused == 0 and not res["status"].any()
        first = np.concatenate([[0], np.cumsum(counts)])
        for k, s in enumerate(live):
            flight[s].append(pcm[first[k] * 2048:first[k + 1] * 2048].copy())
    p.close()
    for s in range(len(mem)):
        assert same_bits(np.concatenate(flight[s]), shaped[0][s]), s


def test_the_steady_feed_still_continues_launches_through_the_cells(streams):
    """consecutive batches of one shape are consecutive launches of one plan and meet in the cross-launch cells, with the stages
    as without them; the chained launches' bits are those of one batch at a time"""
    c, data, table = streams["stereo48"]
    (kept, pcm0), (shaped, pcm1) = steady(data, table, 6, 24, 12, False, **SPEC), steady(data, table, 6, 24, 12, True, **SPEC)
    kept, shaped = kept["chained"], shaped["chained"]
    print("continued launches of 24: kept plans %d, device plans %d" % (kept, shaped))
    assert kept > 0 and shaped > 0
    for a, b in zip(pcm0, pcm1):
        assert same_bits(a, b)
    one = aacgpu.Pipeline(channels=2, max_streams=6, max_frames=2, lanes=1, **SPEC)
    for b in range(24):
        fr = packed([table] * 6, [0] * 6, [(2 * b) % 12] * 6, [2] * 6)
        want, res, refused = one.decode(data, fr, np.arange(6), np.full(6, 2, np.uint32))
        assert refused == 0 and same_bits(want, pcm1[b]), b
    one.close()


def test_a_chain_across_three_runs(streams, oracle):
    """max_frames 40 on two streams: chains of three runs (the in-launch rendezvous) with filters and noise bands in every run —
    the stereo stream fed round, 40 frames a batch, against the host-planned path bit for bit and the oracle"""
    c, data, table = streams["stereo48"]
    mem = [(data, np.concatenate([table] * 4)[:40]), (data, np.concatenate([table[5:], table] * 3)[:40])]
    script = [([0, 1], [40, 40], [0, 0])]
    for mode in (False, True):
        got = run_script(mem, script, 2, 3, 40, mode, **SPEC)
        assert got[2] == 0
        host = HostRoute(2, 2, 3, oracle, **HOST)
        fr = packed([m[1] for m in mem], [0, 0], [0, 0], [40, 40])
        pcm, ref, out = host.decode(data, fr, [0, 1], [40, 40])
        assert host.routes == {EX_RV}
        assert same_bits(np.concatenate(got[0]), pcm)
        close_to(np.concatenate(got[0]), ref)
        host.close()


@pytest.mark.parametrize("name,si", [("mono48", 3), ("mono16", 8)])
def test_stages_zero_keeps_the_path_as_it_was(streams, oracle, emu_tns, name, si):
    """a `stages = 0` pipeline on the same bytes: a frame with noise bands is refused (silent, counted once) as ever, the others
    decode as the reference does — TNS the identity — and its PCM differs from the SPEC pipeline's on the frames whose filters
    ran: the comparison of the first test would otherwise pass with the filters never run"""
    c, data, table = streams[name]
    S = 4
    mem = [(data, table)] * S
    script = rect_script(S, 4, 12)
    plain = run_script(mem, script, 1, si, 4, False, parse_options=OPTIONS)
    spec = run_script(mem, script, 1, si, 4, False, **SPEC)
    parser = aacgpu.Parser(sample_index=si)
    out = parser.parse_batch(data, table, 1, 1, OPTIONS, True)
    parser.close()
    assert not out["results"]["status"].any()
    pns = (out["units"]["flags"] & aacgpu.UNIT_HAS_PNS) != 0
    m_off, total = records_layout(emu_tns, 12)
    hbuf = np.zeros(total, np.uint8)
    assert emu_tns.emu_tns_host(si, out["units"].ctypes.data, out["results"].ctypes.data, out["tns"].ctypes.data, 12, 1, 1, hbuf.ctypes.data) == 0
    filt = np.array([bool(r["order"].any()) for r in hbuf[:12 * 512].view(aacgpu.DEV_TNS_DTYPE)])
    both = [f for f in range(12) if filt[f] and not pns[f]]
    assert pns.any() and len(both) >= 2, "the stream has noise frames, and frames with a filter and without noise bands"
    # refused: the noise frames, once each, with a status; nothing else
    assert spec[2] == 0 and plain[2] == S * int(pns.sum())
    for s in range(S):
        assert np.array_equal(plain[1][s] != 0, pns), "a status on the noise frames and on no other"
        assert same_bits(plain[0][s], plain[0][0]) and same_bits(spec[0][s], spec[0][0])
    # the rest as the reference decodes it: the oracle without TNS records and without the noise stage, the refused frames silent
    units = out["units"].copy()
    units["stream"], units["n_out_ch"], units["pcm_offset"] = 0, 1, np.arange(12, dtype=np.uint32) * 1024
    quiet = units[pns]
    silent(quiet)
    units[pns] = quiet
    units["ch"]["flags"] = 0
    ref = oracle.decode_batch(units, out["q"], out["meta"], 12 * 1024, np.zeros((1, 1, 1024), np.float32), sample_index=si)
    close_to(plain[0][0], ref)
    # ... and where a filter ran, the SPEC pipeline's samples are others
    a, b = plain[0][0].reshape(12, 1024), spec[0][0].reshape(12, 1024)
    for f in both:
        assert not same_bits(a[f], b[f]), "frame %d carries a filter with a region: the stages' PCM must differ from the reference route's" % f


def test_malformed_and_odd_frames(streams):
    """a malformed frame among clean ones goes silent and is counted once with its status, and nobody else's PCM changes; a TNS
    order of 13 refuses the frame with AACG_PARSE_TNS_ORDER where TNS records are made (and only there); stages with int16 PCM
    fail at create with AACG_ERR_UNSUPPORTED"""
    c, data, table = streams["stereo48"]
    bad = data.copy()
    off, length = int(table[5]["byte_offset"]), int(table[5]["byte_length"])
    bad[off + 7: off + length] = 0xFF                           # frame 5: a raw_data_block with no CPE in it
    both = np.concatenate([data, bad])
    S = 4
    for mode in (False, True):
        clean = run_script([(data, table)] * S, rect_script(S, 4, 12), 2, 3, 4, mode, **SPEC)
        p = aacgpu.Pipeline(channels=2, max_streams=S, max_frames=4, device_plans=mode, **SPEC)
        pcm, status, refusals = [], [], 0
        for live, counts, at in rect_script(S, 4, 12):
            fr = packed([table] * S, [0, len(data), 0, 0], at, counts)          # slot 1 reads the copy with the bad frame
            out, res, refused = p.decode(both, fr, np.array(live, np.uint32), np.array(counts, np.uint32))
            pcm.append(out.reshape(S, 4 * 2048))
            status.append(res["status"].reshape(S, 4))
            refusals += refused
        p.close()
        pcm, status = np.concatenate(pcm, axis=1), np.concatenate(status, axis=1)
        assert refusals == 1 and status[1][5] != 0 and np.count_nonzero(status) == 1
        for s in (0, 2, 3):
            assert same_bits(pcm[s], clean[0][s]), "a neighbour's PCM changed"
        frames = pcm[1].reshape(12, 2048)
        want = clean[0][1].reshape(12, 2048)
        # (frame 5 is its predecessor's tail alone, frame 6 starts from a silent tail: both differ; frame 7 follows frame 6's own tail)
        assert same_bits(frames[:5], want[:5]) and same_bits(frames[7:], want[7:]), "the stream's frames away from the bad one changed"
        assert not same_bits(frames[5], want[5]) and np.isfinite(frames).all()
    # TNS order 13: the parser refuses the frame when TNS records are requested (orders 13..20 stay out of scope)
    c13, d13, t13 = streams["order13"]
    at = c13["oddFrame"]
    for kw, want in ((SPEC, PARSE_TNS_ORDER), (dict(parse_options=OPTIONS), 0)):
        p = aacgpu.Pipeline(channels=1, max_streams=1, max_frames=12, sample_index=c13["sampleIndex"], **kw)
        out, res, refused = p.decode(d13, t13, [0], 12)
        p.close()
        assert int(res["status"][at]) == want and refused == (1 if want else 0) and np.count_nonzero(res["status"]) == (1 if want else 0)
    with pytest.raises(aacgpu.AacgError) as e:
        aacgpu.Pipeline(channels=2, max_streams=2, max_frames=4, output_kind=aacgpu.OUTPUT_I16, tns_spec=True)
    assert e.value.code == ERR_UNSUPPORTED
    with pytest.raises(aacgpu.AacgError) as e:
        aacgpu.Pipeline(channels=2, max_streams=2, max_frames=4, output_kind=aacgpu.OUTPUT_I16, pns_spec=True)
    assert e.value.code == ERR_UNSUPPORTED


def test_behind_the_plugin_surface(tmp_path):
    """SharedEngine({ resident: true, tnsMode, pnsMode }) under Node: readChunk() returns the same samples, bit for bit, as the
    parsing route on the same engine options, in both plan modes, and the decoders report the resident route"""
    d = str(tmp_path)
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "stage_cases.js"), d], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "test_resident_stages.js"), "gpu", d], capture_output=True, text=True, timeout=500)
    print(r.stdout)
    assert r.returncode == 0 and "resident stages gpu tests ok" in r.stdout, r.stdout + r.stderr
