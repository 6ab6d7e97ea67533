"""Parity tests proper: the HIP path, called through the C ABI, against (a) the golden vectors the
REFERENCE produced and (b) the oracle on seeded synthetic batches.  All need a real MI355X.

Tolerances: spectral stage (dequant, MS, IS) bit-exact; PCM RMS error <= 1e-5 on the [-1,1) scale
(BASELINE.json allows 1e-4); overlap state within 1e-5 relative to its peak.
"""
import numpy as np
import pytest

import aacgpu
import aacgpu_workload
import orc

pytestmark = pytest.mark.gpu
RMS_TOL = 1e-5


REL_TOL = 5e-6          # relative to the signal RMS; the reference's own IMDCT is 1.3e-6 from exact


def rms(a, b):
    """RMS error on the [-1,1) PCM scale; also gates the error relative to the signal level."""
    a = np.asarray(a, np.float64).ravel()
    b = np.asarray(b, np.float64).ravel()
    d = a - b
    err = float(np.sqrt(np.mean(d * d)))
    sig = float(np.sqrt(np.mean(b * b)))
    assert err <= REL_TOL * sig + 1e-9, "relative RMS error %.3e (signal rms %.3e)" % (err / max(sig, 1e-30), sig)
    return err


def overlaps(eng, S, C):
    return np.stack([[eng.get_overlap(s, c) for c in range(C)] for s in range(S)])


SCENARIOS = ["scn_stereo", "scn_split", "scn_7ch", "scn_mono"]


def test_native_library_is_loaded(engine_lib):
    assert engine_lib.aacg_kernel_name().decode() == "aacg_imdct_run_quant_rv"
    maps = open("/proc/self/maps").read()
    assert "libaacgpu.so" in maps


def test_tables_match_reference(golden):
    eng = aacgpu.Engine(aacgpu.INPUT_SPEC_F32, 1, 1)
    for which, name in ((0, "tables.iq"), (1, "tables.sf"), (2, "tables.sine_long"), (3, "tables.kbd_long"),
                        (4, "tables.sine_short"), (5, "tables.kbd_short")):
        assert np.array_equal(eng.table(which).view(np.uint32), golden[name].view(np.uint32)), name
    eng.close()


@pytest.mark.parametrize("name", SCENARIOS)
@pytest.mark.parametrize("inp", ["q", "spec"])
def test_scenarios_vs_reference(golden, name, inp):
    """Multi-frame scenarios the reference decoded through its own readChunk(): all window sequences and
    transitions, both shapes, MS, IS, zero bands, grouped shorts, split windows, 7 channels, mono."""
    units = golden[name + ".units"].view(aacgpu.UNIT_DTYPE).ravel()
    ref = golden[name + ".pcm"]
    C = ref.shape[2]
    kind = aacgpu.INPUT_QUANT_I16 if inp == "q" else aacgpu.INPUT_SPEC_F32
    eng = aacgpu.Engine(kind, max_streams=1, max_channels=C)
    pcm = eng.decode_batch(units, golden[name + "." + inp], golden[name + ".meta"] if inp == "q" else None, ref.size)
    assert not np.isnan(pcm).any()
    assert rms(pcm, ref) < RMS_TOL
    ov = overlaps(eng, 1, C)[0]
    scale = max(1.0, float(np.abs(golden[name + ".overlap"]).max()))
    assert np.abs(ov - golden[name + ".overlap"]).max() / scale < 1e-5
    eng.close()


def test_cfg1_mono_long_frame(golden):
    """BASELINE config 1."""
    units = np.zeros(1, aacgpu.UNIT_DTYPE)
    units["n_out_ch"] = 1
    units["n_ch"] = 1
    units["ch"]["max_sfb"][0, 0] = 49
    units["ch"]["group_count"][0, 0] = 1
    units["ch"]["group_len"][0, 0, 0] = 1
    eng = aacgpu.Engine(aacgpu.INPUT_SPEC_F32, 1, 1)
    pcm = eng.decode_batch(units, golden["cfg1.spec"], None, 1024)
    assert rms(pcm, golden["cfg1.pcm"]) < RMS_TOL
    ref_ov = golden["cfg1.overlap"][0]
    assert np.abs(eng.get_overlap(0, 0) - ref_ov).max() < 1e-5 * float(np.abs(ref_ov).max())
    eng.close()


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.mark.parametrize("name", SCENARIOS)
def test_spectral_stage_bit_exact(golden, name):
    torch = _torch()
    units = golden[name + ".units"].view(aacgpu.UNIT_DTYPE).ravel()
    C = golden[name + ".pcm"].shape[2]
    eng = aacgpu.Engine(aacgpu.INPUT_QUANT_I16, 1, C)
    plan = eng.plan(units)
    dq = torch.from_numpy(golden[name + ".q"]).cuda()
    dm = torch.from_numpy(golden[name + ".meta"].view(np.int16)).cuda()
    ds = torch.zeros(dq.shape, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    eng.spectral_device(plan, dq.data_ptr(), dm.data_ptr(), ds.data_ptr(), 0)      # 0 = the engine's own stream
    eng.synchronize()
    spec = ds.cpu().numpy()
    assert np.array_equal(spec.view(np.uint32), golden[name + ".spec"].view(np.uint32))
    plan.destroy()
    eng.close()


@pytest.mark.parametrize("mix,layout,intensity", [(False, ("cpe",), False), (True, ("cpe",), True),
                                                  (True, ("cpe", "cpe", "cpe", "sce"), False), (True, ("sce",), False)])
def test_synthetic_vs_oracle(oracle, mix, layout, intensity):
    """BASELINE configs 2/3/5 at a size the oracle finishes in seconds: 16 streams x 24 frames."""
    S, T = 16, 24
    wl = aacgpu_workload.make_batch(n_streams=S, n_frames=T, layout=layout, mix=mix, intensity=intensity, seed=4321)
    C = wl["C"]
    ov = np.zeros((S, C, 1024), np.float32)
    ref, spec_ref = oracle.decode_batch(wl["units"], wl["q"], wl["meta"], wl["n_pcm"], ov, want_spec=True)
    eng = aacgpu.Engine(aacgpu.INPUT_QUANT_I16, S, C)
    pcm = eng.decode_batch(wl["units"], wl["q"], wl["meta"], wl["n_pcm"])
    assert rms(pcm, ref) < RMS_TOL
    assert np.abs(overlaps(eng, S, C) - ov).max() < 1e-5 * max(1.0, float(np.abs(ov).max()))
    eng.close()
    eng = aacgpu.Engine(aacgpu.INPUT_SPEC_F32, S, C)
    pcm = eng.decode_batch(wl["units"], spec_ref, None, wl["n_pcm"])
    assert rms(pcm, ref) < RMS_TOL
    eng.close()


def test_consecutive_batches_equal_one_batch(oracle):
    """Stream state lives in the engine: T frames as 3 batches == one batch == the oracle."""
    S, T = 4, 21
    wl = aacgpu_workload.make_batch(n_streams=S, n_frames=T, mix=True, seed=77)
    ov = np.zeros((S, 2, 1024), np.float32)
    ref = oracle.decode_batch(wl["units"], wl["q"], wl["meta"], wl["n_pcm"], ov).reshape(S, T, 2048)
    eng = aacgpu.Engine(aacgpu.INPUT_QUANT_I16, S, 2)
    units = wl["units"].reshape(S, T)
    got = np.empty((S, T, 2048), np.float32)
    for lo, hi in ((0, 9), (9, 10), (10, 21)):
        u = units[:, lo:hi].copy()
        n = hi - lo
        u["pcm_offset"] = (np.arange(S)[:, None] * n + np.arange(n)[None, :]) * 2048
        pcm = eng.decode_batch(u.ravel(), wl["q"], wl["meta"], S * n * 2048)
        got[:, lo:hi] = pcm.reshape(S, n, 2048)
    assert rms(got, ref) < RMS_TOL
    eng.close()


def test_plan_reuse_device_path(oracle):
    """A plan launched repeatedly continues the streams (double-buffered overlap, flip per launch); a second
    plan on the same streams makes the first one stale."""
    torch = _torch()
    S, T = 8, 16
    eng = aacgpu.Engine(aacgpu.INPUT_QUANT_I16, S, 2)
    wls = [aacgpu_workload.make_batch(n_streams=S, n_frames=T, mix=True, seed=5, frame_base=T * i) for i in range(3)]
    plan = eng.plan(wls[0]["units"])                       # same shape for every batch? sequences differ -> per-batch plans
    ov = np.zeros((S, 2, 1024), np.float32)
    stream = 0                                             # the engine's own HIP stream
    # identical side info three times (only the coefficients change): one plan, three launches
    for i in range(3):
        q = wls[i]["q"]
        ref = oracle.decode_batch(wls[0]["units"], q, wls[0]["meta"], wls[0]["n_pcm"], ov)
        dq = torch.from_numpy(q).cuda()
        dm = torch.from_numpy(wls[0]["meta"].view(np.int16)).cuda()
        dp = torch.empty(wls[0]["n_pcm"], dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        eng.decode_device(plan, dq.data_ptr(), dm.data_ptr(), dp.data_ptr(), stream)
        eng.synchronize()
        assert rms(dp.cpu().numpy(), ref) < RMS_TOL, i
    assert np.abs(overlaps(eng, S, 2) - ov).max() < 1e-5 * max(1.0, float(np.abs(ov).max()))
    plan2 = eng.plan(wls[0]["units"])
    dq = torch.from_numpy(wls[0]["q"]).cuda()
    dm = torch.from_numpy(wls[0]["meta"].view(np.int16)).cuda()
    dp = torch.empty(wls[0]["n_pcm"], dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    eng.decode_device(plan2, dq.data_ptr(), dm.data_ptr(), dp.data_ptr(), stream)
    with pytest.raises(aacgpu.AacgError) as ei:
        eng.decode_device(plan, dq.data_ptr(), dm.data_ptr(), dp.data_ptr(), stream)
    assert ei.value.code == -7
    eng.synchronize()
    plan.destroy()
    plan2.destroy()
    eng.close()


def test_plans_come_and_go_while_kernels_run(oracle):
    """Plan buffers are recycled through the engine's free list and filled by asynchronous copies: plans of changing size,
    created and destroyed without any synchronisation in between, launched on two streams — every batch still equals the
    oracle (a recycled buffer overwritten while a kernel still reads it, or read before its upload landed, would not)."""
    torch = _torch()
    rng = np.random.default_rng(77)
    S = 6
    eng = aacgpu.Engine(aacgpu.INPUT_QUANT_I16, 2 * S, 2)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    ov = [np.zeros((2 * S, 2, 1024), np.float32) for _ in range(2)]          # slot k owns streams k*S .. k*S+S-1
    pending = []                                                              # (plan, device buffers, reference, slot)
    checked = 0
    for it in range(40):
        k = it & 1
        wl = aacgpu_workload.make_batch(n_streams=int(rng.integers(1, S + 1)), n_frames=int(rng.integers(1, 40)), mix=True, seed=1000 + it,
                                        stream_base=k * S)
        full = np.zeros((2 * S, 2, 1024), np.float32)
        full[:] = ov[k]
        ref = oracle.decode_batch(wl["units"], wl["q"], wl["meta"], wl["n_pcm"], full)
        ov[k] = full
        with torch.cuda.stream(streams[k]):
            dq = torch.from_numpy(wl["q"]).cuda(non_blocking=True)
            dm = torch.from_numpy(wl["meta"].view(np.int16)).cuda(non_blocking=True)
            dp = torch.empty(wl["n_pcm"], dtype=torch.float32, device="cuda")
        plan = eng.plan(wl["units"])
        eng.decode_device(plan, dq.data_ptr(), dm.data_ptr(), dp.data_ptr(), streams[k].cuda_stream)
        pending.append((plan, (dq, dm, dp), ref, k))
        if len(pending) > 2:                                                  # retire the oldest: its kernel may still be running
            old_plan, bufs, old_ref, ok = pending.pop(0)
            old_plan.destroy()
            streams[ok].synchronize()
            assert rms(bufs[2].cpu().numpy(), old_ref) < RMS_TOL, it
            checked += 1
    torch.cuda.synchronize()
    for old_plan, bufs, old_ref, ok in pending:
        assert rms(bufs[2].cpu().numpy(), old_ref) < RMS_TOL
        old_plan.destroy()
    assert checked == 38
    eng.close()


def test_overlap_set_get_reset():
    eng = aacgpu.Engine(aacgpu.INPUT_SPEC_F32, 2, 2)
    v = np.arange(1024, dtype=np.float32)
    eng.set_overlap(1, 1, v)
    assert np.array_equal(eng.get_overlap(1, 1), v)
    assert not eng.get_overlap(1, 0).any()
    # overlap is what the next frame starts from: a zero spectrum frame outputs overlap / 32768 (ONLY_LONG)
    wl = aacgpu_workload.make_batch(n_streams=2, n_frames=1)
    pcm = eng.decode_batch(wl["units"], np.zeros((4, 1024), np.float32), None, wl["n_pcm"]).reshape(2, 1024, 2)
    assert np.allclose(pcm[1, :, 1], v / 32768.0, rtol=0, atol=1e-7)
    eng.set_overlap(1, 1, v)
    eng.reset_stream(1)
    assert not eng.get_overlap(1, 1).any()
    eng.close()


def test_full_size_properties():
    """BASELINE config 2 at full size (256 streams x 16 frames = 4096 stereo frames), checked through
    size-independent properties: linearity of the filterbank seam, and TDAC — a frame's first-half
    output plus the previous tail reconstructs, so decoding frames one batch at a time equals decoding
    them in one batch bit-for-bit."""
    S, T = 256, 16
    wl = aacgpu_workload.make_batch(n_streams=S, n_frames=T, seed=2)
    rng = np.random.default_rng(0)
    a = (rng.standard_normal((S * T * 2, 1024)) * 100).astype(np.float32)
    b = (rng.standard_normal((S * T * 2, 1024)) * 100).astype(np.float32)

    def run(x):
        eng = aacgpu.Engine(aacgpu.INPUT_SPEC_F32, S, 2)
        out = eng.decode_batch(wl["units"], x, None, wl["n_pcm"])
        eng.close()
        return out

    pa, pb, pab = run(a), run(b), run((a + b).astype(np.float32))
    assert not np.isnan(pab).any()
    scale = float(np.sqrt(np.mean(pab.astype(np.float64) ** 2)))
    lin = np.sqrt(np.mean((pa.astype(np.float64) + pb - pab) ** 2))
    assert lin < 2e-6 * max(scale, 1e-3) + 1e-7
    # one batch of 16 frames == 16 batches of 1 frame, bit for bit (same kernels, state through HBM)
    eng = aacgpu.Engine(aacgpu.INPUT_SPEC_F32, S, 2)
    units = wl["units"].reshape(S, T)
    got = np.empty((S, T, 2048), np.float32)
    for t in range(T):
        u = units[:, t].copy()
        u["pcm_offset"] = np.arange(S) * 2048
        got[:, t] = eng.decode_batch(u, a, None, S * 2048).reshape(S, 2048)
    eng.close()
    d = np.abs(got.ravel() - pa)
    assert d.max() <= 1e-6 * max(1.0, float(np.abs(pa).max()))


def test_errors():
    eng = aacgpu.Engine(aacgpu.INPUT_QUANT_I16, 1, 2)
    wl = aacgpu_workload.make_batch(n_streams=1, n_frames=2)
    meta = wl["meta"].copy()
    meta[0, 3] = (13 << 12) | 150                         # NOISE_BT: the reference cannot decode it either
    with pytest.raises(aacgpu.AacgError) as ei:
        eng.decode_batch(wl["units"], wl["q"], meta, wl["n_pcm"])
    assert ei.value.code == -5
    u = wl["units"].copy()
    u["stream"] = 3
    with pytest.raises(aacgpu.AacgError) as ei:
        eng.decode_batch(u, wl["q"], wl["meta"], wl["n_pcm"])
    assert ei.value.code == -4
    with pytest.raises(aacgpu.AacgError):
        eng.decode_batch(wl["units"], wl["q"], wl["meta"], 100)          # pcm buffer too small
    eng.close()


def test_pipelined_submit_wait(oracle):
    """aacg_submit / aacg_wait: two batches in flight on two streams, pinned buffers; kernels stay in
    submission order (they chain through the overlap state), so 6 pipelined batches == one 48-frame batch."""
    S, T, NB = 8, 8, 6
    eng = aacgpu.Engine(aacgpu.INPUT_QUANT_I16, S, 2)
    wl = aacgpu_workload.make_batch(n_streams=S, n_frames=T * NB, mix=True, intensity=True, seed=31)
    ov = np.zeros((S, 2, 1024), np.float32)
    ref = oracle.decode_batch(wl["units"], wl["q"], wl["meta"], wl["n_pcm"], ov).reshape(S, T * NB, 2048)
    units = wl["units"].reshape(S, T * NB)
    bufs, tickets = [], []
    for b in range(NB):
        u = units[:, b * T:(b + 1) * T].copy()
        u["pcm_offset"] = (np.arange(S)[:, None] * T + np.arange(T)[None, :]) * 2048
        blocks = (u["coef_offset"].ravel()[:, None] + np.arange(2)[None, :]).ravel()
        q = eng.pinned((S * T * 2, 1024), np.int16)
        m = eng.pinned((S * T * 2, 120), np.uint16)
        q[:] = wl["q"][blocks]
        m[:] = wl["meta"][blocks]
        u["coef_offset"] = np.arange(S * T).reshape(S, T) * 2
        u["meta_offset"] = u["coef_offset"]
        pcm = eng.pinned((S * T * 2048,), np.float32)
        pcm[:] = np.nan
        uu = np.ascontiguousarray(u.ravel())
        bufs.append((uu, q, m, pcm))
        tickets.append(eng.submit(uu, q, m, pcm))
        if b >= 1:
            eng.wait(tickets[b - 1])                       # keep two in flight
    eng.wait(tickets[-1])
    got = np.stack([bufs[b][3].reshape(S, T, 2048) for b in range(NB)], axis=1).reshape(S, NB * T, 2048)
    assert rms(got, ref) < RMS_TOL
    assert np.abs(overlaps(eng, S, 2) - ov).max() < 1e-5 * max(1.0, float(np.abs(ov).max()))
    eng.close()


def _ragged_batch(seed=5):
    """Streams with different frame counts, units of different streams interleaved in the list (decode order only has
    to hold per stream)."""
    counts = [3, 17, 1, 33, 16, 2]
    parts = []
    for s, T in enumerate(counts):
        wl = aacgpu_workload.make_batch(n_streams=1, n_frames=T, mix=True, intensity=(s % 2 == 0), seed=seed + s, stream_base=s)
        parts.append(wl)
    n_frames = sum(counts)
    units = np.concatenate([p["units"] for p in parts])
    q = np.concatenate([p["q"] for p in parts])
    meta = np.concatenate([p["meta"] for p in parts])
    base = np.cumsum([0] + counts[:-1])
    off = np.concatenate([np.full(c, b) for c, b in zip(counts, base)])
    units["pcm_offset"] += (off * 2048).astype(np.uint32)
    units["coef_offset"] += (off * 2).astype(np.uint32)
    units["meta_offset"] += (off * 2).astype(np.uint32)
    # interleave streams round-robin while keeping each stream's own order
    order, cursors = [], [0] * len(counts)
    starts = list(base)
    while len(order) < n_frames:
        for s, T in enumerate(counts):
            if cursors[s] < T:
                order.append(starts[s] + cursors[s])
                cursors[s] += 1
    return units[np.array(order)], q, meta, n_frames * 2048, len(counts)


def test_ragged_interleaved_streams(oracle):
    units, q, meta, n_pcm, S = _ragged_batch()
    ov = np.zeros((S, 2, 1024), np.float32)
    ref = oracle.decode_batch(units, q, meta, n_pcm, ov)
    eng = aacgpu.Engine(aacgpu.INPUT_QUANT_I16, S, 2)
    pcm = eng.decode_batch(units, q, meta, n_pcm)
    assert rms(pcm, ref) < RMS_TOL
    assert np.abs(overlaps(eng, S, 2) - ov).max() < 1e-5 * max(1.0, float(np.abs(ov).max()))
    eng.close()


def test_extremes(oracle):
    """Maximum band counts and group counts, eight channels, escape magnitudes up to 8190, |q| >= 8191 -> NaN like the
    reference's out-of-range IQ_TABLE read, all-zero band types -> silence with overlap flushed, empty batch refused."""
    S = 1
    wl = aacgpu_workload.make_batch(n_streams=S, n_frames=6, layout=("cpe", "cpe", "cpe", "cpe"), mix=True, seed=9)
    u, q, meta = wl["units"].copy(), wl["q"].copy(), wl["meta"].copy()
    assert u["n_out_ch"][0] == 8
    short = u["ch"]["window_sequence"][:, 0] == 2
    for c in range(2):                                         # eight groups of one window, maxSFB 14
        gl = u["ch"]["group_len"][:, c].copy()
        gl[short] = 1
        u["ch"]["group_len"][:, c] = gl
        u["ch"]["group_count"][short, c] = 8
    bt = np.full(120, 11 << 12, np.uint16) | 236                # every band escape-coded
    for i in np.nonzero(short)[0]:
        meta[u["meta_offset"][i]] = np.where(np.arange(120) < 112, bt | 0x400, 0)
        meta[u["meta_offset"][i] + 1] = np.where(np.arange(120) < 112, bt, 0)
    q[::7, ::13] = 8190
    q[3::11, 5::17] = -8190
    ov = np.zeros((S, 8, 1024), np.float32)
    ref = oracle.decode_batch(u, q, meta, wl["n_pcm"], ov)
    eng = aacgpu.Engine(aacgpu.INPUT_QUANT_I16, S, 8)
    pcm = eng.decode_batch(u, q, meta, wl["n_pcm"])
    assert np.isfinite(ref).all()
    rms(pcm, ref)                                              # |PCM| reaches the hundreds here: the relative gate inside rms() applies
    # |q| = 8191 and beyond: NaN in exactly the frames (and their successors through the overlap) where the oracle has NaN
    q2 = q.copy()
    q2[int(u["coef_offset"][8]), 40] = 8191
    q2[int(u["coef_offset"][12]) + 1, 7] = -32768
    ov[:] = 0
    ref2 = oracle.decode_batch(u, q2, meta, wl["n_pcm"], ov)
    eng.reset_stream(0)
    pcm2 = eng.decode_batch(u, q2, meta, wl["n_pcm"])
    assert np.isnan(ref2).any() and np.array_equal(np.isnan(pcm2), np.isnan(ref2))
    ok = ~np.isnan(ref2)
    rms(pcm2[ok], ref2[ok])
    # all bands ZERO_BT: output is the flushed overlap, then exact silence
    eng.reset_stream(0)
    eng.decode_batch(u, q, meta, wl["n_pcm"])
    zmeta = np.zeros_like(meta)
    first = eng.decode_batch(u, q, zmeta, wl["n_pcm"]).reshape(6, 1024, 8)
    assert np.abs(first[0]).max() > 0 and not first[2:].any()
    # empty batch
    with pytest.raises(aacgpu.AacgError) as ei:
        eng.decode_batch(u[:0], q, meta, wl["n_pcm"])
    assert ei.value.code == -1
    eng.close()


def test_many_streams_multi_round(oracle):
    """2048 streams x 16 frames (8 batches' worth, 2048 workgroups: many rounds per CU); the oracle checks a sample of
    the streams (streams are independent) and a checksum of checksums guards the rest against cross-talk."""
    S, T = 2048, 16
    wl = aacgpu_workload.make_batch(n_streams=S, n_frames=T, mix=True, seed=123)
    eng = aacgpu.Engine(aacgpu.INPUT_QUANT_I16, S, 2)
    pcm = eng.decode_batch(wl["units"], wl["q"], wl["meta"], wl["n_pcm"]).reshape(S, T * 2048)
    assert np.isfinite(pcm).all()
    units = wl["units"].reshape(S, T)
    for s in (0, 1, 255, 256, 1023, 2047):
        u = units[s].copy()
        u["stream"] = 0
        ov = np.zeros((1, 2, 1024), np.float32)
        ref = oracle.decode_batch(u, wl["q"], wl["meta"], wl["n_pcm"], ov)[s * T * 2048:(s + 1) * T * 2048]
        assert rms(pcm[s], ref) < RMS_TOL
        assert np.abs(overlaps(eng, s + 1, 2)[s] - ov[0]).max() < 1e-5 * max(1.0, float(np.abs(ov).max()))
    # decoding again in two halves (streams 0..1023, 1024..2047) from a fresh engine gives bit-identical PCM
    eng2 = aacgpu.Engine(aacgpu.INPUT_QUANT_I16, S, 2)
    half = S * T // 2
    a = eng2.decode_batch(wl["units"][:half], wl["q"], wl["meta"], wl["n_pcm"])[:half * 2048]
    ub = wl["units"][half:].copy()
    b = eng2.decode_batch(ub, wl["q"], wl["meta"], wl["n_pcm"])[half * 2048:]
    assert np.array_equal(np.concatenate([a, b]).view(np.uint32), pcm.ravel().view(np.uint32))
    eng.close()
    eng2.close()


@pytest.mark.parametrize("seed", list(range(100, 124)))
def test_fuzz_vs_oracle(oracle, seed):
    """24 random batches: random channel layouts (1..8 channels), frame counts, window sequences in any order, both
    shapes and previous shapes, groupings, maxSFB (also 0), common / split windows, band types, MS masks, escapes."""
    wl = aacgpu_workload.random_batch(seed, n_streams=4, max_frames=40)
    S, C = wl["n_streams"], wl["max_channels"]
    ov = np.zeros((S, C, 1024), np.float32)
    ref = oracle.decode_batch(wl["units"], wl["q"], wl["meta"], wl["n_pcm"], ov)
    eng = aacgpu.Engine(aacgpu.INPUT_QUANT_I16, S, C)
    pcm = eng.decode_batch(wl["units"], wl["q"], wl["meta"], wl["n_pcm"])
    rms(pcm, ref)
    assert np.abs(overlaps(eng, S, C) - ov).max() < 1e-5 * max(1.0, float(np.abs(ov).max()))
    eng.close()


@pytest.mark.parametrize("T", [32, 47, 128])
def test_long_chains_double_duty(oracle, T):
    """BASELINE config 4 shape (few streams, long chains): later runs of 16 frames whose first wave recomputes the
    predecessor's tail before its own frame; also through a reused plan (flip) and the f32 seam."""
    S = 6
    wl = aacgpu_workload.make_batch(n_streams=S, n_frames=T, mix=True, intensity=True, seed=900 + T)
    ov = np.zeros((S, 2, 1024), np.float32)
    ref, spec = oracle.decode_batch(wl["units"], wl["q"], wl["meta"], wl["n_pcm"], ov, want_spec=True)
    eng = aacgpu.Engine(aacgpu.INPUT_QUANT_I16, S, 2)
    pcm = eng.decode_batch(wl["units"], wl["q"], wl["meta"], wl["n_pcm"])
    assert rms(pcm, ref) < RMS_TOL
    assert np.abs(overlaps(eng, S, 2) - ov).max() < 1e-5 * max(1.0, float(np.abs(ov).max()))
    # the next batch of the same shape continues the streams
    ref2 = oracle.decode_batch(wl["units"], wl["q"], wl["meta"], wl["n_pcm"], ov)
    pcm2 = eng.decode_batch(wl["units"], wl["q"], wl["meta"], wl["n_pcm"])
    assert rms(pcm2, ref2) < RMS_TOL
    eng.close()
    eng = aacgpu.Engine(aacgpu.INPUT_SPEC_F32, S, 2)
    pcm = eng.decode_batch(wl["units"], spec, None, wl["n_pcm"])
    assert rms(pcm, ref) < RMS_TOL
    eng.close()


@pytest.mark.parametrize("sample_index", [8, 5])
def test_extremes_at_the_tables_maxima(oracle, sample_index):
    """The real maxima next to test_extremes: at sample index 8 eight one-window groups of 15 bands (120 band records, the
    whole of aacg_band_meta), at 5 long windows of 51 bands; every band escape-coded, magnitudes up to 8190, MS on every band
    of the first CPE; rms() and the per-block gate against the exact-roots oracle."""
    import edge_cases
    import parity
    S = 1
    wl = aacgpu_workload.make_batch(n_streams=S, n_frames=8, layout=("cpe", "cpe", "cpe", "cpe"), mix=True, seed=19)
    u, q, meta = wl["units"].copy(), wl["q"].copy(), wl["meta"].copy()
    lo, so = edge_cases.tables(oracle, sample_index)
    short = u["ch"]["window_sequence"][:, 0] == 2
    for c in range(2):
        gl = u["ch"]["group_len"][:, c].copy()
        gl[short] = 1
        u["ch"]["group_len"][:, c] = gl
        u["ch"]["group_count"][short, c] = 8
        u["ch"]["max_sfb"][:, c] = np.where(short, len(so) - 1, len(lo) - 1)
    nb = np.where(short, 8 * (len(so) - 1), len(lo) - 1)
    assert nb.max() == (120 if sample_index == 8 else 112) and (sample_index != 5 or (nb == 51).any())
    bt = np.full(120, 11 << 12, np.uint16) | 236
    for i in range(len(u)):
        for c in range(2):
            meta[u["meta_offset"][i] + c] = np.where(np.arange(120) < nb[i], bt | (0x400 if c == 0 and i % 4 == 0 else 0), 0)
    q[::7, ::13] = 8190
    q[3::11, 5::17] = -8190
    q[1::5, 1016:] = 8190                                      # the top of the top band
    ov = np.zeros((S, 8, 1024), np.float32)
    ref = oracle.decode_batch(u, q, meta, wl["n_pcm"], ov, sample_index=sample_index)
    exact = parity.exact_reference(oracle, u, q, meta, wl["n_pcm"], np.zeros((S, 8, 1024), np.float32), sample_index=sample_index)
    eng = aacgpu.Engine(aacgpu.INPUT_QUANT_I16, S, 8, sample_index=sample_index)
    pcm = eng.decode_batch(u, q, meta, wl["n_pcm"])
    assert np.isfinite(ref).all()
    rms(pcm, ref)
    w = parity.assert_blocks(pcm, exact, u, what="sample index %d" % sample_index)
    print("per-block worst si %d: rms %.3e max %.3e" % (sample_index, w[0], w[1]))
    assert np.abs(overlaps(eng, S, 8) - ov).max() < 1e-5 * max(1.0, float(np.abs(ov).max()))
    eng.close()


@pytest.mark.parametrize("sample_index,max_long", [(5, 49), (6, 47), (8, 43), (0, 41)])
def test_other_sample_rates(oracle, sample_index, max_long):
    """Band tables of other sampling rates (tables.js:34-155) through the real engine: 32, 24, 16, 96 kHz, max_sfb stretched
    onto each table's own long and short counts (edge_cases.stretch_max_sfb; max_long: the cap below the table once applied),
    the per-block gate against the exact-roots oracle next to rms()."""
    import edge_cases
    import parity
    wl = aacgpu_workload.random_batch(600 + sample_index, n_streams=3, max_frames=12)
    units, meta = edge_cases.stretch_max_sfb(oracle, wl, sample_index, max_long)
    S, C = wl["n_streams"], wl["max_channels"]
    ov = np.zeros((S, C, 1024), np.float32)
    ref = oracle.decode_batch(units, wl["q"], meta, wl["n_pcm"], ov, sample_index=sample_index)
    exact = parity.exact_reference(oracle, units, wl["q"], meta, wl["n_pcm"], np.zeros((S, C, 1024), np.float32),
                                   sample_index=sample_index)
    eng = aacgpu.Engine(aacgpu.INPUT_QUANT_I16, S, C, sample_index=sample_index)
    pcm = eng.decode_batch(units, wl["q"], meta, wl["n_pcm"])
    rms(pcm, ref)
    w = parity.assert_blocks(pcm, exact, units, what="sample index %d" % sample_index)
    print("per-block worst si %d: rms %.3e max %.3e" % (sample_index, w[0], w[1]))
    assert np.abs(overlaps(eng, S, C) - ov).max() < 1e-5 * max(1.0, float(np.abs(ov).max()))
    eng.close()


# ---- the exact bench workload, and the multi-process path ------------------------------------------------
BENCH_WORKLOADS = {
    # name: (streams, frames per stream, window-sequence mix, element layout, sampled streams)
    "cfg2": (256, 16, False, ("cpe",), 16),
    "cfg3": (256, 16, True, ("cpe",), 16),
    "cfg4": (32, 128, True, ("cpe",), 4),                     # one GPU's shard of config 4: chains of 8 runs, double-duty first waves
    "cfg5": (256, 16, True, ("cpe", "cpe", "cpe", "sce"), 16),  # 4096 frames x 7 channels
}


@pytest.mark.parametrize("name", sorted(BENCH_WORKLOADS))
def test_bench_workload_vs_oracle(oracle, name):
    """bench.py's own step at BASELINE's full sizes — config 2 (256 streams x 16 ONLY_LONG stereo frames, KBD), config 3 (the
    window-sequence mix: filter_bank.js:105-202, all four sequences and both shapes), one GPU's shard of config 4 (32 streams x
    128 frames: the overlap state chained through eight runs, filter_bank.js:38-41) and config 5 (4096 frames of 3 CPE + LFE,
    the 7-way interleave of decoder.js:203-215) — int16 seam, one launch of a plan on device-resident buffers, same generator and
    seed as bench.py.  Against the oracle: the sampled streams at full precision (the oracle decodes exactly those streams'
    units alone), and the rest through split invariance: they are bit-identical whether decoded in the full launch or in a
    launch of their own."""
    torch = _torch()
    S, T, mix, layout, n_sampled = BENCH_WORKLOADS[name]
    C = sum(2 if e == "cpe" else 1 for e in layout)
    wl = aacgpu_workload.make_batch(n_streams=S, n_frames=T, mix=mix, layout=layout, seed=0xAAC00002)
    eng = aacgpu.Engine(aacgpu.INPUT_QUANT_I16, max_streams=S, max_channels=C)
    plan = eng.plan(wl["units"])
    # the route the planner picks: frames of more than two channels take the multichannel variant (non-temporal loads of the
    # spectra, aacg_engine_nt.hip), config 4's long chains the run-to-run rendezvous, the rest the plain kernel
    assert eng.plan_kernels(plan) == {"cfg2": "aacg_imdct_run_quant", "cfg3": "aacg_imdct_run_quant", "cfg4": "aacg_imdct_run_quant_rv",
                                      "cfg5": "aacg_imdct_run_quant_nt"}[name]
    d_q, d_meta = torch.from_numpy(wl["q"]).cuda(), torch.from_numpy(wl["meta"].view(np.int16)).cuda()
    d_pcm = torch.full((wl["n_pcm"],), float("nan"), dtype=torch.float32, device="cuda")
    stream = torch.cuda.Stream()
    eng.decode_device(plan, d_q.data_ptr(), d_meta.data_ptr(), d_pcm.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    pcm = d_pcm.cpu().numpy().reshape(S, T * 1024 * C)
    assert np.isfinite(pcm).all()
    sampled = list(range(0, S, S // n_sampled))
    units = wl["units"]
    for s in sampled:
        ov = np.zeros((S, C, 1024), np.float32)
        ref = oracle.decode_batch(units[units["stream"] == s], wl["q"], wl["meta"], wl["n_pcm"], ov).reshape(S, T * 1024 * C)[s]
        assert rms(pcm[s], ref) < RMS_TOL                        # rms() also gates the error relative to the signal level
        for c in range(C):
            assert np.abs(eng.get_overlap(s, c) - ov[s, c]).max() <= 1e-5 * max(1.0, float(np.abs(ov[s, c]).max()))
    plan.destroy()
    rest = units[~np.isin(units["stream"], sampled)]
    eng2 = aacgpu.Engine(aacgpu.INPUT_QUANT_I16, max_streams=S, max_channels=C)
    alone = eng2.decode_batch(rest, wl["q"], wl["meta"], wl["n_pcm"]).reshape(S, T * 1024 * C)
    others = [s for s in range(S) if s not in sampled]
    assert np.array_equal(alone[others].view(np.uint32), pcm[others].view(np.uint32))
    eng.close()
    eng2.close()


@pytest.mark.parametrize("S,T", [(64, 16), (8, 48)])
def test_one_plan_on_alternating_hip_streams(S, T):
    """Launches of ONE plan continue each other's overlap state (and, for chains longer than a run, reuse the rendezvous
    cells): the engine orders them on the device also when they alternate between two HIP streams with no host
    synchronisation in between (include/aacgpu.h, aacg_decode_device).  Eight batches that way are bit-identical to eight
    batches on one stream."""
    torch = _torch()
    wl = aacgpu_workload.make_batch(n_streams=S, n_frames=T, mix=True, seed=4242)
    d_q, d_meta = torch.from_numpy(wl["q"]).cuda(), torch.from_numpy(wl["meta"].view(np.int16)).cuda()
    out = []
    for streams in ([torch.cuda.Stream()], [torch.cuda.Stream(), torch.cuda.Stream()]):
        eng = aacgpu.Engine(aacgpu.INPUT_QUANT_I16, max_streams=S, max_channels=2)
        plan = eng.plan(wl["units"])
        d_pcm = [torch.full((wl["n_pcm"],), float("nan"), dtype=torch.float32, device="cuda") for _ in range(8)]
        torch.cuda.synchronize()
        for i in range(8):
            eng.decode_device(plan, d_q.data_ptr(), d_meta.data_ptr(), d_pcm[i].data_ptr(), streams[i % len(streams)].cuda_stream)
        torch.cuda.synchronize()
        out.append(np.stack([t.cpu().numpy() for t in d_pcm]))
        plan.destroy()
        eng.close()
    assert np.isfinite(out[0]).all()
    assert np.array_equal(out[0].view(np.uint32), out[1].view(np.uint32))


def test_two_ranks_share_a_gpu(tmp_path):
    """The sharded path with the product in it: two rank processes (torch.distributed.run, gloo for the barrier), each with
    its own aacgpu.Engine on cuda:0 for its stream shard; their PCM, concatenated, is bit-identical to one process decoding
    every stream (SURVEY.md §4 'multi-GPU' row; on an 8-GPU node the same ranks sit on 8 devices)."""
    import json
    import os
    import aacgpu_shard
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path)
    S, T = 6, 20
    rc = aacgpu_shard.self_launch(2, os.path.join(root, "tests", "shard_rank.py"),
                                  ["--out", out, "--streams", str(S), "--frames", str(T), "--decoder", "engine"], timeout=900)
    assert rc == 0
    summary = json.load(open(os.path.join(out, "summary.json")))
    assert summary["world"] == 2 and summary["frames"] == S * T
    wl = aacgpu_workload.make_batch(n_streams=S, n_frames=T, mix=True, intensity=True, seed=0xAAC00004)
    eng = aacgpu.Engine(aacgpu.INPUT_QUANT_I16, max_streams=S, max_channels=2)
    whole = eng.decode_batch(wl["units"], wl["q"], wl["meta"], wl["n_pcm"])
    eng.close()
    parts = np.concatenate([np.fromfile(os.path.join(out, "pcm_rank%d.f32" % r), np.float32) for r in range(2)])
    assert parts.size == whole.size and np.array_equal(parts.view(np.uint32), whole.view(np.uint32))


def test_two_ranks_cut_the_streams_in_time(tmp_path):
    """The other partitioning of SURVEY.md §8e with the product in it: each rank's engine decodes a span of frames of every
    stream plus the one frame in front of it (for its tail only); the spans together == one engine running straight through."""
    import os
    import aacgpu_shard
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path)
    S, T = 4, 37
    rc = aacgpu_shard.self_launch(2, os.path.join(root, "tests", "shard_rank.py"),
                                  ["--out", out, "--streams", str(S), "--frames", str(T), "--decoder", "engine", "--shard", "time"], timeout=900)
    assert rc == 0
    wl = aacgpu_workload.make_batch(n_streams=S, n_frames=T, mix=True, intensity=True, seed=0xAAC00004)
    eng = aacgpu.Engine(aacgpu.INPUT_QUANT_I16, max_streams=S, max_channels=2)
    whole = eng.decode_batch(wl["units"], wl["q"], wl["meta"], wl["n_pcm"]).reshape(S, T, -1)
    eng.close()
    spans = [aacgpu_shard.time_shard(T, r, 2) for r in range(2)]
    parts = [np.fromfile(os.path.join(out, "pcm_rank%d.f32" % r), np.float32).reshape(S, hi - lo, -1) for r, (lo, hi, _) in enumerate(spans)]
    got = np.concatenate(parts, axis=1)
    assert got.shape == whole.shape and np.array_equal(got.view(np.uint32), whole.view(np.uint32))


def test_bench_launches_its_own_ranks():
    """`python bench.py --gpus 2` without a launcher starts two ranks itself (before touching the GPU) and rank 0 prints the
    JSON line with n_gpus 2.  The box has one GPU, so the ranks share it (--share-gpu, gloo barrier): this checks the launch
    path and the whole-job arithmetic, not scaling."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "20", "--warmup", "5", "--precondition-ms", "20",
                        "--dist-backend", "gloo", "--share-gpu"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["steps"] == 20 and line["output_ok"] and line["parity_rms"] < 1e-5
    assert abs(line["value"] - 2 * 4096 / (line["ms_per_step"] * 1e-3)) < 1e-6 * line["value"]


def test_bench_dumps_its_last_timed_step(tmp_path, oracle):
    """`bench.py --steps K --dump-outputs DIR`: the line times exactly K steps (one run of the region), and DIR/pcm.npy is the PCM
    of the last of them.  With one buffer set every step decodes the same config-2 batch, so that PCM is the batch decoded
    behind itself: the oracle's second pass over it, chained through the overlap state."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "37", "--warmup", "3", "--precondition-ms", "20", "--nbuf", "1",
                        "--no-cpu-baseline", "--no-parity", "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 37 and line["timing"]["repeats"] == 1 and line["output_ok"]
    assert sorted(os.listdir(tmp_path)) == ["pcm.npy"]
    pcm = np.load(tmp_path / "pcm.npy")
    wl = aacgpu_workload.make_batch(n_streams=256, n_frames=16, seed=0xAAC00002)
    ov = np.zeros((256, 2, 1024), np.float32)
    first = oracle.decode_batch(wl["units"], wl["q"], wl["meta"], wl["n_pcm"], ov)
    ref = oracle.decode_batch(wl["units"], wl["q"], wl["meta"], wl["n_pcm"], ov)
    assert pcm.dtype == np.float32 and pcm.shape == (wl["n_pcm"],)
    assert rms(pcm, ref) < RMS_TOL and not np.allclose(first, ref)


def test_plan_refresh_units_keeps_one_plan(oracle):
    """aacg_plan_refresh_units: batch after batch of the same streams — new window sequences, shapes, grouping, M/S and block
    offsets every time (the config-3 mix at different phases) — runs on ONE plan whose unit records are replaced from the
    host's, against the oracle chained through the overlap state; a batch of another structure is refused with
    LAYOUT_CHANGE and leaves the plan usable."""
    torch = _torch()
    S, T = 12, 16
    eng = aacgpu.Engine(aacgpu.INPUT_QUANT_I16, max_streams=S, max_channels=2)
    ov = np.zeros((S, 2, 1024), np.float32)
    stream = torch.cuda.Stream()
    plan = None
    for b in range(4):
        wl = aacgpu_workload.make_batch(n_streams=S, n_frames=T, mix=True, intensity=True, seed=7300 + b, frame_base=b * T + b)
        if plan is None:
            plan = eng.plan(wl["units"])
        else:
            eng.plan_refresh_units(plan, wl["units"], stream.cuda_stream)
        d_q, d_meta = torch.from_numpy(wl["q"]).cuda(), torch.from_numpy(wl["meta"].view(np.int16)).cuda()
        d_pcm = torch.full((wl["n_pcm"],), float("nan"), dtype=torch.float32, device="cuda")
        eng.decode_device(plan, d_q.data_ptr(), d_meta.data_ptr(), d_pcm.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        ref = oracle.decode_batch(wl["units"], wl["q"], wl["meta"], wl["n_pcm"], ov)
        assert rms(d_pcm.cpu().numpy(), ref) < RMS_TOL
    assert np.abs(overlaps(eng, S, 2) - ov).max() <= 1e-5 * max(1.0, float(np.abs(ov).max()))
    other = aacgpu_workload.make_batch(n_streams=S, n_frames=T - 1, mix=True, seed=1)
    with pytest.raises(aacgpu.AacgError) as ei:
        eng.plan_refresh_units(plan, other["units"], stream.cuda_stream)
    assert ei.value.code == -6                                   # AACG_ERR_LAYOUT_CHANGE
    moved = wl["units"].copy()
    moved["pcm_offset"][3] += 2048
    with pytest.raises(aacgpu.AacgError):
        eng.plan_refresh_units(plan, moved, stream.cuda_stream)
    eng.decode_device(plan, d_q.data_ptr(), d_meta.data_ptr(), d_pcm.data_ptr(), stream.cuda_stream)   # still the last good records
    stream.synchronize()
    assert np.isfinite(d_pcm.cpu().numpy()).all()
    plan.destroy()
    eng.close()


def test_two_gpus_rccl_config4():
    """On a box with at least two GPUs (skipped on the one-GPU boxes of this pool): `bench.py --gpus 2 --workload cfg4` with one
    rank per GPU and RCCL (= the nccl backend over xGMI) carrying the harness's barrier and 8-byte MAX — BASELINE config 4's
    launch line at N = 2, so that the driver's scaling run needs nothing this suite has not run.  Each rank checks its own batch
    against the oracle (parity_rms); the line must name nccl and the world size the backend reports."""
    import json
    import os
    import subprocess
    import sys
    torch = _torch()
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs (one rank per GPU over RCCL)")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--workload", "cfg4", "--steps", "50", "--warmup", "10",
                        "--precondition-ms", "50"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["output_ok"] and line["parity_rms"] < 1e-5 and line["scaling"] == "weak"
    assert "nccl" in line["config"]["collectives"] and "world size 2" in line["config"]["collectives"]
    assert abs(line["value"] - 2 * 4096 / (line["ms_per_step"] * 1e-3)) < 1e-6 * line["value"]


@pytest.mark.parametrize("layout,T", [(("cpe", "cpe", "cpe", "sce"), 40), (("sce", "cpe", "cpe", "sce"), 21), (("sce", "cpe", "cpe", "cpe", "sce"), 7),
                                      (("sce",) * 8, 5), (("cpe", "cpe", "cpe", "sce"), 16)])
def test_multichannel_long_chains(oracle, layout, T):
    """Multichannel layouts (7 channels, 5.1, 7.1, eight mono elements) with chains longer than a run: the in-place
    overlap-add + consecutive-sample stores of the multichannel epilogue, later runs that redo the frame before them, two
    consecutive batches chained through the overlap state; 24 streams so that many workgroups run side by side."""
    S = 24
    C = sum(2 if e == "cpe" else 1 for e in layout)
    eng = aacgpu.Engine(aacgpu.INPUT_QUANT_I16, max_streams=S, max_channels=C)
    ov = np.zeros((S, C, 1024), np.float32)
    for batch in range(2):
        wl = aacgpu_workload.make_batch(n_streams=S, n_frames=T, layout=layout, mix=True, intensity=True, seed=900 + batch, frame_base=batch * T)
        ref = oracle.decode_batch(wl["units"], wl["q"], wl["meta"], wl["n_pcm"], ov)
        pcm = eng.decode_batch(wl["units"], wl["q"], wl["meta"], wl["n_pcm"])
        assert rms(pcm, ref) < RMS_TOL
        got = overlaps(eng, S, C)
        assert np.abs(got - ov).max() <= 1e-5 * max(1.0, float(np.abs(ov).max()))
    eng.close()


# ---- stand-alone known-answer tests of the transform stage (aacg_debug_transform) ---------------------------
def _unreorder(y, N):
    """Invert mdct.js:90-114: from the N IMDCT-order outputs back to the N/4 complex values (re, im) behind them (every value
    appears twice in the output; both copies must agree)."""
    n8, n4, n2 = N // 8, N // 4, N // 2
    re, im, re2, im2 = np.zeros(n4), np.zeros(n4), np.zeros(n4), np.zeros(n4)
    k = np.arange(n8)
    im[n8 + k] = y[2 * k];                 re[n8 - 1 - k] = -y[2 * k + 1]
    re2[k] = y[n4 + 2 * k];                im2[n4 - 1 - k] = -y[n4 + 2 * k + 1]
    re[n8 + k] = y[n2 + 2 * k];            im[n8 - 1 - k] = -y[n2 + 2 * k + 1]
    im2[k] = -y[3 * n4 + 2 * k];           re2[n4 - 1 - k] = y[3 * n4 + 2 * k + 1]
    tol = 1e-5 * max(1.0, float(np.abs(y).max()))
    assert np.allclose(re, re2, rtol=0, atol=tol) and np.allclose(im, im2, rtol=0, atol=tol)
    return re, im


def _rel(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2)))


VM = pytest.mark.parametrize("vm", [False, True], ids=["f32-seam", "int16-seam"])


@VM
def test_imdct_2048_kat(golden, vm):
    """mdct.js:62-115, N = 2048: the kernels' long-window IMDCT alone against the reference's MDCT.process vectors.
    Tolerance 5e-6 of the output RMS (the reference's own float32 twiddle recurrence is 1.3e-6 from exact).  Both variants of
    the stage: the f32 seam's (mirror-lane exchange as ds_bpermute) and the int16 seam's (columns dealt out by long_col, DPP)."""
    for v in range(4):
        got = aacgpu.debug_transform(golden["imdct2048.in"][v], vm=vm)
        assert _rel(got, golden["imdct2048.out"][v]) < 5e-6


@VM
def test_imdct_256_kat(golden, vm):
    """N = 256: four reference vectors as windows 0, 2, 4, 6 of one EIGHT_SHORT spectrum (odd windows zero: the window
    overlap then leaves every IMDCT's 256 outputs in the clear)."""
    x = np.zeros((8, 128), np.float32)
    x[0::2] = golden["imdct256.in"]
    s = aacgpu.debug_transform(x.ravel(), is_short=True, vm=vm)[:1024].reshape(8, 128)
    for v in range(4):
        y = np.concatenate([s[2 * v], s[2 * v + 1]])
        assert _rel(y, golden["imdct256.out"][v]) < 5e-6


@VM
def test_fft_512_kat(golden, vm):
    """fft.js:105-192, 512 points, inverse, unscaled: with the MDCT rotations replaced by the identity the long-window stage is
    the FFT of z[k] = X[1023 - 2k] + i X[2k]; the reference's FFT.process vectors are fed through that map."""
    for v in range(3):
        z = golden["fft512.in"][v].astype(np.float32)                   # [512][re, im]
        X = np.zeros(1024, np.float32)
        k = np.arange(512)
        X[1023 - 2 * k] = z[:, 0]
        X[2 * k] = z[:, 1]
        re, im = _unreorder(aacgpu.debug_transform(X, identity_rotation=True, vm=vm).astype(np.float64), 2048)
        want = golden["fft512.out"][v].astype(np.float64)
        assert _rel(np.stack([re, im], 1), want) < 5e-6


@VM
def test_fft_64_kat(golden, vm):
    """64 points: three reference vectors as windows 0, 2, 4 of an EIGHT_SHORT spectrum, identity rotations."""
    x = np.zeros((8, 128), np.float32)
    k = np.arange(64)
    for v in range(3):
        z = golden["fft64.in"][v].astype(np.float32)
        x[2 * v, 127 - 2 * k] = z[:, 0]
        x[2 * v, 2 * k] = z[:, 1]
    s = aacgpu.debug_transform(x.ravel(), is_short=True, identity_rotation=True, vm=vm)[:1024].reshape(8, 128).astype(np.float64)
    for v in range(3):
        re, im = _unreorder(np.concatenate([s[2 * v], s[2 * v + 1]]), 256)
        assert _rel(np.stack([re, im], 1), golden["fft64.out"][v].astype(np.float64)) < 5e-6


def test_distance_from_the_reference_is_the_roots_recurrence(oracle, golden):
    """SURVEY.md 9.2 / DESIGN.md 2: the engine uses correctly rounded FFT twiddles, the reference a float32 recurrence that
    drifts (fft.js:59-103).  Against the oracle as it follows the reference the kernels' IMDCT is ~1e-6 off; against the same
    oracle with exact roots (orc_set_fft_roots) it is several times closer: the distance is the reference's table, not the
    engine's arithmetic."""
    for vm in (False, True):
        for v in range(2):
            x = golden["imdct2048.in"][v]
            got = aacgpu.debug_transform(x, vm=vm)
            to_reference = _rel(got, oracle.imdct(x))
            with oracle.exact_fft_roots():
                to_exact = _rel(got, oracle.imdct(x))
            assert to_reference < 5e-6 and to_exact < 4e-7 and to_exact < 0.5 * to_reference, (vm, v, to_reference, to_exact)


def _pcm16(ref):
    return np.clip(np.rint(ref.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)


@pytest.mark.parametrize("layout,T,inp", [(("cpe",), 40, "q"), (("cpe",), 16, "spec"), (("cpe", "cpe", "cpe", "sce"), 20, "q"), (("sce",), 18, "q")])
def test_int16_output(oracle, layout, T, inp):
    """AACG_OUTPUT_I16 engines (aacg_imdct_run_*_i16): the same samples as int16, round to nearest, saturating; every path of
    the epilogue (stereo fast path, multichannel in-place path, single channels, later runs of long chains).  Against the
    oracle's float PCM rounded the same way: at most one step off, and only for samples within the float error of a rounding
    boundary."""
    S = 12
    C = sum(2 if e == "cpe" else 1 for e in layout)
    wl = aacgpu_workload.make_batch(n_streams=S, n_frames=T, layout=layout, mix=True, intensity=True, seed=31)
    ov = np.zeros((S, C, 1024), np.float32)
    ref, spec = oracle.decode_batch(wl["units"], wl["q"], wl["meta"], wl["n_pcm"], ov, want_spec=True)
    want = _pcm16(ref)
    kind = aacgpu.INPUT_QUANT_I16 if inp == "q" else aacgpu.INPUT_SPEC_F32
    eng = aacgpu.Engine(kind, max_streams=S, max_channels=C, output_kind=aacgpu.OUTPUT_I16)
    got = eng.decode_batch(wl["units"], wl["q"] if inp == "q" else spec, wl["meta"] if inp == "q" else None, wl["n_pcm"])
    assert got.dtype == np.int16
    d = got.astype(np.int32) - want
    assert np.abs(d).max() <= 1 and np.count_nonzero(d) <= 1e-2 * d.size, (np.abs(d).max(), np.count_nonzero(d))
    assert np.abs(want).max() > 1000
    sat = np.full((1, 1024), 8190, np.int16)                     # far beyond full scale: saturates instead of wrapping
    u1 = wl["units"][:1].copy()
    u1["stream"] = 0; u1["pcm_offset"] = 0; u1["coef_offset"] = 0; u1["meta_offset"] = 0
    if inp == "q" and layout == ("cpe",):
        m = wl["meta"][:2].copy()
        m[:] = (1 << 12) | 300                                    # sf index 300: 2^25
        big = eng.decode_batch(u1, np.repeat(sat, 2, 0), m, 2048)
        assert big.max() == 32767 and big.min() == -32768
    eng.close()


# ---- chains longer than a run: the run-to-run rendezvous of the 16-wave kernels (aacg_imdct_run_*_rv) ------------------------
@pytest.mark.parametrize("layout,S,T,seam", [(("cpe",), 300, 40, "q"), (("cpe",), 64, 128, "q"), (("cpe",), 40, 33, "f"), (("sce",), 40, 50, "q"),
                                             (("cpe", "cpe", "cpe", "sce"), 24, 20, "q")])
def test_rendezvous_between_runs_equals_recomputed_frames(oracle, layout, S, T, seam):
    """Plain batches with chains longer than 16 frames: the engine's route (every run 16 frames, tails handed over through a
    rendezvous cell; aacg_imdct_run_*_rv) against the old one (later runs recompute the frame before them: _dd / predecessor
    waves; forced with AACG_DEBUG_ROUTE_RECOMPUTE) — the same bits, PCM and overlap state, over two chained batches, with more
    workgroups than the chip holds at once (so that both sides of a rendezvous arrive first somewhere) — and the oracle's values."""
    _rendezvous_against_recompute(oracle, layout, S, T, seam, "f32")


@pytest.mark.parametrize("layout,S,T,seam", [(("cpe",), 300, 48, "q"), (("cpe", "cpe", "cpe", "sce"), 24, 32, "f")])
def test_rendezvous_between_runs_equals_recomputed_frames_int16(oracle, layout, S, T, seam):
    """The same with int16 PCM: _rv_i16 (_rv_i16_nt) against _dd_i16 (a later run of 16 frames: T >= 32, not 33..47), the same
    bits; and the oracle's PCM rounded, at most one step off."""
    _rendezvous_against_recompute(oracle, layout, S, T, seam, "i16")


def _rendezvous_against_recompute(oracle, layout, S, T, seam, out):
    wl0 = aacgpu_workload.make_batch(n_streams=S, n_frames=T, layout=layout, mix=True, intensity=True, seed=5200)
    C = wl0["C"]
    kind = aacgpu.INPUT_QUANT_I16 if seam == "q" else aacgpu.INPUT_SPEC_F32
    i16 = out == "i16"
    outs, states, routes = [], [], []
    for route in (0, aacgpu.DEBUG_ROUTE_RECOMPUTE):                  # the engine's route, and the old one
        eng = aacgpu.Engine(kind, max_streams=S, max_channels=C, output_kind=aacgpu.OUTPUT_I16 if i16 else aacgpu.OUTPUT_F32)
        eng.debug_set_route(route)
        got = []
        for batch in range(2):
            wl = aacgpu_workload.make_batch(n_streams=S, n_frames=T, layout=layout, mix=True, intensity=True, seed=5200 + batch, frame_base=batch * T)
            coeffs, meta = wl["q"], wl["meta"]
            if seam == "f":
                _, spec = oracle.decode_batch(wl["units"], wl["q"], wl["meta"], wl["n_pcm"], np.zeros((S, C, 1024), np.float32), want_spec=True)
                coeffs, meta = spec.astype(np.float32), None
            if batch == 0:
                plan = eng.plan(wl["units"])
                routes.append(eng.plan_kernels(plan))
                plan.destroy()
            got.append(eng.decode_batch(wl["units"], coeffs, meta, wl["n_pcm"]))
        outs.append(np.concatenate(got))
        states.append(overlaps(eng, S, C))
        eng.close()
    # (multichannel frames: the rendezvous kernels' variant with non-temporal loads of the spectra)
    assert routes[0].endswith(("_rv" + ("_i16" if i16 else "")) + ("_nt" if C > 2 else "")) and "_rv" not in routes[1]
    if i16:
        assert routes[1].endswith("_dd_i16")
    assert outs[0].dtype == (np.int16 if i16 else np.float32)
    assert np.array_equal(outs[0].view(np.uint16 if i16 else np.uint32), outs[1].view(np.uint16 if i16 else np.uint32))
    assert np.array_equal(states[0].view(np.uint32), states[1].view(np.uint32))
    if i16:
        ov = np.zeros((S, C, 1024), np.float32)
        for batch in range(2):
            wl = aacgpu_workload.make_batch(n_streams=S, n_frames=T, layout=layout, mix=True, intensity=True, seed=5200 + batch, frame_base=batch * T)
            ref = oracle.decode_batch(wl["units"], wl["q"], wl["meta"], wl["n_pcm"], ov)
            d = outs[0][batch * wl["n_pcm"]:(batch + 1) * wl["n_pcm"]].astype(np.int32) - _pcm16(ref)
            assert np.abs(d).max() <= 1 and np.count_nonzero(d) <= 1e-2 * d.size
        assert np.abs(states[0] - ov).max() <= 1e-5 * max(1.0, float(np.abs(ov).max()))
    elif S * T <= 12000:
        ov = np.zeros((S, C, 1024), np.float32)
        ref = []
        for batch in range(2):
            wl = aacgpu_workload.make_batch(n_streams=S, n_frames=T, layout=layout, mix=True, intensity=True, seed=5200 + batch, frame_base=batch * T)
            ref.append(oracle.decode_batch(wl["units"], wl["q"], wl["meta"], wl["n_pcm"], ov))
        assert rms(outs[0], np.concatenate(ref)) < RMS_TOL
        assert np.abs(states[0] - ov).max() <= 1e-5 * max(1.0, float(np.abs(ov).max()))


# ---- consecutive launches of one plan overlapped: aacg_decode_pipelined -------------------------------------------------------
def _device_batches(torch, base, n, seam, oracle, seed):
    """n consecutive batches of the same streams on the device (the structure of batch 0, new coefficients): inputs, outputs"""
    rng = np.random.default_rng(seed)
    ins, host = [], []
    for j in range(n):
        q = base["q"] if j == 0 else (np.roll(base["q"], 131 * j, axis=0) * rng.choice([-1, 1])).astype(np.int16)
        if seam == "f":
            h = (np.sign(q) * np.abs(q.astype(np.float32)) ** (4.0 / 3.0) * 2.0 ** 4).astype(np.float32)
        else:
            h = np.ascontiguousarray(q)
        host.append(h)
        ins.append(torch.from_numpy(h).cuda())
    return ins, host


@pytest.mark.parametrize("layout,S,T,n,seam,mix", [(("cpe",), 256, 16, 72, "q", False), (("cpe",), 256, 16, 64, "f", True), (("cpe",), 300, 5, 64, "q", True),
                                                    (("cpe",), 32, 128, 64, "q", True), (("cpe", "cpe", "cpe", "sce"), 64, 16, 64, "q", True),
                                                    (("sce",), 700, 3, 64, "q", True)])
def test_pipelined_launches_equal_the_serialised_route_bit_for_bit(oracle, layout, S, T, n, seam, mix):
    """>= 64 back-to-back launches of ONE plan through aacg_decode_pipelined (the engine's internal streams taken in turn; the chains of
    neighbouring launches meet in cross-launch cells, nobody waits) against the same launches through aacg_decode_device on one
    stream (the plain kernels, every launch behind the one before it): np.array_equal on uint32 views, every launch's PCM and
    the final overlap state — BASELINE config 2 / 3 / 4 / 5 shapes, a grid larger than the chip (both arrival orders occur),
    both seams; the first launches against the oracle.  The routes taken are asserted."""
    torch = _torch()
    base = aacgpu_workload.make_batch(n_streams=S, n_frames=T, layout=layout, mix=mix, intensity=mix, seed=7300)
    C = base["C"]
    kind = aacgpu.INPUT_QUANT_I16 if seam == "q" else aacgpu.INPUT_SPEC_F32
    ins, host = _device_batches(torch, base, n, seam, oracle, 7)
    d_meta = torch.from_numpy(base["meta"].view(np.int16)).cuda() if seam == "q" else None
    mp = d_meta.data_ptr() if d_meta is not None else None
    results = []
    for pipelined in (False, True):
        eng = aacgpu.Engine(kind, max_streams=S, max_channels=C)
        plan = eng.plan(base["units"])
        name = eng.plan_kernels(plan, pipelined=pipelined)
        wide = "_nt" if C > 2 else ""
        if pipelined:
            assert name == "aacg_imdct_run_%s_rv%s" % ("quant" if seam == "q" else "f32", wide)
        else:
            assert name == "aacg_imdct_run_%s%s%s" % ("quant" if seam == "q" else "f32", "_rv" if T > 16 else "", wide)
        outs = [torch.full((base["n_pcm"],), float("nan"), dtype=torch.float32, device="cuda") for _ in range(n)]
        torch.cuda.synchronize()
        for j in range(n):
            if pipelined:
                eng.decode_pipelined(plan, ins[j].data_ptr(), mp, outs[j].data_ptr())
            else:
                eng.decode_device(plan, ins[j].data_ptr(), mp, outs[j].data_ptr(), 0)
        eng.synchronize()
        torch.cuda.synchronize()
        if pipelined:
            assert eng.pipeline_chained() == n - 1                   # every launch but the first continued the one before it
        results.append(([o.cpu().numpy() for o in outs], overlaps(eng, S, C)))
        plan.destroy()
        eng.close()
    (serial, s_state), (piped, p_state) = results
    for j in range(n):
        assert not np.isnan(piped[j]).any(), j
        assert np.array_equal(piped[j].view(np.uint32), serial[j].view(np.uint32)), "launch %d differs from the serialised route" % j
    assert np.array_equal(p_state.view(np.uint32), s_state.view(np.uint32))
    if seam == "q":                                                  # ... and the serialised route is the oracle's, on the first launches
        ov = np.zeros((S, C, 1024), np.float32)
        for j in range(2 if S * T > 3000 else 4):
            assert rms(serial[j], oracle.decode_batch(base["units"], host[j], base["meta"], base["n_pcm"], ov)) < RMS_TOL


@pytest.mark.parametrize("layout,S,T,seam", [(("cpe",), 24, 7, "q"), (("cpe", "sce"), 20, 19, "q"), (("cpe",), 16, 5, "f")])
def test_pipelined_launches_every_launch_against_the_oracle(oracle, layout, S, T, seam):
    """The soak's pipelined leg as a test the driver runs: 208 back-to-back launches of ONE plan through
    aacg_decode_pipelined — every window sequence, intensity, chains shorter and longer than a run (19 frames: the run-to-run AND
    the launch-to-launch rendezvous), new coefficients every launch — and EVERY launch's PCM against the oracle, which carries
    the same streams' overlap state from launch to launch; the final overlap state too.  A fault common to the pipelined and
    the serialised route behind the first launches would show here and nowhere else in the suite."""
    torch = _torch()
    n = 208
    base = aacgpu_workload.make_batch(n_streams=S, n_frames=T, layout=layout, mix=True, intensity=True, seed=7700)
    C = base["C"]
    kind = aacgpu.INPUT_QUANT_I16 if seam == "q" else aacgpu.INPUT_SPEC_F32
    ins, host = _device_batches(torch, base, n, seam, oracle, 11)
    d_meta = torch.from_numpy(base["meta"].view(np.int16)).cuda() if seam == "q" else None
    mp = d_meta.data_ptr() if d_meta is not None else None
    eng = aacgpu.Engine(kind, max_streams=S, max_channels=C)
    plan = eng.plan(base["units"])
    outs = [torch.full((base["n_pcm"],), float("nan"), dtype=torch.float32, device="cuda") for _ in range(n)]
    torch.cuda.synchronize()
    for j in range(n):
        eng.decode_pipelined(plan, ins[j].data_ptr(), mp, outs[j].data_ptr())
    eng.synchronize()
    assert eng.pipeline_chained() == n - 1
    ov = np.zeros((S, C, 1024), np.float32)
    worst = 0.0
    for j in range(n):
        got = outs[j].cpu().numpy()
        assert not np.isnan(got).any(), j
        worst = max(worst, rms(got, oracle.decode_batch(base["units"], host[j], base["meta"] if seam == "q" else None, base["n_pcm"], ov)))
    assert worst < RMS_TOL
    state = overlaps(eng, S, C)
    assert np.allclose(state, ov, rtol=0, atol=1e-4 * max(1.0, float(np.abs(ov).max())))
    plan.destroy()
    eng.close()


@pytest.mark.parametrize("layout,S,T", [(("cpe",), 256, 16), (("cpe", "cpe", "cpe", "sce"), 40, 24)])
def test_pipelined_int16_pcm_equals_the_serialised_route(oracle, layout, S, T):
    """AACG_OUTPUT_I16 engines through the pipeline (aacg_imdct_run_*_rv_i16): 64 overlapped launches against the same launches
    one behind the other — the same int16 samples and the same overlap state; the first launch against the oracle's PCM rounded
    the same way."""
    torch = _torch()
    n = 64
    base = aacgpu_workload.make_batch(n_streams=S, n_frames=T, layout=layout, mix=True, intensity=True, seed=7500)
    C = base["C"]
    ins, host = _device_batches(torch, base, n, "q", oracle, 9)
    d_meta = torch.from_numpy(base["meta"].view(np.int16)).cuda()
    results = []
    for pipelined in (False, True):
        eng = aacgpu.Engine(aacgpu.INPUT_QUANT_I16, max_streams=S, max_channels=C, output_kind=aacgpu.OUTPUT_I16)
        plan = eng.plan(base["units"])
        name = eng.plan_kernels(plan, pipelined=pipelined)
        wide = "_nt" if C > 2 else ""
        assert name == ("aacg_imdct_run_quant_rv_i16" + wide if pipelined or T > 16 else "aacg_imdct_run_quant_i16" + wide)
        outs = [torch.full((base["n_pcm"],), -1, dtype=torch.int16, device="cuda") for _ in range(n)]
        torch.cuda.synchronize()
        for j in range(n):
            if pipelined:
                eng.decode_pipelined(plan, ins[j].data_ptr(), d_meta.data_ptr(), outs[j].data_ptr())
            else:
                eng.decode_device(plan, ins[j].data_ptr(), d_meta.data_ptr(), outs[j].data_ptr(), 0)
        eng.synchronize()
        torch.cuda.synchronize()
        if pipelined:
            assert eng.pipeline_chained() == n - 1
        results.append(([o.cpu().numpy() for o in outs], overlaps(eng, S, C)))
        plan.destroy()
        eng.close()
    (serial, s_state), (piped, p_state) = results
    for j in range(n):
        assert np.array_equal(piped[j], serial[j]), "launch %d differs from the serialised route" % j
    assert np.array_equal(p_state.view(np.uint32), s_state.view(np.uint32))
    ov = np.zeros((S, C, 1024), np.float32)
    d = serial[0].astype(np.int32) - _pcm16(oracle.decode_batch(base["units"], host[0], base["meta"], base["n_pcm"], ov))
    assert np.abs(d).max() <= 1 and np.count_nonzero(d) <= 1e-2 * d.size


def test_pipelined_launches_mixed_with_everything_else(oracle):
    """The pipeline next to the other entry points on the same streams — aacg_decode_device of the same plan, another plan, the
    host-buffer path, aacg_get_overlap, a fork from and a join onto a caller's stream: mixing costs the overlap, never the
    result.  One engine does the sequence mixed, one does it serially."""
    torch = _torch()
    S, T = 64, 16
    base = aacgpu_workload.make_batch(n_streams=S, n_frames=T, mix=True, intensity=True, seed=7400)
    n = 12
    ins, host = _device_batches(torch, base, n, "q", oracle, 8)
    d_meta = torch.from_numpy(base["meta"].view(np.int16)).cuda()
    mp = d_meta.data_ptr()
    side = torch.cuda.Stream()

    def run(mixed):
        eng = aacgpu.Engine(aacgpu.INPUT_QUANT_I16, max_streams=S, max_channels=2)
        plan, plan_b = eng.plan(base["units"]), None
        outs = [torch.full((base["n_pcm"],), float("nan"), dtype=torch.float32, device="cuda") for _ in range(n)]
        got = [None] * n
        torch.cuda.synchronize()
        for j in range(n):
            how = ["p", "p", "p", "d", "p", "b", "p", "p", "h", "p", "s", "p"][j] if mixed else "d"
            if how == "p":
                eng.decode_pipelined(plan, ins[j].data_ptr(), mp, outs[j].data_ptr())
            elif how == "d":                                        # the same plan, serial, on the engine's stream
                eng.decode_device(plan, ins[j].data_ptr(), mp, outs[j].data_ptr(), 0)
            elif how == "b":                                        # another plan for the same streams (made now: it starts from the current state)
                plan_b = eng.plan(base["units"])
                eng.decode_pipelined(plan_b, ins[j].data_ptr(), mp, outs[j].data_ptr())
                plan.destroy()
                plan = plan_b
            elif how == "h":                                        # the host-buffer path
                got[j] = eng.decode_batch(base["units"], host[j], base["meta"], base["n_pcm"])
                plan.destroy()
                plan = eng.plan(base["units"])                      # (a plan is stale once something else has advanced its streams)
            elif how == "s":                                        # input produced on a caller's stream, output consumed there
                with torch.cuda.stream(side):
                    tmp = ins[j].clone()
                    eng.pipeline_fork(side.cuda_stream)
                    eng.decode_pipelined(plan, tmp.data_ptr(), mp, outs[j].data_ptr())
                    eng.pipeline_join(side.cuda_stream)
                    got[j] = outs[j].clone()
                side.synchronize()
                got[j] = got[j].cpu().numpy()
            if mixed and j == 6:
                eng.get_overlap(3, 1)                                # host reads the state in the middle: a full stop, nothing more
        eng.synchronize()
        torch.cuda.synchronize()
        state = overlaps(eng, S, 2)
        res = [got[j] if got[j] is not None else outs[j].cpu().numpy() for j in range(n)]
        plan.destroy()
        eng.close()
        return res, state

    (a, sa), (b, sb) = run(True), run(False)
    for j in range(n):
        assert np.array_equal(a[j].view(np.uint32), b[j].view(np.uint32)), j
    assert np.array_equal(sa.view(np.uint32), sb.view(np.uint32))
