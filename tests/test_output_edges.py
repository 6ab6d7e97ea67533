"""Edges of the output: what a NaN sample becomes in int16 PCM, channels no unit covers (aacgpu.h: every frame block is fully
written, those channels zero) on every device path and through the resident pipeline, and the multichannel (_nt) kernels
against the plain ones on the same stream."""
import numpy as np
import pytest

import aacgpu as A
import aacgpu_workload as W
import parity

WIDE = ("cpe", "cpe", "cpe", "sce")


def _nan_batch():
    """test_extremes' batch (eight channels, escape magnitudes) with |q| = 8191 and -32768 in two frames: the reference's
    out-of-range IQ read makes those frames (and their successors through the overlap) NaN"""
    wl = W.make_batch(n_streams=1, n_frames=6, layout=("cpe", "cpe", "cpe", "cpe"), mix=True, seed=9)
    u, q, meta = wl["units"].copy(), wl["q"].copy(), wl["meta"].copy()
    q[::7, ::13] = 8190
    q[3::11, 5::17] = -8190
    q[int(u["coef_offset"][8]), 40] = 8191
    q[int(u["coef_offset"][12]) + 1, 7] = -32768
    return u, q, meta, wl["n_pcm"]


def _check_nan_pcm16(got, oracle):
    u, q, meta, n_pcm = _nan_batch()
    ref = oracle.decode_batch(u, q, meta, n_pcm, np.zeros((1, 8, 1024), np.float32))
    nan = np.isnan(ref)
    assert nan.any() and not nan.all()
    assert np.all(got[nan] == -32768)
    x = np.where(nan, 0.0, ref.astype(np.float64)) * 32768.0     # |PCM| reaches the hundreds here: elsewhere, saturation
    assert np.all(got[x > 32768.0 * 1.001] == 32767) and np.all(got[x < -32768.0 * 1.001] == -32768)


def test_nan_becomes_minus_32768_in_the_emulator(oracle):
    import emu_lib
    u, q, meta, n_pcm = _nan_batch()
    pool, par = emu_lib.new_pool(1, 8)
    got = emu_lib.Emu().decode(u, q, meta, n_pcm, pool, par, int16_out=True, poison=0x7F7F)
    _check_nan_pcm16(got, oracle)


@pytest.mark.gpu
def test_nan_becomes_minus_32768_on_the_device(oracle):
    u, q, meta, n_pcm = _nan_batch()
    eng = A.Engine(A.INPUT_QUANT_I16, 1, 8, output_kind=A.OUTPUT_I16)
    got = eng.decode_batch(u, q, meta, n_pcm, out=np.full(n_pcm, 0x7F7F, np.int16))
    eng.close()
    _check_nan_pcm16(got, oracle)


# ---- channels no unit covers ------------------------------------------------------------------------------------------------------
def _holes(layout, C, S=4, T=8):
    """a layout of fewer channels than the engine's frames: units with n_out_ch = C, the channels behind theirs uncovered"""
    wl = W.make_batch(n_streams=S, n_frames=T, layout=layout, mix=True, intensity=True, seed=6100 + C)
    u = wl["units"].copy()
    f = u["pcm_offset"] // (1024 * wl["C"])
    u["n_out_ch"] = C
    u["pcm_offset"] = f * 1024 * C
    return u, wl["q"], wl["meta"], S * T * 1024 * C, wl["C"]


@pytest.mark.gpu
@pytest.mark.parametrize("layout,C", [(("sce",), 2), (("cpe",), 6)])
@pytest.mark.parametrize("path", ["serial", "pipelined", "int16"])
def test_uncovered_channels_are_zero_on_the_device(oracle, layout, C, path):
    import torch
    units, q, meta, n_pcm, covered = _holes(layout, C)
    S = 4
    i16 = path == "int16"
    eng = A.Engine(A.INPUT_QUANT_I16, S, C, output_kind=A.OUTPUT_I16 if i16 else A.OUTPUT_F32)
    plan = eng.plan(units)
    d_q, d_m = torch.from_numpy(q).cuda(), torch.from_numpy(meta.view(np.int16)).cuda()
    if i16:
        d_pcm = torch.full((n_pcm,), 0x7F7F, dtype=torch.int16, device="cuda")
    else:
        d_pcm = torch.full((n_pcm,), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    if path == "pipelined":
        eng.decode_pipelined(plan, d_q.data_ptr(), d_m.data_ptr(), d_pcm.data_ptr())
    else:
        eng.decode_device(plan, d_q.data_ptr(), d_m.data_ptr(), d_pcm.data_ptr(), 0)
    eng.synchronize()
    torch.cuda.synchronize()
    got = d_pcm.cpu().numpy()
    plan.destroy()
    eng.close()
    frames = got.reshape(-1, 1024, C)
    assert np.all(frames[:, :, covered:] == 0)
    exact = parity.exact_reference(oracle, units, q, meta, n_pcm, np.zeros((S, C, 1024), np.float32))
    if i16:
        parity.assert_blocks_int16(got, exact, units)
    else:
        parity.assert_blocks(got, exact, units)


@pytest.mark.gpu
def test_resident_pipeline_clears_the_channels_a_stereo_stream_leaves():
    """ADVICE (round 6) item 1: a stereo stream through a channels = 6 pipeline, on the lane whose last batch was 5.1 PCM: channels
    0-1 are the reference's, channels 2-5 exactly zero (the plan of a layout with holes clears the lane's PCM buffer)"""
    from resident_kit import CASES, load
    case = {c["name"]: c for c in CASES}
    d51, t51, _ = load(case["surround48"])
    d2, t2, ref2 = load(case["stereo48"])
    F = 5
    data = np.concatenate([d51, d2])
    t2 = t2.copy()
    t2["byte_offset"] += len(d51)
    p = A.Pipeline(channels=6, max_streams=2, max_frames=F, sample_index=3, lanes=2)
    t_a = p.submit(data, t51[:F], [0], F)                    # lane 0: 5.1 PCM
    t_b = p.submit(data, t2[:F], [1], F)                     # lane 1: the stereo stream's first frames (its layout is learnt here)
    t_c = p.submit(data, t2[F:2 * F], [1], F)                # lane 0 again
    for t, ref, a in ((t_a, None, 0), (t_b, ref2, 0), (t_c, ref2, F)):
        pcm, res, refused = p.collect(t)
        assert refused == 0 and not res["status"].any()
        frames = pcm.reshape(F * 1024, 6)
        if ref is None:
            assert np.isfinite(pcm).all()
            continue
        assert np.all(frames[:, 2:] == 0)
        want = ref[a * 2048:(a + F) * 2048].astype(np.float64)        # (five frames may be a quiet stretch: per sample, not by rms)
        assert np.abs(frames[:, :2].ravel() - want).max() <= 1e-5 * max(1.0, 4.0 * float(np.sqrt(np.mean(want ** 2))))
    elems, kept = p.stream_layout(1)
    assert elems == [2] and kept == 1
    p.close()


# ---- the multichannel kernels against the plain ones -----------------------------------------------------------------------------
def _shift(units, pcm, blocks, cces=0):
    u = units.copy()
    u["pcm_offset"] += pcm
    u["coef_offset"] += blocks
    u["meta_offset"] += blocks
    u["stream"] += 1
    u["reserved1"] = np.where(u["flags"] & A.UNIT_CCE, u["reserved1"] + cces, u["reserved1"])
    return u


@pytest.mark.gpu
@pytest.mark.parametrize("family,T,out,cce", [("", 8, "f32", False), ("_rv", 24, "f32", False), ("_i16", 8, "i16", False),
                                              ("_rv_i16", 24, "i16", False), ("_cpl", 8, "f32", True)])
def test_multichannel_kernels_equal_the_plain_ones(family, T, out, cce):
    """one 7-channel stream decoded on its own (every unit in a wide frame: the _nt kernel) and padded with five stereo streams
    (fewer than half of the units wide: the plain kernel): that stream's PCM and overlap state, the same bits"""
    wide = W.make_batch(n_streams=1, n_frames=T, layout=WIDE, mix=True, intensity=True, seed=6300)
    pad = W.make_batch(n_streams=5, n_frames=T, layout=("cpe",), mix=True, intensity=True, seed=6301)
    if cce:
        uw, qw, mw, cw = W.add_cce(wide, points=(2,), seed=6302)
        up, qp, mp, cp = W.add_cce(pad, points=(2,), seed=6303)
    else:
        (uw, qw, mw), (up, qp, mp), cw, cp = (wide["units"], wide["q"], wide["meta"]), (pad["units"], pad["q"], pad["meta"]), None, None
    H = 8 if cce else 7
    both = np.concatenate([uw, _shift(up, wide["n_pcm"], len(qw), len(cw) if cce else 0)])
    qb, mb = np.concatenate([qw, qp]), np.concatenate([mw, mp])
    cb = np.concatenate([cw, cp]) if cce else None
    i16 = out == "i16"
    runs = []
    for units, q, meta, c, n_pcm in ((uw, qw, mw, cw, wide["n_pcm"]), (both, qb, mb, cb, wide["n_pcm"] + pad["n_pcm"])):
        eng = A.Engine(A.INPUT_QUANT_I16, 6, H, output_kind=A.OUTPUT_I16 if i16 else A.OUTPUT_F32, cce_mode=A.CCE_SPEC if cce else A.CCE_REFERENCE)
        plan = eng.plan(units, cce=c)
        route = eng.plan_kernels(plan)
        plan.destroy()
        pcm = eng.decode_batch(units, q, meta, n_pcm, cce=c) if cce else eng.decode_batch(units, q, meta, n_pcm)
        state = np.stack([eng.get_overlap(0, ch) for ch in range(H)])
        eng.close()
        runs.append((route, pcm[:wide["n_pcm"]], state))
    (r_nt, a, sa), (r_plain, b, sb) = runs
    assert r_nt.endswith("aacg_imdct_run_quant" + family + "_nt") and r_plain.endswith("aacg_imdct_run_quant" + family), (r_nt, r_plain)
    v = np.uint16 if i16 else np.uint32
    assert np.array_equal(a.view(v), b.view(v))
    assert np.array_equal(sa.view(np.uint32), sb.view(np.uint32))
