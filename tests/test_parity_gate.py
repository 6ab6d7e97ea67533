"""The per-block gate of tests/parity.py checked on the CPU: the exact-roots context reaches decode_batch, and planted faults in the
oracle's own PCM fail the gate — two of them faults the batch-wide rms() of test_gpu_parity.py lets through."""
import numpy as np
import pytest

import aacgpu_workload as W
import parity
from test_gpu_parity import rms


@pytest.fixture(scope="module")
def batch(oracle):
    """256 stereo streams x 16 frames (8192 blocks): the exact-roots PCM and the reference oracle's"""
    S, T = 256, 16
    wl = W.make_batch(n_streams=S, n_frames=T, mix=True, intensity=True, seed=4711)
    exact = parity.exact_reference(oracle, wl["units"], wl["q"], wl["meta"], wl["n_pcm"], np.zeros((S, 2, 1024), np.float32))
    ref = oracle.decode_batch(wl["units"], wl["q"], wl["meta"], wl["n_pcm"], np.zeros((S, 2, 1024), np.float32))
    return wl, exact, ref


def test_exact_roots_reach_decode_batch(oracle, batch):
    """orc_set_fft_roots swaps a process-global table: decode_batch inside the context differs from the reference's by the roots'
    distance (~1e-6 of the signal), and the table is back to the reference's after it"""
    wl, exact, ref = batch
    d = np.sqrt(np.mean((exact.astype(np.float64) - ref) ** 2)) / np.sqrt(np.mean(ref.astype(np.float64) ** 2))
    assert 1e-7 < d < 5e-6
    again = oracle.decode_batch(wl["units"], wl["q"], wl["meta"], wl["n_pcm"], np.zeros((256, 2, 1024), np.float32))
    assert np.array_equal(again.view(np.uint32), ref.view(np.uint32))


def test_the_gate_passes_the_exact_reference_itself(batch):
    wl, exact, _ = batch
    assert parity.assert_blocks(exact, exact, wl["units"]) == (0.0, 0.0)
    assert len(parity.block_index(wl["units"])[0]) == 8192


def _fails(got, exact, units):
    with pytest.raises(AssertionError):
        parity.assert_blocks(got, exact, units)


def test_one_block_off_by_1e4(batch):
    """(a) one block of the batch scaled by 1 + 1e-4: the batch rms() passes, the per-block gate does not"""
    wl, exact, ref = batch
    got = exact.copy()
    idx = parity.block_index(wl["units"])[0]
    got[idx[5000]] *= np.float32(1 + 1e-4)
    rms(got, ref)
    _fails(got, exact, wl["units"])


def test_systematic_error_of_3e6(batch):
    """(b) every sample scaled by 1 + 3e-6: the batch rms() passes, the per-block gate does not"""
    wl, exact, ref = batch
    got = (exact.astype(np.float64) * (1 + 3e-6)).astype(np.float32)
    rms(got, ref)
    _fails(got, exact, wl["units"])


def test_one_sample_moved(batch):
    """(c) one sample moved by 1e-3 of its block's peak"""
    wl, exact, _ = batch
    got = exact.copy()
    blk = parity.block_index(wl["units"])[0][1234]
    got[blk[700]] += np.float32(1e-3) * np.abs(exact[blk]).max()
    _fails(got, exact, wl["units"])


@pytest.mark.parametrize("fill", [np.nan, 0.0])
def test_one_channel_of_one_frame_not_written(batch, fill):
    """(d) one channel of one frame left as NaN (never written) or zero"""
    wl, exact, _ = batch
    got = exact.copy()
    got[parity.block_index(wl["units"])[0][4321]] = fill
    _fails(got, exact, wl["units"])
