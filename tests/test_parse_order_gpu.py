"""GPU: the lane-order pass in front of the parse kernel and of the span walk (aacg_parser.hip, order_and_clear), at the counts where
it takes another path: table order up to 64 frames, the fused aacg_parse_prepare launch up to 16 384, the three sorting kernels
beyond — and, for the frame parse, memsets and the three kernels at any count when a region to clear is no multiple of 16 bytes
(65 frames x 424 bytes of TNS records).  Inputs are copies of aacgpu_workload.tiny_frame (10 bytes: one SCE, eight coefficients);
what every frame or span must give is known in closed form, and the lane emulator gives the same bytes."""
import functools

import numpy as np
import pytest

import aacgpu
import aacgpu_workload
import emu_lib
import walk_cases

WANT_Q = [1, -2, 0, 3, -4, 4, 0, 0]
BAND_WORD = 0x50c8                       # book 5, scalefactor table index 200


@functools.lru_cache(maxsize=None)
def standin():
    return aacgpu_workload.standin_codebooks()


@functools.lru_cache(maxsize=None)
def batch_case(n):
    """Frame i: the tiny frame, then 8 (i % 5) + (i % 3) zero bytes — five length buckets, odd offsets."""
    tiny = aacgpu_workload.tiny_frame(*standin())[0]
    assert len(tiny) == 10
    i = np.arange(n)
    frames = np.zeros(n, aacgpu.PARSE_FRAME_DTYPE)
    frames["byte_length"] = 10 + 8 * (i % 5) + (i % 3)
    frames["byte_offset"] = np.concatenate([[0], np.cumsum(frames["byte_length"])[:-1]])
    data = np.zeros(int(frames["byte_length"].sum()), np.uint8)
    data[(frames["byte_offset"][:, None] + np.arange(10)[None, :]).reshape(-1)] = np.tile(tiny, n)
    return data, frames


@functools.lru_cache(maxsize=None)
def batch_reference(n, want_tns):
    data, frames = batch_case(n)
    return emu_lib.emu_parse(emu_lib.Emu(), 3, *standin(), data, frames, 1, 1, aacgpu.PARSE_REFERENCE_QUIRKS, want_tns)


@functools.lru_cache(maxsize=None)
def walk_case(n):
    """Span i: 1 + i % 3 tiny blocks back to back."""
    tiny = aacgpu_workload.tiny_frame(*aacgpu.standard_codebooks())[0]
    assert len(tiny) == 10
    blocks = 1 + np.arange(n) % 3
    spans = np.zeros(n, aacgpu.PARSE_FRAME_DTYPE)
    spans["byte_length"] = 10 * blocks
    spans["byte_offset"] = np.concatenate([[0], np.cumsum(spans["byte_length"])[:-1]])
    return np.tile(tiny, int(blocks.sum())), spans, blocks


@pytest.fixture(scope="module")
def walk_emu(tmp_path_factory):
    return walk_cases.build_emu(tmp_path_factory.mktemp("walk_emu"))


@pytest.mark.gpu
@pytest.mark.parametrize("n,want_tns", [(64, False), (65, False), (16384, False), (16385, False), (65, True)],
                         ids=["64-table-order", "65-fused", "16384-fused-limit", "16385-three-kernels", "65-tns-memsets"])
def test_gpu_parse_batch_at_every_lane_order_path(n, want_tns):
    data, frames = batch_case(n)
    p = aacgpu.Parser(*standin(), sample_index=3)
    got = p.parse_batch(data, frames, 1, 1, aacgpu.PARSE_REFERENCE_QUIRKS, want_tns)
    p.close()
    res = got["results"]
    assert not res["status"].any()
    assert (res["bits_used"] == 80).all()
    assert (got["q"][:, :8] == np.array(WANT_Q, np.int16)).all() and not got["q"][:, 8:].any()
    assert (got["meta"][:, :2] == BAND_WORD).all() and not got["meta"][:, 2:].any()      # the frame's two bands
    assert np.array_equal(got["units"]["coef_offset"], np.arange(n))
    want = batch_reference(n, want_tns)
    for key in ("results", "units", "q", "meta") + (("tns",) if want_tns else ()):
        assert got[key].tobytes() == want[key].tobytes(), key


@pytest.mark.gpu
@pytest.mark.parametrize("n", [64, 65, 16385], ids=["64-table-order", "65-fused", "16385-three-kernels"])
def test_gpu_walk_at_every_lane_order_path(walk_emu, n):
    data, spans, blocks = walk_case(n)
    p = aacgpu.Parser(sample_index=3)
    frames, res = p.walk(data, spans, 3)
    p.close()
    assert np.array_equal(res["n_frames"], blocks) and not res["status"].any()
    assert np.array_equal(res["bytes_consumed"], 10 * blocks)
    j = np.arange(3)[None, :]
    inside = j < blocks[:, None]
    assert np.array_equal(frames["byte_offset"], np.where(inside, spans["byte_offset"][:, None] + 10 * j, 0))
    assert np.array_equal(frames["byte_length"], np.where(inside, 10, 0))
    want_f, want_r = walk_cases.emu_walk(walk_emu, 3, data, spans, 3)
    assert frames.tobytes() == want_f.tobytes() and res.tobytes() == want_r.tobytes()
