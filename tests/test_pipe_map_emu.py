"""The resident batch's refresh map built on the device (aacg_pipe_map, aac.js_amd/csrc/aacg_pipe_map.h: map_body) against the map the
host planner lists for the same batch (aacg_pipe::plan_list), byte for byte: the kernel's source run lane by lane on CPU threads
(tests/emu/map_emu.cpp with tests/emu/devport_emu.h).  Ragged batches (each stream its own frame count, packed stream after
stream), 1 / 2 / 6 / 8-channel layouts, layouts whose last elements are dropped (kept < n), streams without a layout yet."""
import ctypes as C

import numpy as np
import pytest

import aacgpu
import emu_lib

MAP_DTYPE = np.dtype([("parsed_index", "<u4"), ("frame_units", "<u4")])          # aacg_refresh_map
STREAM_DTYPE = np.dtype([("frame_first", "<u4"), ("frames", "<u4"), ("unit_first", "<u4"), ("frame_units", "<u4")])    # aacg_pipe_stream
MAX_CHANNELS = 8


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    L = emu_lib.build_driver("map_emu", ["tests/emu/map_emu.cpp"], tmp_path_factory.mktemp("map_emu"))
    L.emu_pipe_map.argtypes = [C.c_void_p] * 5 + [C.c_uint32] * 6 + [C.c_void_p] * 4
    return L


def kept_of(nch, channels):
    """decoder.js:233 as the pipeline learns it: elements while they fit the output channels; one that would cross the end stops it"""
    chan = kept = 0
    for e, c in enumerate(nch):
        if chan + c <= channels and kept == e:
            kept = e + 1
        chan += c
    return kept


def run(lib, layouts, counts, channels, blocks=None, slots=None):
    """layouts[s]: element channel counts of stream s's frames ([] = not learnt).  -> (host map, device map, units, table)"""
    S = len(counts)
    learn = channels > 2
    Cp, U = (MAX_CHANNELS, 8) if learn else (channels, 1)
    n, kept, nch = np.zeros(S, np.uint8), np.zeros(S, np.uint8), np.zeros((S, 8), np.uint8)
    for s, lay in enumerate(layouts):
        if not learn:
            lay = [channels]
        n[s], kept[s] = len(lay), kept_of(lay, channels)
        nch[s, :len(lay)] = lay
    slots = np.arange(S, dtype=np.uint32)[::-1].copy() if slots is None else np.asarray(slots, np.uint32)
    counts = np.asarray(counts, np.uint32)
    max_units = int(counts.sum()) * U
    host, dev = np.zeros(max_units, MAP_DTYPE), np.full(max_units, 0xFFFFFFFFFFFFFFFF, np.uint64).view(MAP_DTYPE)     # poisoned
    units, table = np.zeros(max_units, aacgpu.UNIT_DTYPE), np.zeros(S, STREAM_DTYPE)
    blocks = min(S, 256) if blocks is None else blocks
    got = lib.emu_pipe_map(n.ctypes.data, kept.ctypes.data, nch.ctypes.data, slots.ctypes.data, counts.ctypes.data, S, channels, Cp, U,
                           blocks, max_units, host.ctypes.data, dev.ctypes.data, units.ctypes.data, table.ctypes.data)
    assert got >= 0
    return host[:got], dev, units[:got], table, (n, kept, nch, slots, counts, Cp, U)


def listed(n, kept, nch, slots, counts, Cp, U, channels):
    """The map as the round-6 planner listed it, packed by prefix (frame f of stream s is frame first_s + f)"""
    out, first = [], 0
    for s in range(len(counts)):
        for f in range(int(counts[s])):
            for e in range(int(kept[s])):
                out.append(((first + f) * U + e, int(n[s]) | (int(kept[s]) << 8)))
        first += int(counts[s])
    return np.array(out, MAP_DTYPE) if out else np.zeros(0, MAP_DTYPE)


def check(lib, layouts, counts, channels, **kw):
    host, dev, units, table, (n, kept, nch, slots, cnt, Cp, U) = run(lib, layouts, counts, channels, **kw)
    nu = len(host)
    assert nu == int(sum(int(c) * int(k) for c, k in zip(cnt, kept)))
    assert host.tobytes() == dev[:nu].tobytes(), "the kernel's map differs from the host planner's"
    assert (dev[nu:].view(np.uint64) == 0xFFFFFFFFFFFFFFFF).all(), "the kernel wrote past the plan's units"
    assert host.tobytes() == listed(n, kept, nch, slots, cnt, Cp, U, channels).tobytes()
    # each map entry pairs with its unit: same frame, element e of it, the unit's coefficient block at the element's first channel
    if nu:
        frame = host["parsed_index"] // U
        assert (units["coef_offset"] // Cp == frame).all() and (units["pcm_offset"] == frame * 1024 * channels).all()
        first = np.concatenate([[0], np.cumsum(cnt)[:-1]])
        assert (table["frame_first"] == first).all() and (table["frames"] == cnt).all()


@pytest.mark.parametrize("channels", [1, 2])
def test_map_mono_stereo_ragged(lib, channels):
    rng = np.random.default_rng(channels)
    for S, max_frames in [(1, 1), (3, 16), (37, 16), (256, 16), (256, 4)]:
        counts = rng.integers(1, max_frames + 1, S)
        check(lib, [[]] * S, counts, channels)


@pytest.mark.parametrize("channels", [6, 8])
def test_map_multichannel_layouts(lib, channels):
    """learnt layouts: 5.1 and 7.1 as the reference deals them out, narrower ones, layouts wider than the channels (the elements
    beyond them dropped: kept < n), and streams with no layout yet (kept = 0: no units)"""
    pool = [[1, 2, 2, 1], [1, 2, 2, 2, 1], [2], [1], [2, 2, 2, 2], [1, 2, 2, 1, 2, 1], [2, 2, 2, 1, 1], [], [1, 1, 1, 1, 1, 1, 1, 1]]
    rng = np.random.default_rng(channels)
    for S, max_frames in [(1, 16), (9, 16), (64, 8), (256, 16)]:
        layouts = [pool[int(i)] for i in rng.integers(0, len(pool), S)]
        layouts[:min(S, len(pool))] = pool[:min(S, len(pool))]
        counts = rng.integers(1, max_frames + 1, S)
        check(lib, layouts, counts, channels)
    assert kept_of([2, 2, 2, 2], 6) == 3 and kept_of([1, 2, 2, 1, 2, 1], 6) == 4 and kept_of([1, 2, 2, 2, 1], 6) == 3


def test_map_rectangle_and_few_workgroups(lib):
    """every count equal (aacg_pipeline_submit's batch: first_s = s * F), and fewer workgroups than streams (each walks several)"""
    check(lib, [[1, 2, 2, 1]] * 40, [16] * 40, 6)
    check(lib, [[]] * 100, [7] * 100, 2)
    rng = np.random.default_rng(7)
    check(lib, [[1, 2, 2, 1], [2, 2, 2, 2], []] * 30, rng.integers(1, 17, 90), 6, blocks=7)
    check(lib, [[]] * 256, rng.integers(1, 17, 256), 2, blocks=1)
