"""A resident batch's plan shaped on the device (aacg_plan_shape, aac.js_amd/csrc/aacg_plan_shape.h: shape_body) against what the host
planner makes of the same batch and the same rotation state (aacg_pipe::plan_list's units through aacg_plan_build), byte for byte:
unit records, the rendezvous cut of the run table in its XCD-aware block order, its link records, the refresh map, the counts.  The
kernel's source runs lane by lane on CPU threads (tests/emu/shape_emu.cpp with tests/emu/devport_emu.h) into poisoned buffers;
nothing may be written past the counts.  And the engine's own part without a device (aacg_shape.cpp): the per-shape figures against
aacg_plan_build's, the capacity check, and the rule which consecutive launches of a shaped plan may meet in the cross-launch cells."""
import ctypes as C

import numpy as np
import pytest

import emu_lib

MAX_CHANNELS = 8
OV_BUFFERS = 16
POISON = 0xA5
ERR_INVALID_ARG, ERR_CAPACITY = -1, -4
# tests/test_pipe_map_emu.py's pool: 5.1 and 7.1 as the reference deals them out, narrower ones, layouts wider than the channels, no layout
POOL = [[1, 2, 2, 1], [1, 2, 2, 2, 1], [2], [1], [2, 2, 2, 2], [1, 2, 2, 1, 2, 1], [2, 2, 2, 1, 1], [], [1, 1, 1, 1, 1, 1, 1, 1]]
STREAM_DTYPE = np.dtype([("frame_first", "<u4"), ("frames", "<u4"), ("unit_first", "<u4"), ("frame_units", "<u4"), ("slot", "<u4"),
                         ("run_first", "<u4"), ("link_first", "<u4"), ("rot", "<u4"), ("nch", "<u4"), ("reserved", "<u4", 3)])   # aacg_shape_stream
RUN_DTYPE = np.dtype([("pred_unit", "<i4"), ("n_units", "<i4"), ("is_last", "<i4"), ("wave_nch", "<u4"), ("ov0", "<i4", 2), ("rot", "<i4", 2),
                      ("unit", "<i4", 16), ("wave_unit", "<i4", 16), ("wave_coef", "<u4", 16), ("wave_meta", "<u4", 16)])       # aacg_run


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    L = emu_lib.build_driver("shape_emu", ["tests/emu/shape_emu.cpp", "aac.js_amd/csrc/aacg_shape.cpp", "aac.js_amd/csrc/aacg_plan.cpp",
                                           "aac.js_amd/csrc/aacg_tables.cpp"], tmp_path_factory.mktemp("shape_emu"))
    L.emu_plan_shape.argtypes = [C.c_void_p] * 5 + [C.c_uint32] * 5 + [C.c_void_p, C.c_uint32] + [C.c_uint32] * 3 + [C.c_void_p] * 13
    L.emu_shape_capacity.argtypes = [C.c_uint32] * 4 + [C.c_void_p]
    L.emu_shape_same.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    L.emu_shape_error.restype = C.c_char_p
    sizes = np.zeros(5, np.uint32)
    L.emu_shape_sizes(sizes.ctypes.data_as(C.c_void_p))
    assert list(sizes) == [80, RUN_DTYPE.itemsize, 16, 8, STREAM_DTYPE.itemsize] and RUN_DTYPE.itemsize == 288
    return L


def kept_of(nch, channels):
    """decoder.js:233 as the pipeline learns it: elements while they fit the output channels; one that would cross the end stops it"""
    chan = kept = 0
    for e, c in enumerate(nch):
        if chan + c <= channels and kept == e:
            kept = e + 1
        chan += c
    return kept


def capacity(lib, streams, frames, elems, channels):
    out = np.zeros(4, np.uint64)
    lib.emu_shape_capacity(streams, frames, elems, channels, out.ctypes.data)
    return [int(v) for v in out]


class Shaped:
    pass


def shape(lib, layouts, counts, channels, slots=None, n_slots=None, parity=None, blocks=None, limits=None):
    """layouts[s]: element channel counts of stream s's frames ([] = not learnt).  Runs both planners; -> their outputs, or the
    error code aacg_shape_plan refused the shape with."""
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
    n_slots = int(slots.max()) + 1 if n_slots is None else n_slots
    counts = np.asarray(counts, np.uint32)
    parity = np.zeros(n_slots * channels, np.uint8) if parity is None else np.asarray(parity, np.uint8)
    assert len(parity) == n_slots * channels
    lim = (S, int(counts.max()), U) if limits is None else limits
    cap_units, cap_runs, _, _ = capacity(lib, *lim, channels)
    cap_units, cap_runs = max(cap_units, int(counts.sum()) * U) + 3, max(cap_runs, S * U * 3) + 3      # room behind the counts: nothing may land there
    cap = np.array([cap_units, cap_runs], np.uint64)
    r = Shaped()
    r.host = [np.zeros(cap_units * 80, np.uint8), np.zeros(cap_runs * 288, np.uint8), np.zeros(cap_runs * 16, np.uint8), np.zeros(cap_units * 8, np.uint8)]
    r.dev = [np.full(len(b), POISON, np.uint8) for b in r.host]
    r.table = np.zeros(S, STREAM_DTYPE)
    r.figures = np.zeros(16, np.uint64)
    r.chains = [np.zeros((S * 8, 5), np.uint32), np.zeros((S * 8, 5), np.uint32)]
    blocks = min(S, 256) if blocks is None else blocks
    r.rc = lib.emu_plan_shape(n.ctypes.data, kept.ctypes.data, nch.ctypes.data, slots.ctypes.data, counts.ctypes.data, S, n_slots, channels, Cp, U,
                              parity.ctypes.data, blocks, *lim, cap.ctypes.data, *[b.ctypes.data for b in r.host], *[b.ctypes.data for b in r.dev],
                              r.table.ctypes.data, r.figures.ctypes.data, r.chains[0].ctypes.data, r.chains[1].ctypes.data)
    r.err = lib.emu_shape_error().decode()
    r.kept, r.counts, r.slots, r.nch, r.parity, r.channels = kept, counts, slots, nch, parity, channels
    return r


NAMES = ["n_units", "n_runs", "n_links", "zero_fill", "wide_frames", "long_chains", "pcm_floats", "n_chains"]


def check(lib, layouts, counts, channels, **kw):
    r = shape(lib, layouts, counts, channels, **kw)
    assert r.rc == 0, (r.rc, r.err)
    host, dev = dict(zip(NAMES, map(int, r.figures[:8]))), dict(zip(NAMES, map(int, r.figures[8:])))
    assert host == dev, "the engine's per-shape figures differ from aacg_plan_build's"
    nu, nr = host["n_units"], host["n_runs"]
    assert nu == int(sum(int(c) * int(k) for c, k in zip(r.counts, r.kept)))
    assert nr == int(sum(-(-int(c) // 16) * int(k) for c, k in zip(r.counts, r.kept)))
    assert host["n_links"] == int(sum((-(-int(c) // 16) - 1) * int(k) for c, k in zip(r.counts, r.kept)))
    assert (r.chains[0][:host["n_chains"]] == r.chains[1][:host["n_chains"]]).all(), "the chains a launch advances differ"
    for what, size, cnt, h, d in zip(["unit records", "runs_rv", "links_rv", "refresh map"], [80, 288, 16, 8], [nu, nr, nr, nu], r.host, r.dev):
        assert h[:cnt * size].tobytes() == d[:cnt * size].tobytes(), "the kernel's %s differ from the host planner's" % what
        assert (d[cnt * size:] == POISON).all(), "the kernel wrote %s past the plan's count" % what
    r.figs = host
    r.runs = r.host[1][:nr * 288].view(RUN_DTYPE)
    return r


def test_counts_around_a_run_and_the_xcd_order(lib):
    """counts 1, 15, 16, 17, 32, 33 and max_frames 40: chains of one, two and three runs (no link, one link, two links); slots
    out of order; a rotation state that differs between the channels of one stream"""
    counts = [1, 15, 16, 17, 32, 33, 40]
    assert [-(-c // 16) - 1 for c in counts] == [0, 0, 0, 1, 1, 2, 2]
    slots = [5, 2, 9, 0, 7, 3, 8]
    assert any(a > b for a, b in zip(slots, slots[1:])) and any(a < b for a, b in zip(slots, slots[1:]))
    rng = np.random.default_rng(1)
    parity = rng.integers(0, OV_BUFFERS, 10 * 2).astype(np.uint8)
    assert parity.any() and any(parity[2 * s] != parity[2 * s + 1] for s in slots)
    r = check(lib, [[]] * 7, counts, 2, slots=slots, n_slots=10, parity=parity, limits=(7, 40, 1))
    assert r.figs["n_runs"] == 13 and r.figs["n_runs"] % 8 and r.figs["n_runs"] > 8 and r.figs["long_chains"] and not r.figs["zero_fill"]
    # the rotation reached the run records: each chain's run reads the buffers the engine's state names
    for run in r.runs:
        slot = int(run["ov0"][0]) // (2 * OV_BUFFERS * 1024)
        assert [int(v) for v in run["rot"]] == [int(parity[2 * slot]), int(parity[2 * slot + 1])]
    # fewer runs than eight (one column each), exactly eight, and mono
    for cnts, want in [([17, 1, 40], 6), ([16] * 8, 8), ([33, 33, 17, 1], 9)]:
        for ch in (1, 2):
            rr = check(lib, [[]] * len(cnts), cnts, ch, parity=rng.integers(0, OV_BUFFERS, len(cnts) * ch), limits=(8, 40, 1))
            assert rr.figs["n_runs"] == want


@pytest.mark.parametrize("channels", [1, 2])
def test_mono_stereo_ragged(lib, channels):
    rng = np.random.default_rng(channels)
    for S, max_frames in [(1, 1), (3, 16), (37, 16), (256, 16), (256, 4), (61, 40)]:
        counts = rng.integers(1, max_frames + 1, S)
        slots = rng.permutation(S + 5)[:S]
        check(lib, [[]] * S, counts, channels, slots=slots, n_slots=S + 5, parity=rng.integers(0, OV_BUFFERS, (S + 5) * channels), limits=(S, max_frames, 1))


@pytest.mark.parametrize("channels", [6, 8])
def test_multichannel_layouts(lib, channels):
    """learnt layouts: among them layouts with kept < n, layouts that do not cover the output channels (zero_fill) and streams with
    no layout (no unit, no run)"""
    rng = np.random.default_rng(channels)
    keeps = [kept_of(l, channels) for l in POOL]
    assert any(k < len(l) for k, l in zip(keeps, POOL)) and any(k and sum(l[:k]) != channels for k, l in zip(keeps, POOL)) and [] in POOL
    for S, max_frames in [(1, 16), (9, 40), (64, 8), (256, 16), (40, 40)]:
        layouts = [POOL[int(i)] for i in rng.integers(0, len(POOL), S)]
        layouts[:min(S, len(POOL))] = POOL[:min(S, len(POOL))]
        counts = rng.integers(1, max_frames + 1, S)
        slots = rng.permutation(S + 3)[:S]
        r = check(lib, layouts, counts, channels, slots=slots, n_slots=S + 3, parity=rng.integers(0, OV_BUFFERS, (S + 3) * channels), limits=(S, max_frames, 8))
        if S >= len(POOL):
            assert r.figs["zero_fill"] and r.figs["wide_frames"]
    # a batch whose every layout covers the channels has nothing to clear; one whose first stream has no layout: plan unit 0 is another's
    full = [1, 2, 2, 1] if channels == 6 else [1, 2, 2, 2, 1]
    assert not check(lib, [full] * 5, [3, 17, 16, 40, 1], channels, parity=rng.integers(0, OV_BUFFERS, 5 * channels)).figs["zero_fill"]
    check(lib, [[], [2], full, []], [40, 7, 33, 2], channels, parity=rng.integers(0, OV_BUFFERS, 4 * channels))
    r = check(lib, [[], []], [4, 9], channels)
    assert r.figs["n_units"] == 0 and r.figs["n_runs"] == 0 and r.figs["pcm_floats"] == 0


def test_fewer_workgroups_than_streams(lib):
    rng = np.random.default_rng(7)
    check(lib, [[1, 2, 2, 1], [2, 2, 2, 2], []] * 30, rng.integers(1, 41, 90), 6, blocks=7, parity=rng.integers(0, OV_BUFFERS, 90 * 6))
    check(lib, [[]] * 256, rng.integers(1, 17, 256), 2, blocks=1, parity=rng.integers(0, OV_BUFFERS, 512))
    check(lib, [[]] * 256, rng.integers(1, 41, 256), 2, blocks=5, slots=rng.permutation(256), parity=rng.integers(0, OV_BUFFERS, 512))


def test_capacity(lib):
    """the most a batch within the limits can have, and a shape beyond it refused before anything is written"""
    assert capacity(lib, 256, 128, 1, 2) == [256 * 128, 256 * 8, 1792, 1]         # 1 792 links: DESIGN.md 7a's 88 MB for three sets
    assert capacity(lib, 256, 16, 1, 2)[:3] == [4096, 256, 0]                       # max_frames <= 16: no link, no cell
    assert capacity(lib, 64, 40, 8, 6) == [64 * 6 * 40, 64 * 6 * 3, 64 * 6 * 2, 6]  # at most one element per channel
    # the largest shape of the limits fits
    r = check(lib, [[1, 1, 1, 1, 1, 1]] * 4, [40] * 4, 6, limits=(4, 40, 8))
    assert [r.figs["n_units"], r.figs["n_runs"], r.figs["n_links"]] == capacity(lib, 4, 40, 8, 6)[:3]
    for counts, limits in [([40] * 4, (4, 39, 8)), ([8] * 5, (4, 40, 8))]:
        r = shape(lib, [[1, 2, 2, 1]] * len(counts), counts, 6, limits=limits)
        assert r.rc == ERR_CAPACITY and r.err
        assert all((d == POISON).all() for d in r.dev) and not r.table["frames"].any(), "a refused shape was written"
    r = shape(lib, [[]] * 3, [4, 4, 4], 2, slots=[0, 1, 5], n_slots=4)
    assert r.rc == ERR_CAPACITY
    r = shape(lib, [[]] * 3, [4, 4, 4], 2, slots=[2, 1, 2], n_slots=4)
    assert r.rc == ERR_INVALID_ARG and "twice" in r.err


def test_sequence_rule(lib):
    """identical table -> the launch continues its predecessor; anything else -> a new sequence"""
    def table(counts, slots, parity=None, layouts=None):
        return shape(lib, layouts or [[]] * len(counts), counts, 2 if layouts is None else 6, slots=slots, n_slots=8, parity=parity).table

    def same(a, b):
        return bool(lib.emu_shape_same(a.ctypes.data, len(a), b.ctypes.data, len(b)))

    a = table([3, 16, 7], [4, 1, 6])
    assert same(a, table([3, 16, 7], [4, 1, 6]))
    # the rotation moves on with every launch: a rotation word that differs alone does not break a sequence
    moved = table([3, 16, 7], [4, 1, 6], parity=(np.arange(16) % OV_BUFFERS).astype(np.uint8))
    assert (moved["rot"] != a["rot"]).any() and same(a, moved)
    # the same counts with two slots swapped is another shape, and so are other counts, fewer streams, another order
    swapped = table([3, 16, 7], [1, 4, 6])
    assert sorted(swapped["slot"]) == sorted(a["slot"]) and (swapped["frames"] == a["frames"]).all() and not same(a, swapped)
    assert not same(a, table([3, 16, 8], [4, 1, 6])) and not same(a, table([3, 16], [4, 1])) and not same(a, table([16, 3, 7], [1, 4, 6]))
    # another layout in the same slot with the same counts
    x, y = table([3, 5], [0, 1], layouts=[[1, 2, 2, 1], [2]]), table([3, 5], [0, 1], layouts=[[1, 2, 2, 1], [1]])
    assert (x["frames"] == y["frames"]).all() and not same(x, y) and same(x, x.copy())
