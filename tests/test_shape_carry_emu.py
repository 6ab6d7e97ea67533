"""Each channel's window shape carried from frame to frame on the device (aacg_units_carry_shape, aac.js_amd/csrc/aacg_shape_carry.h:
carry_body) against a plain walk of the rule, byte for byte on the whole unit array: the kernel's source run lane by lane on CPU
threads (tests/emu/carry_emu.cpp with tests/emu/devport_emu.h).

The rule: the engine holds W[slot][c]; for each stream of a batch, its frames in order, each unit's channel k (output channel
c = channel + k) gets window_shape_prev = the stream's first frame ? W[slot][c] : window_shape of the frame before, and after the
batch W[slot][c] is the last frame's window_shape.  A silent frame's shape is 0; channels without a unit keep their W; nothing else
in a record changes."""
import ctypes as C

import numpy as np
import pytest

import aacgpu
import emu_lib

DEV_UNIT_DTYPE = np.dtype([("d", aacgpu.UNIT_DTYPE), ("gmap", "<u4", (2,)), ("cpl_first", "<u4"), ("cpl_n", "<u4")])      # aacg_dev_unit
MAP_DTYPE = np.dtype([("parsed_index", "<u4"), ("frame_units", "<u4")])                                                 # aacg_refresh_map


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    L = emu_lib.build_driver("carry_emu", ["tests/emu/carry_emu.cpp"], tmp_path_factory.mktemp("carry_emu"))
    L.emu_carry.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]
    L.emu_carry.restype = None
    L.emu_carry_entry.argtypes = [C.c_uint32] * 3
    L.emu_carry_entry.restype = C.c_uint32
    L.emu_carry_now.argtypes = [C.c_uint32]
    L.emu_carry_now.restype = C.c_uint32
    sizes = (C.c_uint32 * 3)()
    L.emu_carry_sizes(sizes)
    assert sizes[0] == DEV_UNIT_DTYPE.itemsize and sizes[1] == MAP_DTYPE.itemsize
    L.threads = int(sizes[2])
    return L


def kept_of(nch, channels):
    chan = kept = 0
    for e, c in enumerate(nch):
        if chan + c <= channels and kept == e:
            kept = e + 1
        chan += c
    return kept


def make_batch(rng, layouts, slots, counts, channels, silent=(), kept_word_zero=False):
    """The refreshed unit records of a batch as the resident route lists them (a stream's frames consecutive, a frame's kept units
    adjacent), every byte random where the refresh or the planner may put anything, window_shape 0 / 1, and the refresh map.
    silent: (stream position, frame) pairs whose units are what the refresh makes of a refused frame (ONLY_LONG, sine, nothing
    coded).  kept_word_zero: bits 8..15 of frame_units 0 where every element is kept (0 = all)."""
    recs, maps = [], []
    first = 0
    for s, (lay, slot, F) in enumerate(zip(layouts, slots, counts)):
        kept = kept_of(lay, channels)
        for f in range(F):
            chan = 0
            for e in range(kept):
                u = np.frombuffer(rng.integers(0, 256, DEV_UNIT_DTYPE.itemsize, dtype=np.uint8).tobytes(), DEV_UNIT_DTYPE).copy()
                u["d"]["stream"], u["d"]["channel"], u["d"]["n_ch"], u["d"]["n_out_ch"] = slot, chan, lay[e], channels
                u["d"]["pcm_offset"] = (first + f) * 1024 * channels
                u["d"]["ch"]["window_shape"] = rng.integers(0, 2, (1, 2))
                if (s, f) in silent:
                    u["d"]["flags"] = 0
                    u["d"]["ch"] = np.zeros((1, 2), u["d"]["ch"].dtype)
                    u["d"]["ch"]["group_count"] = 1
                    u["d"]["ch"]["group_len"][..., 0] = 1
                recs.append(u)
                word = len(lay) | ((0 if kept_word_zero and kept == len(lay) else kept) << 8)
                maps.append(((first + f) * 8 + e, word))
                chan += lay[e]
        first += F
    units = np.concatenate(recs) if recs else np.zeros(0, DEV_UNIT_DTYPE)
    units["d"]["ch"]["window_shape_prev"] = 0xA5          # poisoned: what the parser wrote there is not what a launch may rely on
    return units, np.array(maps, MAP_DTYPE) if maps else np.zeros(0, MAP_DTYPE)


def walk(units, W, channels):
    """The rule, unit by unit in listing order: (the records it leaves, the W it leaves).  W: [slots][channels] of 0 / 1."""
    out, W = units.copy(), W.copy()
    last = {}                                                # (slot, channel) -> shape of the frame before, within this batch
    for i in range(len(out)):
        d = out["d"][i]
        slot, chan = int(d["stream"]), int(d["channel"])
        for k in range(int(d["n_ch"])):
            c = chan + k
            out["d"]["ch"]["window_shape_prev"][i, k] = last.get((slot, c), W[slot, c])
            last[(slot, c)] = int(d["ch"]["window_shape"][k])
    for (slot, c), v in last.items():
        W[slot, c] = v
    return out, W


def entries_of(lib, W):
    return np.array([lib.emu_carry_entry(int(v), int(v), 0) for v in W.ravel()], np.uint32).reshape(W.shape)      # as the host writes them


def now_of(lib, E):
    return np.array([lib.emu_carry_now(int(v)) for v in E.ravel()], np.uint8).reshape(E.shape)


def launch(lib, units, maps, E, channels, serial, blocks=None, reverse=0):
    """one launch over a copy of the records (window_shape_prev poisoned: make_batch); E (the entries) is updated in place"""
    got = units.copy()
    assert (got["d"]["ch"]["window_shape_prev"] == 0xA5).all()
    n = len(got)
    blocks = max(1, (n + lib.threads - 1) // lib.threads) if blocks is None else blocks
    lib.emu_carry(got.ctypes.data, maps.ctypes.data, n, E.ctypes.data, E.shape[0], channels, serial, blocks, reverse)
    return got


def check(lib, rng, layouts, counts, channels, n_slots=None, W=None, slots=None, serial=1, **kw):
    S = len(counts)
    slots = list(rng.permutation(n_slots or S)[:S]) if slots is None else slots
    n_slots = n_slots or (max(slots) + 1)
    W = rng.integers(0, 2, (n_slots, channels)).astype(np.uint8) if W is None else W
    batch_kw = {k: kw.pop(k) for k in ("silent", "kept_word_zero") if k in kw}
    units, maps = make_batch(rng, layouts, slots, counts, channels, **batch_kw)
    want, W_after = walk(units, W, channels)
    E = entries_of(lib, W)
    got = launch(lib, units, maps, E, channels, serial, **kw)
    assert got.tobytes() == want.tobytes(), "the kernel's records differ from the rule's (or a byte outside window_shape_prev moved)"
    assert (now_of(lib, E) == W_after).all(), "the state the launch left differs from the rule's"
    # every byte but window_shape_prev of the channels a unit has is the input's
    mask = units.copy()
    mask["d"]["ch"]["window_shape_prev"] = got["d"]["ch"]["window_shape_prev"]
    assert mask.tobytes() == got.tobytes()
    for i in range(len(units)):
        for k in range(int(units["d"]["n_ch"][i]), 2):
            assert got["d"]["ch"]["window_shape_prev"][i, k] == 0xA5, "a channel the unit does not have was written"
    return units, maps, E, W, W_after


LAYOUTS = {1: [[1]], 2: [[2]], 6: [[1, 2, 2, 1], [2, 2, 2], [1, 2, 2, 2, 1], [2], [1]], 8: [[1, 2, 2, 2, 1], [2, 2, 2, 2], [1, 1, 1, 1, 1, 1, 1, 1], [1, 2, 2, 2, 2]]}


@pytest.mark.parametrize("channels", [1, 2, 6, 8])
def test_carry_layouts_ragged(lib, channels):
    """1 / 2 / 6 / 8 channels, layouts whose last element is dropped ([1, 2, 2, 2, 1] in 6 channels keeps 3; [1, 2, 2, 2, 2] in 8 keeps
    4), ragged counts with one-frame streams, non-zero incoming W, streams in any slot order"""
    rng = np.random.default_rng(100 + channels)
    pool = LAYOUTS[channels]
    for S, max_frames in [(1, 1), (1, 5), (3, 4), (9, 16), (40, 7)]:
        layouts = [pool[int(i)] for i in rng.integers(0, len(pool), S)]
        layouts[:min(S, len(pool))] = pool[:min(S, len(pool))]
        counts = [int(c) for c in rng.integers(1, max_frames + 1, S)]
        counts[0] = 1
        check(lib, rng, layouts, counts, channels, n_slots=S + 3)
    assert kept_of([1, 2, 2, 2, 1], 6) == 3 and kept_of([1, 2, 2, 2, 2], 8) == 4
    # W all ones coming in, and the map's "0 = all" form of the kept count
    check(lib, rng, [pool[0]] * 4, [3, 1, 2, 4], channels, W=np.ones((4, channels), np.uint8), kept_word_zero=True)


def test_carry_silent_frames(lib):
    """a silent unit (a refused frame) in the first, a middle and the last frame of a stream: its shape is 0, so the frame behind it
    starts from sine, and a silent last frame leaves W = 0 whatever came in"""
    rng = np.random.default_rng(5)
    for channels, lay in [(2, [2]), (6, [1, 2, 2, 1])]:
        silent = {(0, 0), (1, 2), (2, 4), (3, 0), (3, 1), (4, 0)}
        units, maps, E, W, W_after = check(lib, rng, [lay] * 5, [5, 5, 5, 3, 1], channels, W=np.ones((5, channels), np.uint8), slots=[4, 0, 3, 1, 2], silent=silent)
        assert (W_after[3] == 0).all() and (W_after[2] == 0).all()      # streams at positions 2 and 4 (slots 3 and 2) end silent
        got, _ = walk(units, W, channels)
        kept = len(lay)
        # position 0's second frame starts from sine on every channel (its first frame is silent), though W came in as 1
        assert (got["d"]["ch"]["window_shape_prev"][kept:2 * kept][np.arange(kept)[:, None], np.arange(2)[None, :]][got["d"]["n_ch"][kept:2 * kept, None] > np.arange(2)] == 0).all()


def test_carry_two_batches_absent_stream_keeps_state(lib):
    """two consecutive batches, the second without one of the streams: that stream's W stays, the others continue"""
    rng = np.random.default_rng(6)
    channels, lay = 6, [1, 2, 2, 1]
    W0 = rng.integers(0, 2, (4, channels)).astype(np.uint8)
    u1, m1 = make_batch(rng, [lay] * 4, [0, 1, 2, 3], [4, 2, 1, 3], channels)
    u2, m2 = make_batch(rng, [lay] * 3, [3, 0, 2], [2, 4, 1], channels)
    want1, W1 = walk(u1, W0, channels)
    want2, W2 = walk(u2, W1, channels)
    E = entries_of(lib, W0)
    assert launch(lib, u1, m1, E, channels, 7).tobytes() == want1.tobytes() and (now_of(lib, E) == W1).all()
    assert launch(lib, u2, m2, E, channels, 8).tobytes() == want2.tobytes() and (now_of(lib, E) == W2).all()
    assert (W2[1] == W1[1]).all()
    # a stream narrower than the engine's channels leaves the channels beyond it alone
    u3, m3 = make_batch(rng, [[2]], [1], [3], channels)
    want3, W3 = walk(u3, W2, channels)
    assert launch(lib, u3, m3, E, channels, 9).tobytes() == want3.tobytes() and (now_of(lib, E) == W3).all() and (W3[1, 2:] == W2[1, 2:]).all()


def test_carry_same_serial_twice_is_idempotent(lib):
    """the stale-plan retry: the same batch launched twice with one serial gives the same records and the same W — the second launch
    starts from what the first started from, not from what it left; a third with a NEW serial continues from what they left"""
    rng = np.random.default_rng(7)
    for channels, lay in [(2, [2]), (8, [1, 2, 2, 2, 1])]:
        W0 = rng.integers(0, 2, (6, channels)).astype(np.uint8)
        units, maps = make_batch(rng, [lay] * 5, [5, 0, 2, 1, 4], [1, 4, 2, 1, 3], channels)
        want, W1 = walk(units, W0, channels)
        E = entries_of(lib, W0)
        a = launch(lib, units, maps, E, channels, 3)
        E1 = E.copy()
        b = launch(lib, units, maps, E, channels, 3, reverse=1)
        assert a.tobytes() == want.tobytes() and b.tobytes() == want.tobytes() and (E == E1).all() and (now_of(lib, E) == W1).all()
        # other records for the second attempt (the retry refreshes again: same bytes in practice, but the rule is per serial)
        units2, maps2 = make_batch(rng, [lay] * 5, [5, 0, 2, 1, 4], [1, 4, 2, 1, 3], channels)
        want2, W1b = walk(units2, W0, channels)
        assert launch(lib, units2, maps2, E, channels, 3).tobytes() == want2.tobytes() and (now_of(lib, E) == W1b).all()
        want3, W2 = walk(units, W1b, channels)
        assert launch(lib, units, maps, E, channels, 4).tobytes() == want3.tobytes() and (now_of(lib, E) == W2).all()


def test_carry_256_streams_and_few_workgroups(lib):
    """256 streams, and fewer workgroups than units need (each lane walks several units), in either workgroup order"""
    rng = np.random.default_rng(8)
    counts = [int(c) for c in rng.integers(1, 17, 256)]
    check(lib, rng, [[2]] * 256, counts, 2, n_slots=256)
    check(lib, rng, [[1, 2, 2, 1], [2, 2, 2], [1]] * 30, [int(c) for c in rng.integers(1, 9, 90)], 6, n_slots=100, blocks=2)
    check(lib, rng, [[1, 2, 2, 1], [2, 2, 2], [1]] * 30, [int(c) for c in rng.integers(1, 9, 90)], 6, n_slots=100, blocks=3, reverse=1)
    check(lib, rng, [[2]] * 256, counts, 2, n_slots=256, blocks=1)
