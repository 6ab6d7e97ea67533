"""The conceal stage (aacg_units_conceal, aac.js_amd/csrc/aacg_units_conceal.h: conceal_body) against the rule of include/aacgpu.h
in numpy (conceal_kit.rule), byte for byte — unit records, every spectrum and band-word block, the results and BOTH sides of every
slot's state: the kernel's source run lane by lane on CPU threads (tests/emu/conceal_emu.cpp with tests/emu/devport_emu.h) over
hand-made records, a few frames of a few streams."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import aacgpu
import conceal_kit as kit
import emu_lib
import refresh_rule
from resident_kit import GROUPS, NODE, parse_dims
from resident_kit import shape_streams          # noqa: F401  (fixture: tests/js/shape_cases.js)

HERE = os.path.dirname(os.path.abspath(__file__))
BAD = 1                 # AACG_PARSE_INSUFFICIENT_DATA
CUTS = refresh_rule.cuts()


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    L = emu_lib.build_driver("conceal_emu", ["tests/emu/conceal_emu.cpp"], tmp_path_factory.mktemp("conceal_emu"))
    L.emu_conceal.argtypes = [C.c_void_p] * 5 + [C.c_uint32] * 3 + [C.c_void_p] + [C.c_uint32] * 4 + [C.c_int]
    sizes = (C.c_uint32 * 9)()
    L.emu_conceal_sizes(sizes)
    assert list(sizes) == [kit.DEV_UNIT_DTYPE.itemsize, kit.STREAM_DTYPE.itemsize, 256, kit.HEAD_BYTES, kit.ELEM_BYTES, kit.BLOCK_BYTES,
                           kit.side_bytes(1), kit.side_bytes(2), kit.side_bytes(8)]
    return L


def aligned(n_bytes, fill):
    raw = np.full(n_bytes + 16, fill, np.uint8)
    return raw[(-raw.ctypes.data) % 16:][:n_bytes]


class Feed:
    """streams on slots with layouts; batch after batch through the emulated launch and the rule, compared byte for byte"""

    def __init__(self, lib, members, n_slots, Cp, fade_steps, hold, seed):
        self.lib, self.members, self.Cp, self.fade, self.hold = lib, members, Cp, fade_steps, hold       # members: {slot: (layout, kept)}
        self.rng = np.random.default_rng(seed)
        self.S = kit.State(n_slots, Cp)
        self.state = aligned(self.S.bytes.size, 0xA5)
        self.n_slots, self.n_batches = n_slots, 0
        self.words = None                # band words of the next good frames (default random)
        self.window = None               # (window_sequence, group lengths) of the next good frames

    def reset(self, slot):
        self.S.reset(slot)

    def batch(self, statuses, blocks=None, reverse=0):
        """statuses: [(slot, [status of each frame])] in the batch's order -> (concealed frame indices, the launch's outputs)"""
        rng, Cp = self.rng, self.Cp
        n = sum(len(st) for _, st in statuses)
        streams, units, first = [], [], 0
        res = np.zeros(n, kit.RESULT_DTYPE)
        q = rng.integers(-300, 300, (n * Cp, 1024)).astype(np.int16)
        meta = ((rng.integers(0, 16, (n * Cp, 120)) << 12) | (rng.integers(0, 8, (n * Cp, 120)) << 9) | rng.integers(0, 428, (n * Cp, 120))).astype(np.uint16)
        if self.words is not None:
            meta[:] = self.words
        for slot, st in statuses:
            lay, kept = self.members[slot]
            streams.append(dict(frame_first=first, frames=len(st), unit_first=len(units), slot=slot, layout=lay, kept=kept))
            for f, status in enumerate(st):
                i = first + f
                res[i] = (status, 0 if status else len(lay), 0, int(rng.integers(0, 8)), int(rng.integers(0, 1 << 20)))
                chan = 0
                for e in range(kept):
                    u = np.frombuffer(rng.integers(0, 256, kit.DEV_UNIT_DTYPE.itemsize, dtype=np.uint8).tobytes(), kit.DEV_UNIT_DTYPE).copy()
                    d = u["d"]
                    d["stream"], d["channel"], d["n_ch"], d["tns_offset"] = slot, chan, lay[e], 0
                    d["coef_offset"] = d["meta_offset"] = i * Cp + chan
                    if status:                       # what the refresh makes of a refused frame
                        d["flags"] = 0
                        d["ch"] = np.zeros((), kit.CHAN_DTYPE)
                        d["ch"]["group_count"], d["ch"]["group_len"][..., 0] = 1, 1
                        u["gmap"] = 0
                    else:
                        for c in range(2):
                            seq, lens = self.window if self.window else (int(rng.integers(0, 4)), None)
                            lens = (lens or CUTS[int(rng.integers(0, 128))]) if seq == kit.EIGHT_SHORT else [1]
                            d["ch"]["window_sequence"][0, c], d["ch"]["group_count"][0, c] = seq, len(lens)
                            d["ch"]["group_len"][0, c] = 0
                            d["ch"]["group_len"][0, c, :len(lens)] = lens
                            u["gmap"][0, c] = refresh_rule.group_map(d["ch"][0, c]) if seq == kit.EIGHT_SHORT and c < lay[e] else 0
                    units.append(u[0])
                    chan += lay[e]
            first += len(st)
        units = np.array(units, kit.DEV_UNIT_DTYPE)
        tab = kit.stream_records(streams, self.S)
        # the launch, over 16-byte aligned copies with the state as the launches before left it
        g_units, g_res = units.copy(), res.copy()
        g_q, g_meta = aligned(q.nbytes, 0), aligned(meta.nbytes, 0)
        g_q[:], g_meta[:] = q.reshape(-1).view(np.uint8), meta.reshape(-1).view(np.uint8)
        longest = max(len(st) for _, st in statuses)
        jobs = len(statuses) * longest * Cp
        self.lib.emu_conceal(g_units.ctypes.data, g_res.ctypes.data, g_q.ctypes.data, g_meta.ctypes.data, tab.ctypes.data, len(streams), longest, Cp,
                             self.state.ctypes.data, self.n_slots, self.fade, self.hold, (jobs + 3) // 4 if blocks is None else blocks, reverse)
        # the rule
        d, gmap = units["d"].copy(), units["gmap"].copy()
        before = (q.copy(), meta.copy())
        concealed = kit.rule(d, gmap, res, q, meta, streams, self.S, self.fade, self.hold)
        want = units.copy()
        want["d"], want["gmap"] = d, gmap
        assert g_units.tobytes() == want.tobytes(), "unit records"
        assert g_res.tobytes() == res.tobytes(), "results"
        assert g_q.tobytes() == q.tobytes(), "spectrum blocks"
        assert g_meta.tobytes() == meta.tobytes(), "band-word blocks"
        assert self.state.tobytes() == self.S.bytes.tobytes(), "the state, both sides of every slot"
        self.n_batches += 1
        return concealed, dict(units=g_units, q=q, meta=meta, res=g_res, before=before, streams=streams)


STEREO = {0: ([2], 1), 1: ([2], 1), 2: ([2], 1)}


def test_a_refusal_in_mid_batch_and_at_a_batchs_start(lib):
    """frame 1 of 3 repeats frame 0 one step down; the next batch's FIRST frame repeats what the batch before left, and the second
    frame of that run is two steps down; the neighbour slot's records do not move.  Workgroups forward, in reverse, and one only"""
    F = Feed(lib, STEREO, 3, 2, 2, 6, 1)
    got, o = F.batch([(2, [0, BAD, 0]), (0, [0, 0])])
    assert got == [1]
    assert (o["q"][2:4] == o["before"][0][0:2]).all() and (o["meta"][2:4] == kit.fade(o["before"][1][0:2], 2)).all()
    assert F.S.r[2] == 0 and F.S.parity == [1, 0, 1] and F.S.fresh == [0, 1, 0]
    g_before = F.S.G[2]["blocks"][0][1].copy()
    got, o = F.batch([(0, [0]), (2, [BAD, BAD, 0, 0])], blocks=2, reverse=1)
    assert got == [1, 2]
    assert (o["meta"][2] == kit.fade(g_before, 2)).all() and (o["meta"][4] == kit.fade(g_before, 4)).all()
    got, _ = F.batch([(2, [BAD]), (1, [BAD]), (0, [BAD])], blocks=1)
    assert got == [0, 2] and F.S.G[1] is None and F.S.r == [1, 0, 1]


def test_a_run_that_straddles_two_batches_and_one_longer_than_the_hold(lib):
    """hold 3: two refused frames end a batch and three begin the next — r runs 1 .. 5, so the fourth and fifth are silent —, then a good
    frame, and the refused frame behind it is one step down again; r is kept at hold + 1"""
    F = Feed(lib, STEREO, 3, 2, 3, 3, 2)
    got, _ = F.batch([(1, [0, BAD, BAD])])
    assert got == [1, 2] and F.S.r[1] == 2
    got, o = F.batch([(1, [BAD, BAD, BAD, 0, BAD])], reverse=1)
    assert got == [0, 4]
    assert (o["units"]["d"]["ch"]["group_count"][1:3] == 1).all() and (o["units"]["d"]["ch"]["max_sfb"][1:3] == 0).all(), "silent units stay silent"
    assert (o["q"][2:6] == o["before"][0][2:6]).all(), "and their blocks are not written"
    assert (o["q"][8:10] == o["before"][0][6:8]).all()
    got, _ = F.batch([(1, [BAD] * 6)])
    assert got == [0, 1] and F.S.r[1] == 4
    got, _ = F.batch([(1, [BAD, BAD])])
    assert got == [] and F.S.r[1] == 4 and F.S.G[1] is not None


def test_all_refused_none_yet_and_a_reset(lib):
    """a stream with no good frame yet stays silent and leaves an empty state; a batch of one slot that is all refused carries G over
    with the new r; a reset between batches empties the slot with its next batch while the neighbour goes on"""
    F = Feed(lib, STEREO, 3, 2, 1, 6, 3)
    got, _ = F.batch([(0, [BAD, BAD]), (1, [0])])
    assert got == [] and F.S.G[0] is None and F.S.bytes[0, 1, :16].view(np.uint32).tolist() == [0, 0, 0, 0]
    got, _ = F.batch([(0, [BAD, 0, BAD]), (1, [BAD, BAD])])
    assert got == [2, 3, 4]
    got, _ = F.batch([(1, [BAD])])
    assert got == [0] and F.S.r[1] == 3
    F.reset(1)
    got, _ = F.batch([(0, [BAD]), (1, [BAD, BAD])], blocks=1)
    assert got == [0] and F.S.G[1] is None and F.S.r[0] == 2
    got, _ = F.batch([(1, [0, BAD])])
    assert got == [1]


def test_three_elements_and_eight_short_windows_in_three_groups(lib):
    """SCE + CPE + LFE of a 5.1 layout whose fourth element is not decoded (kept 3 of 4), eight parser blocks a frame; G has eight short
    windows in three groups in every channel, and the concealed units' group maps are the ones the refresh derives"""
    F = Feed(lib, {0: ([1, 2, 1, 2], 3), 3: ([2], 1)}, 4, 8, 2, 6, 4)
    F.window = (kit.EIGHT_SHORT, [3, 1, 4])
    got, o = F.batch([(3, [0, BAD]), (0, [0, BAD, BAD])])
    assert got == [1, 3, 4]
    u = o["units"]
    assert len(u) == 2 + 9 and (u["d"]["ch"]["window_sequence"][[1, 5, 6, 7, 8]] == kit.EIGHT_SHORT).all()
    want = refresh_rule.group_map(u["d"]["ch"][0, 0])
    assert want == 0x22221000 and u["gmap"][1].tolist() == [want, want]
    assert u["gmap"][5].tolist() == [want, 0] and u["gmap"][6].tolist() == [want, want] and u["gmap"][7].tolist() == [want, 0]
    assert (o["q"][3 * 8 + 4:3 * 8 + 8] == o["before"][0][3 * 8 + 4:3 * 8 + 8]).all(), "the blocks of the element that is not decoded are not written"
    F.window = None
    got, _ = F.batch([(0, [BAD]), (3, [BAD, 0])], reverse=1)
    assert got == [0, 1]


def test_band_types_scalefactors_that_clamp_and_no_fade(lib):
    """words of band type 0, 13, 14 and 15 (zero, noise, intensity) are copied unchanged, type 12 too; coded bands lose r * fade_steps
    and stop at 0; bits 9..11 stay.  With fade_steps = 0 the repeat is G's words"""
    words = np.zeros(120, np.uint16)
    for b in range(120):
        words[b] = ((b % 16) << 12) | ((b % 8) << 9) | [0, 1, 3, 5, 6, 7, 200, 427][b % 8 if b < 64 else (b // 8) % 8]
    F = Feed(lib, STEREO, 3, 2, 3, 6, 5)
    F.words = words
    got, o = F.batch([(0, [0, BAD, BAD])])
    assert got == [1, 2]
    for r, block in ((1, 2), (2, 4)):
        m = o["meta"][block].astype(np.int64)
        bt, sf = words.astype(np.int64) >> 12, words.astype(np.int64) & 0x1ff
        coded = (bt >= 1) & (bt <= 11)
        assert (m[~coded] == words[~coded]).all() and ((m >> 9) == (words >> 9)).all()
        assert ((m & 0x1ff)[coded] == np.maximum(sf[coded] - 3 * r, 0)).all()
        assert ((m & 0x1ff)[coded] == 0).any() and ((m & 0x1ff)[coded] > 0).any()
    F0 = Feed(lib, STEREO, 3, 2, 0, 2, 6)
    F0.words = words
    got, o = F0.batch([(1, [0, BAD, BAD, BAD])])
    assert got == [1, 2] and (o["meta"][2:6] == words).all()


def test_ragged_counts_and_looks_longer_than_a_wave(lib):
    """counts 1, 70 and 2: a look back and a look forward of more than 64 frames, a single-frame stream that is refused, and a stream
    whose last frame is the only good one"""
    F = Feed(lib, STEREO, 3, 2, 1, 66, 7)
    long_run = [0] + [BAD] * 69
    got, _ = F.batch([(1, [0]), (0, long_run), (2, [BAD, 0])], blocks=9)
    assert got == list(range(2, 68)) and F.S.r == [67, 0, 0]
    got, _ = F.batch([(1, [BAD]), (0, [BAD] * 68 + [0, BAD]), (2, [0])], blocks=3, reverse=1)
    assert got == [0, 70] and F.S.r == [1, 1, 0]


def test_conceal_under_sanitizers(tmp_path):
    """the same driver as a program of its own, built with -fsanitize=address,undefined and run as a child process: two batches of
    three streams (a CPE stream, an SCE + CPE + LFE stream, an SCE stream), eight parser channels, over heap blocks of exactly the
    buffers' sizes.  The sanitizers' runtimes are linked into the program: nothing is preloaded."""
    exe = str(tmp_path / "conceal_emu_san")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fno-strict-aliasing", "-DAACG_EMU_BUILD", "-DCONCEAL_EMU_MAIN", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-I", os.path.join(HERE, "emu"), "-pthread", "-Wall", "-Wno-unused-function",
           "-Wno-unknown-pragmas", "-o", exe, os.path.join(HERE, "emu", "conceal_emu.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "conceal_emu: ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.skipif(NODE is None, reason="node not present")
def test_a_table_entry_cut_to_nine_bytes_is_refused(shape_streams):
    """how tests/test_units_conceal_gpu.py drops a frame, on the device parser's source run on the CPU: of every 12-frame stream at
    sample index 3, exactly the entries cut to 9 bytes come back with a status, whichever they are"""
    emu = emu_lib.Emu()
    entries, counts = aacgpu.standard_codebooks()
    for names, C_, si in [g for g in GROUPS if g[2] == 3]:
        U, Cp = parse_dims(C_)
        for name in names.split("+"):
            _, data, table = shape_streams[name]
            for drops in ([4, 9], [5, 6, 7], [3, 4, 5, 6, 7], [0, 1, 6], []):
                out = emu_lib.emu_parse(emu, si, entries, counts, data, kit.dropped(table, drops), U, Cp, aacgpu.PARSE_REFERENCE_QUIRKS, False)
                assert np.flatnonzero(out["results"]["status"]).tolist() == drops, (name, drops, out["results"]["status"].tolist())
