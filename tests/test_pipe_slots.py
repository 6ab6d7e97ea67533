"""The resident route's slot state, record builders, commits and record block (aac.js_amd/csrc/aacg_pipe_slots.h) against the counting
rules restated here in Python integers from the headers' documented formulas — resampler: ceil((N + 1024 F) L / M) - ceil(N L / M);
features: count(N) = max(0, floor((N + P - K) / H) + 1); meter: floor((N + n) / hop) - floor(N / hop); trim: [Q, Q + n) n [S, S + K) —
and cross-checked with the host functions aacg_resample_counts, aacg_features_counts, aacg_loudness_counts and aacg_trim_counts.  The
oracle calls nothing of the header under test.  Three slots, ragged batches of 1 to 3 frames, six consecutive batches, two of which
leave slots out, a reset in mid-run.  Host code through tests/emu/slots_emu.cpp; no GPU."""
import ctypes as C

import numpy as np
import pytest

import emu_lib

ALL = (1 << 64) - 1                                        # AACG_TRIM_ALL
RS, FT, LD, LIM, CN, TR = range(6)                         # record_block's sections, in their order
U32 = "<u4"
DTYPES = [np.dtype([(n, U32) for n in ("frame_first", "frames", "out_first", "n_out", "n0", "slot", "parity", "fresh")]),                       # aacg_resample_stream
          np.dtype([("in_first", U32), ("n_in", U32), ("out_first", U32), ("n_out", U32), ("item_first", U32), ("off0", "<i4"), ("slot", U32), ("flags", U32)]),
          np.dtype([(n, U32) for n in ("frame_first", "frames", "out_first", "n_out", "n0", "slot", "parity", "fresh")]),                       # aacg_loudness_stream
          np.dtype([("frame_first", U32), ("frames", U32), ("slot", U32), ("parity", U32), ("fresh", U32), ("gain", "<f4"), ("unused", U32, (2,))]),
          np.dtype([(n, U32) for n in ("frame_first", "frames", "unit_first", "frame_units", "slot", "nch", "state", "reserved")]),             # aacg_conceal_stream
          np.dtype([(n, U32) for n in ("src_first", "n_keep", "out_first", "item_first")])]                                                      # aacg_trim_stream
SIZES = [32, 32, 32, 32, 32, 16]

N_SLOTS = 3
# (slots in the batch's order, frames of each): ragged, orders vary, the fifth leaves two slots out and the second one
BATCHES = [([0, 1, 2], [1, 2, 3]), ([2, 0], [3, 1]), ([1, 2, 0], [2, 2, 1]), ([0, 1, 2], [3, 1, 2]), ([1], [2]), ([2, 1, 0], [1, 3, 2])]
RESET = (3, 2)                                             # in front of batch 3, slot 2 is reset


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    L = emu_lib.build_driver("slots_emu", ["tests/emu/slots_emu.cpp", "aac.js_amd/csrc/aacg_resample.cpp", "aac.js_amd/csrc/aacg_features.cpp",
                                           "aac.js_amd/csrc/aacg_loudness.cpp", "aac.js_amd/csrc/aacg_trim.cpp"], tmp_path_factory.mktemp("slots_emu"))
    V = C.c_void_p
    L.emu_slots_make.argtypes, L.emu_slots_make.restype = [V], V
    L.emu_slots_free.argtypes, L.emu_slots_free.restype = [V], None
    L.emu_slots_build.argtypes, L.emu_slots_build.restype = [V, V, V, C.c_uint32, C.c_int, V, C.c_uint64], None
    L.emu_slots_commit.argtypes, L.emu_slots_commit.restype = [V, C.c_int], None
    L.emu_slots_reset.argtypes, L.emu_slots_reset.restype = [V, C.c_uint32], None
    L.emu_slots_set_gain.argtypes, L.emu_slots_set_gain.restype = [V, C.c_uint32, C.c_float], None
    L.emu_slots_set_window.argtypes, L.emu_slots_set_window.restype = [V, C.c_uint32, C.c_uint64, C.c_uint64], None
    L.emu_slots_state.argtypes, L.emu_slots_state.restype = [V, C.c_uint32, V, V], None
    L.emu_slots_totals.argtypes, L.emu_slots_totals.restype = [V, V], None
    L.emu_slots_trim_in.argtypes, L.emu_slots_trim_in.restype = [V, V], C.c_uint32
    L.emu_slots_sections.argtypes, L.emu_slots_sections.restype = [V, V], C.c_uint64
    L.emu_slots_copy.argtypes, L.emu_slots_copy.restype = [V, V, C.c_int], None
    L.emu_slots_records.argtypes, L.emu_slots_records.restype = [V, C.c_int, V], C.c_uint64
    L.aacg_resample_counts.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, V, V]
    L.aacg_features_counts.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, V]
    L.aacg_loudness_counts.argtypes = [C.c_uint32, C.c_uint64, C.c_uint64, V]
    L.aacg_trim_counts.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, V, C.c_uint32, V, V]
    return L


# ---- the oracle: the rules in Python integers, state per slot in plain lists ----
def ceil_div(a, b):
    return -((-a) // b)


def ft_count(K, H, P, N):
    return max(0, (N + P - K) // H + 1) if N + P >= K else 0


def trim_span(Q, S, K, n):
    lo, hi = max(Q, S), (Q + n if K == ALL else min(Q + n, S + K))
    return (lo - Q, hi - lo) if hi > lo else (0, 0)


class Model:
    """what the pipeline is (cfg as slots_emu.cpp's emu_slots_make takes it) and the slots' state: absolute clocks, parities, fresh flags"""

    def __init__(self, rs=None, ft=None, hop=0, true_peak=False, channels=2, limiter=False, conceal=False, trim=None):
        self.rs, self.ft, self.hop, self.tp, self.C, self.lim, self.cn, self.tr = rs, ft, hop, true_peak, channels, limiter, conceal, trim is not None
        z = lambda v=0: [v] * N_SLOTS
        self.N = {"rs": z(), "ft": z(), "ld": z()}
        self.parity = {k: z() for k in ("rs", "ft", "ld", "lim", "cn")}
        self.fresh = {k: z(1) for k in ("rs", "ft", "ld", "lim", "cn")}
        self.gain = z(1.0)
        self.S, self.K, self.Q = z(trim[0] if trim else 0), z(trim[1] if trim else 0), z()

    def cfg(self):
        rs, ft = self.rs or (0, 0), self.ft or (0, 0, 0)
        return np.array([N_SLOTS, rs[0], rs[1], ft[0], ft[1], ft[2], self.hop, self.tp, self.C, self.lim, self.cn, self.tr, self.S[0], self.K[0]], np.uint64)

    def stages(self):
        return [k for k, on in (("rs", self.rs), ("ft", self.ft), ("ld", self.hop), ("lim", self.lim), ("cn", self.cn)) if on]

    def build(self, slots, frames, planar, tab):
        """-> ({section: [record tuples in the dtype's field order]}, totals, what each stream brings the trim); changes nothing"""
        rec, firsts = {}, [sum(frames[:s]) for s in range(len(slots))]
        n_in, place = [1024 * f for f in frames], [1024 * f for f in firsts]           # what the next stage receives, and where each stream's lies
        tot = dict.fromkeys(("rs_total", "rs_most", "tr_total", "tr_most", "tr_items", "ft_total", "ft_most", "ft_items", "ld_floats", "tp_floats"), 0)
        if self.rs:
            L, M = self.rs
            n_out = [ceil_div((self.N["rs"][k] + 1024 * f) * L, M) - ceil_div(self.N["rs"][k] * L, M) for k, f in zip(slots, frames)]
            rec[RS] = [(firsts[s], frames[s], sum(n_out[:s]), n_out[s], self.N["rs"][k] % M, k, self.parity["rs"][k], self.fresh["rs"][k]) for s, k in enumerate(slots)]
            n_in, place = n_out, [sum(n_out[:s]) for s in range(len(slots))]
            tot["rs_total"], tot["rs_most"] = sum(n_out), max(n_out)
        trim_in = []
        if self.tr:
            spans = [trim_span(self.Q[k], self.S[k], self.K[k], n) for k, n in zip(slots, n_in)]
            keep = [n for _, n in spans]
            items = [ceil_div(n, 512) if n else (1 if planar and not self.ft else 0) for n in keep]
            rec[TR] = [(place[s] + spans[s][0], keep[s], sum(keep[:s]), sum(items[:s])) for s in range(len(slots))]
            trim_in = list(n_in)
            n_in, place = keep, [p + off for p, (off, _) in zip(place, spans)]
            tot["tr_total"], tot["tr_most"], tot["tr_items"] = sum(keep), max(keep), sum(items)
        if self.ft:
            K, H, P = self.ft
            j0 = [ft_count(K, H, P, self.N["ft"][k]) for k in slots]
            n_out = [ft_count(K, H, P, self.N["ft"][k] + n) - j for k, n, j in zip(slots, n_in, j0)]
            items = [ceil_div(n, 16) if n else 1 for n in n_out]
            rec[FT] = [(place[s], n_in[s], sum(n_out[:s]), n_out[s], sum(items[:s]), j0[s] * H - P - self.N["ft"][k], k,
                        self.parity["ft"][k] | self.fresh["ft"][k] << 1) for s, k in enumerate(slots)]
            tot["ft_total"], tot["ft_most"], tot["ft_items"] = sum(n_out), max(n_out), sum(items)
        if self.hop:
            n_out = [(self.N["ld"][k] + 1024 * f) // self.hop - self.N["ld"][k] // self.hop for k, f in zip(slots, frames)]
            rec[LD] = [(firsts[s], frames[s], sum(n_out[:s]), n_out[s], self.N["ld"][k] % self.hop, k, self.parity["ld"][k], self.fresh["ld"][k]) for s, k in enumerate(slots)]
            tot["ld_floats"], tot["tp_floats"] = sum(n_out) * self.C * 2, sum(n_out) * self.C if self.tp else 0
        if self.lim:
            rec[LIM] = [(firsts[s], frames[s], k, self.parity["lim"][k], self.fresh["lim"][k], np.float32(self.gain[k]), (0, 0)) for s, k in enumerate(slots)]
        if self.cn:
            rec[CN] = [tuple(int(v) for v in row) + (self.parity["cn"][row[4]] | self.fresh["cn"][row[4]] << 1, 0) for row in tab]
        return rec, tot, trim_in

    def commit(self, slots, frames, rec, trim_in, planned):
        for s, (k, f) in enumerate(zip(slots, frames)):
            self.N["rs"][k] += 1024 * f if self.rs else 0
            self.N["ld"][k] += 1024 * f if self.hop else 0
            self.N["ft"][k] += rec[FT][s][1] if self.ft else 0
            self.Q[k] += trim_in[s] if self.tr else 0
            flips = [st for st in self.stages() if st != "cn" or (planned and (rec[CN][s][3] >> 8) & 0xff)]
            for st in flips:
                self.parity[st][k] ^= 1
                self.fresh[st][k] = 0

    def reset(self, k):
        for st in self.stages():
            self.fresh[st][k] = 1
        self.N["rs"][k] = self.N["ft"][k] = self.N["ld"][k] = self.Q[k] = 0


# ---- the driver's side ----
def u32(v):
    return np.ascontiguousarray(v, np.uint32)


def norm(rec):
    return tuple(tuple(v) if isinstance(v, (tuple, list, np.ndarray)) else v for v in rec)


def state_of(lib, h, k):
    out, gain = np.zeros(23, np.uint64), C.c_float()
    lib.emu_slots_state(h, k, out.ctypes.data, C.byref(gain))
    return [int(v) for v in out], gain.value


def want_state(m, k):
    out = []
    for st in ("rs", "ft", "ld", "lim", "cn"):
        on = st in m.stages()
        clock = m.N[st][k] % m.rs[1] if st == "rs" and on else m.N.get(st, [0] * N_SLOTS)[k] if on else 0
        out += [clock, m.parity[st][k], m.fresh[st][k], m.parity[st][k] | m.fresh[st][k] << 1] if on else [0, 0, 0, 0]
    return out + ([m.S[k], m.K[k], m.Q[k]] if m.tr else [0, 0, 0]), (m.gain[k] if m.lim else 0.0)


def records(lib, h, section, n):
    buf = np.zeros(max(n, 1), DTYPES[section])
    got = lib.emu_slots_records(h, section, buf.ctypes.data)
    assert got in (0, n * SIZES[section]) and DTYPES[section].itemsize == SIZES[section]
    return buf[:got // SIZES[section]]


def tab_of(slots, frames, kept):
    """a shaped plan's table as far as the concealment's records take it: frame_first, frames, unit_first, frame_units, slot, nch"""
    rows, unit = [], 0
    for s, (k, f) in enumerate(zip(slots, frames)):
        rows.append((sum(frames[:s]), f, unit, 1 | kept[k] << 8, k, 2))
        unit += f * kept[k]
    return rows


def cross_check(lib, m, slots, frames, rec):
    """the oracle's counts against the untouched host functions, stream by stream"""
    for s, (k, f) in enumerate(zip(slots, frames)):
        if m.rs:
            per, after = np.zeros(f, np.uint32), C.c_uint32()
            assert lib.aacg_resample_counts(m.rs[0], m.rs[1], m.N["rs"][k] % m.rs[1], f, per.ctypes.data, C.byref(after)) == 0
            assert int(per.sum()) == rec[RS][s][3] and after.value == (m.N["rs"][k] + 1024 * f) % m.rs[1]
        if m.ft:
            n = C.c_uint64()
            assert lib.aacg_features_counts(m.ft[0], m.ft[1], m.ft[2], m.N["ft"][k], rec[FT][s][1], C.byref(n)) == 0 and n.value == rec[FT][s][3]
        if m.hop:
            n = C.c_uint64()
            assert lib.aacg_loudness_counts(m.hop, m.N["ld"][k], 1024 * f, C.byref(n)) == 0 and n.value == rec[LD][s][3]
        if m.tr:
            n_in, first, kept = u32([rec["trim_in"][s]]), np.zeros(1, np.uint32), np.zeros(1, np.uint32)
            assert lib.aacg_trim_counts(m.Q[k], m.S[k], m.K[k], n_in.ctypes.data, 1, first.ctypes.data, kept.ctypes.data) == 0
            assert int(kept[0]) == rec[TR][s][1] and (not kept[0] or int(first[0]) == rec[TR][s][0] - rec["place"][s])


def run(lib, m, planar=False, windows=None, gains=None, kept=(1, 1, 1), planned=None, batches=BATCHES, reset=RESET):
    """every batch: build, compare with the oracle field by field, build again, lay out and copy, commit, compare the state.  gains:
    {batch: (slot, gain)} set in front of that batch; planned: per batch, whether it had a plan.  -> what the batches' records were"""
    h = lib.emu_slots_make(m.cfg().ctypes.data)
    seen = []
    try:
        for k, (skip, keep) in (windows or {}).items():
            lib.emu_slots_set_window(h, k, skip, keep)
            m.S[k], m.K[k] = skip, keep
        for i, (slots, frames) in enumerate(batches):
            if reset and i == reset[0]:
                before, _ = state_of(lib, h, reset[1])
                lib.emu_slots_reset(h, reset[1])
                m.reset(reset[1])
                after, gain = state_of(lib, h, reset[1])
                assert (after, gain) == want_state(m, reset[1])
                # clocks and the position start again, fresh is set; parity, gain and window stay
                for st in range(5):
                    assert after[4 * st] == 0 and after[4 * st + 1] == before[4 * st + 1] and after[4 * st + 2] == (1 if ("rs", "ft", "ld", "lim", "cn")[st] in m.stages() else 0)
                assert after[20:22] == before[20:22] and after[22] == 0
            if gains and i in gains:
                lib.emu_slots_set_gain(h, gains[i][0], gains[i][1])
                m.gain[gains[i][0]] = gains[i][1]
            n, plan = len(slots), True if planned is None else planned[i]
            tab = tab_of(slots, frames, kept) if m.cn else None
            tab_np = u32(tab) if m.cn else None
            want, tot, trim_in = m.build(slots, frames, planar, tab)
            base = 4096 + ((n * 36 + 15) & ~15)                                        # a 16-byte aligned place behind a per-stream table
            states = [state_of(lib, h, k) for k in range(N_SLOTS)]
            slots_np, frames_np = u32(slots), u32(frames)
            got = None
            for again in range(2):                                                     # the refused-submission rule: building changes nothing
                lib.emu_slots_build(h, slots_np.ctypes.data, frames_np.ctypes.data, n, int(planar), tab_np.ctypes.data if m.cn else None, base)
                now = [records(lib, h, sec, n).tobytes() for sec in range(6)]
                assert got is None or now == got
                got = now
                assert [state_of(lib, h, k) for k in range(N_SLOTS)] == states
            for sec in range(6):                                                       # every record, field by field
                r = records(lib, h, sec, n)
                assert len(r) == (n if sec in want else 0), (i, sec)
                for s in range(len(r)):
                    assert norm(r[s].tolist()) == norm(want[sec][s]), (i, sec, s)
            totals = np.zeros(10, np.uint64)
            lib.emu_slots_totals(h, totals.ctypes.data)
            assert dict(zip(tot, (int(v) for v in totals))) == tot, i
            tin = np.zeros(n, np.uint32)
            assert lib.emu_slots_trim_in(h, tin.ctypes.data) == len(trim_in) and tin[:len(trim_in)].tolist() == trim_in
            place = [r[0] - trim_span(m.Q[k], m.S[k], m.K[k], t)[0] for r, k, t in zip(want.get(TR, []), slots, trim_in)]
            cross_check(lib, m, slots, frames, dict(want, trim_in=trim_in, place=place))
            check_block(lib, h, m, n, base, got)
            lib.emu_slots_commit(h, int(plan))
            m.commit(slots, frames, want, trim_in, plan)
            for k in range(N_SLOTS):
                assert state_of(lib, h, k) == want_state(m, k), (i, k)
            seen.append(want)
    finally:
        lib.emu_slots_free(h)
    return seen


def check_block(lib, h, m, n, base, rec_bytes):
    """sections in their order from the base, back to back, the trim's absent with a feature stage; the copy puts each section's bytes
    at its place and touches nothing else"""
    sec = np.zeros(12, np.uint64)
    end = int(lib.emu_slots_sections(h, sec.ctypes.data))
    at, size = [int(v) for v in sec[0::2]], [int(v) for v in sec[1::2]]
    present = {RS: bool(m.rs), FT: bool(m.ft), LD: bool(m.hop), LIM: m.lim, CN: m.cn, TR: m.tr and not m.ft}
    assert size == [n * SIZES[i] if present[i] else 0 for i in range(6)]
    assert at[0] == base and base % 16 == 0 and all(at[i + 1] == at[i] + size[i] for i in range(5)) and end == at[5] + size[5]
    block = np.full(end + 64, 0xAA, np.uint8)
    lib.emu_slots_copy(h, block.ctypes.data, -1)
    for i in range(6):
        assert block[at[i]:at[i] + size[i]].tobytes() == (rec_bytes[i] if present[i] else b""), i
    assert (block[:base] == 0xAA).all() and (block[end:] == 0xAA).all()
    one = np.full(end + 64, 0xAA, np.uint8)                                            # one section alone, as choose_plan copies the concealment's
    lib.emu_slots_copy(h, one.ctypes.data, CN)
    assert one[at[CN]:at[CN] + size[CN]].tobytes() == (rec_bytes[CN] if m.cn else b"") and (one[:at[CN]] == 0xAA).all() and (one[at[CN] + size[CN]:] == 0xAA).all()


# ---- the cases ----
@pytest.mark.parametrize("L,M", [(1, 3), (160, 147)])
def test_resampler(lib, L, M):
    seen = run(lib, Model(rs=(L, M)))
    clocks = [r[4] for b in seen for r in b[RS]]
    assert any(c for c in clocks) and all(c < M for c in clocks)                       # the clock wraps modulo M: 1024 is a multiple of neither
    assert sum(r[3] for b in seen for r in b[RS] if r[5] == 0) == ceil_div(8 * 1024 * L, M)      # slot 0's eight frames, however they were split


@pytest.mark.parametrize("pad", [0, 200])
def test_features_behind_a_resampler(lib, pad):
    seen = run(lib, Model(rs=(1, 3), ft=(400, 160, pad), channels=1))
    first = seen[0][FT][0]                                                             # slot 0's first batch: one frame, 342 samples at 16 kHz
    assert first[1] == 342 and first[3] == (0 if pad == 0 else 1) and first[7] == 2    # ... completes no frame without the padding; fresh
    assert any(r[3] > 1 for b in seen for r in b[FT])


def test_features_alone(lib):
    seen = run(lib, Model(ft=(400, 160, 200), channels=1))
    assert seen[0][FT][0][1:4] == (1024, 0, 6) and seen[0][FT][0][5] == -200           # (1024 + 200 - 400) // 160 + 1 frames, the first 200 in front of the batch


@pytest.mark.parametrize("hop,true_peak", [(4800, False), (1000, True), (4800, True)])
def test_meter(lib, hop, true_peak):
    seen = run(lib, Model(hop=hop, true_peak=true_peak, channels=2))
    emits = [r[3] for b in seen for r in b[LD]]
    assert (0 in emits) == (hop == 4800) and any(emits)                                # at hop 4800 some streams emit nothing; 1000 divides no 1024
    assert any(r[4] for b in seen for r in b[LD])                                      # ... and neither hop, so clocks stand inside a hop


@pytest.mark.parametrize("planar", [False, True])
def test_trim_windows(lib, planar):
    seen = run(lib, Model(trim=(1500, 2000)), planar=planar, windows={1: (0, ALL), 2: (100, 300)})
    keep = {k: [r[1] for b, (slots, _) in zip(seen, BATCHES) for r, s in zip(b[TR], slots) if s == k] for k in range(N_SLOTS)}
    assert keep[0] == [0, 548, 1024, 428, 0] and keep[1] == [2048, 2048, 1024, 2048, 3072]      # [1500, 3500) of pieces of 1024, 1024, 1024, 3072, 2048; everything
    assert keep[2] == [300, 0, 0, 300, 0]                                              # a stream that keeps nothing of a batch; reset, its window counts from the start again


@pytest.mark.parametrize("planar", [False, True])
def test_trim_a_window_that_ends_before_the_batch(lib, planar):
    seen = run(lib, Model(trim=(0, 500)), planar=planar, reset=None)
    assert [sum(r[1] for r in b[TR]) for b in seen] == [1500, 0, 0, 0, 0, 0]           # whole batches that keep nothing
    items = [sum(-(-r[1] // 512) if r[1] else int(planar) for r in b[TR]) for b in seen]
    assert items == ([3, 2, 3, 3, 1, 3] if planar else [3, 0, 0, 0, 0, 0])             # a planar stream that keeps nothing is one item, for its zeros


def test_trim_behind_the_resampler_in_front_of_features(lib):
    seen = run(lib, Model(rs=(160, 147), ft=(400, 160, 200), channels=1, trim=(1500, 2000)), windows={1: (0, ALL), 2: (100, 300)})
    for b in seen:
        for rs, tr, ft in zip(b[RS], b[TR], b[FT]):
            assert rs[2] <= tr[0] <= rs[2] + rs[3] and (ft[0], ft[1]) == (tr[0], tr[1])                 # the chained inputs: the kept range of the resampled stream
    assert any(ft[1] == 0 for b in seen for ft in b[FT]) and any(0 < ft[1] < rs[3] for b in seen for rs, ft in zip(b[RS], b[FT]))


def test_limiter_gain_as_it_stands(lib):
    seen = run(lib, Model(limiter=True), gains={2: (1, 0.25), 4: (1, 3.0)})
    gains = [r[5] for b, (slots, _) in zip(seen, BATCHES) for r, s in zip(b[LIM], slots) if s == 1]
    assert gains == [1.0, 0.25, 0.25, 3.0, 3.0]                                        # set between batches: the next batch's records have it, no earlier one
    assert all(r[5] == 1.0 for b in seen for r in b[LIM] if r[2] != 1)


def test_concealment_commits_with_a_plan_and_kept_units(lib):
    planned = [True, True, False, True, True, True]
    seen = run(lib, Model(conceal=True), kept=(1, 0, 2), planned=planned)              # slot 1 has no layout: no unit of it is kept
    side = {k: [r[6] for b, (slots, _) in zip(seen, BATCHES) for r, s in zip(b[CN], slots) if s == k] for k in range(N_SLOTS)}
    assert side[1] == [2] * 5                                                          # never through a launch: fresh, side 0, for ever
    assert side[0] == [2, 1, 0, 0, 1]                                                  # batch 2 had no plan: batch 3 reads the side batch 2 read
    assert side[2] == [2, 1, 0, 2, 1]                                                  # ... and the reset in front of batch 3 sets fresh and leaves the side


@pytest.mark.parametrize("features", [False, True])
def test_every_stage_side_by_side(lib, features):
    """all six sections (five with a feature stage: the trim's records stay down); check_block has the offsets and the bytes"""
    m = Model(rs=(1, 3), ft=(400, 160, 200) if features else None, hop=1000, true_peak=True, channels=1, limiter=True, conceal=True, trim=(1500, 2000))
    seen = run(lib, m, planar=True, windows={1: (0, ALL)}, gains={1: (0, 2.0)}, kept=(1, 1, 0), planned=[True] * 5 + [False])
    assert all(set(b) == ({RS, FT, LD, LIM, CN, TR} if features else {RS, LD, LIM, CN, TR}) for b in seen)
