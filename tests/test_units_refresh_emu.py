"""A plan's unit records rewritten from the parser's (aacg_units_refresh, aac.js_amd/csrc/aacg_units_refresh.h: refresh_body) against
the rule stated in numpy (tests/refresh_rule.py: its docstring is the rule), byte for byte over the whole record array — poisoned
tail records behind n_units included —, the whole result array and the refusal counter: the kernel's source run lane by lane on CPU
threads (tests/emu/refresh_emu.cpp with tests/emu/devport_emu.h), as ceil(n / 256) workgroups of 256 concurrent lanes, workgroups
forward and in reverse.

The inputs: the parser's part of the plan's records (flags, ch, tns_offset, gmap) is 0xA5 before each launch — a set is stale memory
from an older batch —, every other byte of them random; the parsed records of refused frames and of the slots e >= n_units are 0xFF,
or — where a case says so — stale records that would match, which only the status or the element count keeps out."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import aacgpu
import emu_lib
import refresh_rule as R

HERE = os.path.dirname(os.path.abspath(__file__))
TAIL = 3                # poisoned records behind n_units
PARSE_ERROR = 4         # AACG_PARSE_SCALEFACTOR: any status but OK and LAYOUT


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    L = emu_lib.build_driver("refresh_emu", ["tests/emu/refresh_emu.cpp"], tmp_path_factory.mktemp("refresh_emu"))
    L.emu_refresh.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_int]
    L.emu_refresh.restype = None
    sizes = (C.c_uint32 * 4)()
    L.emu_refresh_sizes(sizes)
    assert sizes[0] == R.DEV_UNIT_DTYPE.itemsize and sizes[1] == R.MAP_DTYPE.itemsize and sizes[2] == R.RESULT_DTYPE.itemsize
    L.threads = int(sizes[3])
    assert L.threads == 256
    return L


class Batch:
    """made inputs of one launch: parser frames (records, results), the plan's records and — map mode — the map"""

    def __init__(self, rng, max_units, parse_channels):
        self.rng, self.U, self.Cp = rng, max_units, parse_channels
        self.frames, self.results = [], []

    def frame(self, layout, status=0, n_units=None, stale=False, **kw):
        """one parser frame -> its index.  status != 0 / n_units below the layout: the records nobody may trust are 0xFF, or
        (stale) stay as a frame that parses would have left them"""
        f = len(self.frames)
        recs = R.parsed_frame(self.rng, f, layout, self.U, self.Cp, **kw)
        n = len(layout) if n_units is None else n_units
        if not stale:
            if status:
                recs[:] = np.frombuffer(b"\xff" * recs.nbytes, recs.dtype)
            else:
                recs[n:] = np.frombuffer(b"\xff" * recs[n:].nbytes, recs.dtype)
        self.frames.append(recs)
        r = np.zeros(1, R.RESULT_DTYPE)
        r["status"], r["n_units"], r["n_channels"], r["flags"], r["bits_used"] = status, n, sum(layout), self.rng.integers(0, 8), self.rng.integers(0, 1 << 20)
        self.results.append(r)
        return f

    def finish(self, picks, want=None, listed=None, n_out_ch=None):
        """picks: (frame, element) of each plan unit in the plan's order.  want / listed: per unit (or one for all) -> a map."""
        self.parsed = np.concatenate(self.frames)
        self.res = np.concatenate(self.results)
        idx = np.array([f * self.U + e for f, e in picks], np.int64)
        self.units = R.plan_units(self.rng, self.parsed, idx, self.rng.integers(0, 4, len(idx)), n_out_ch or self.Cp)
        self.map = None
        if want is not None:
            self.map = np.zeros(len(idx), R.MAP_DTYPE)
            self.map["parsed_index"] = idx
            self.map["frame_units"] = np.asarray(want) | (np.asarray(listed if listed is not None else 0) << 8)
        return self

    def plan_of(self, frame, element):
        """index of the plan unit listed for (frame, element)"""
        return int(np.nonzero(self.index() == frame * self.U + element)[0][0])

    def index(self):
        return self.map["parsed_index"] if self.map is not None else np.arange(len(self.units))

    def move(self, frame, element, field="coef_offset"):
        """the plan expects the element elsewhere (or as another element): its record no longer matches"""
        self.units["d"][field][self.plan_of(frame, element)] += 1


def launch(lib, B, units, results, counter, refuse_pns, keep_tns, reverse):
    """one launch over copies: the records with TAIL poisoned ones behind them, the results, the counter"""
    n = len(units)
    got = np.concatenate([units, np.frombuffer(b"\x5c" * (TAIL * R.DEV_UNIT_DTYPE.itemsize), R.DEV_UNIT_DTYPE)])
    res = results.copy()
    cnt = np.array([counter], np.uint32)
    lib.emu_refresh(got.ctypes.data, B.parsed.ctypes.data, res.ctypes.data, B.map.ctypes.data if B.map is not None else None, n, B.U,
                    refuse_pns, keep_tns, cnt.ctypes.data, reverse)
    assert (got[n:].view(np.uint8) == 0x5c).all(), "a record behind n_units was written"
    return got[:n], res, int(cnt[0])


def check(lib, B, refuse_pns=1, keep_tns=0, retry=True):
    """the launch against the rule, workgroups forward and in reverse; then (retry) the same set refreshed again, as after a stale
    plan.  -> (the rule's records, its results, the refused count, per unit: accepted?)"""
    want_u, want_r, want_n, taken = R.refresh(B.units, B.parsed, B.res, B.map, B.U, refuse_pns, keep_tns)
    if B.map is None:
        assert want_r.tobytes() == B.res.tobytes()
    # every byte outside flags, ch, tns_offset and gmap is the input's
    assert R.poison_parser_part(want_u.copy()).tobytes() == B.units.tobytes()
    for reverse in (0, 1):
        got_u, got_r, got_n = launch(lib, B, B.units, B.res, 1000, refuse_pns, keep_tns, reverse)
        diff = np.nonzero((got_u.view(np.uint8).reshape(len(got_u), -1) != want_u.view(np.uint8).reshape(len(got_u), -1)).any(axis=1))[0]
        assert got_u.tobytes() == want_u.tobytes(), "the kernel's records differ from the rule's at units %s (reverse %d)" % (diff[:8], reverse)
        assert got_r.tobytes() == want_r.tobytes(), "the kernel's results differ from the rule's (reverse %d)" % reverse
        assert got_n == 1000 + want_n, "refused: %d counted, the rule has %d" % (got_n - 1000, want_n)
        if retry:
            # the retry: the set as the first pass left it, the results as it left them (LAYOUT where it refused)
            again_u, again_r, again_n = launch(lib, B, got_u, got_r, got_n, refuse_pns, keep_tns, 1 - reverse)
            rule_u, rule_r, rule_n, _ = R.refresh(got_u, B.parsed, got_r, B.map, B.U, refuse_pns, keep_tns)
            assert again_u.tobytes() == got_u.tobytes() == rule_u.tobytes() and again_r.tobytes() == got_r.tobytes() == rule_r.tobytes()
            assert again_n == got_n + want_n == got_n + rule_n
    return want_u, want_r, want_n, taken


def assert_silent(u):
    assert (u["d"]["flags"] == 0).all() and (u["d"]["tns_offset"] == 0).all() and (u["gmap"] == 0).all()
    ch = u["d"]["ch"]
    assert (ch["group_count"] == 1).all() and (ch["group_len"][..., 0] == 1).all() and (ch["group_len"][..., 1:] == 0).all()
    for k in ("window_sequence", "window_shape", "window_shape_prev", "max_sfb", "flags", "reserved"):
        assert (ch[k] == 0).all()


@pytest.mark.parametrize("n_units", [1, 255, 256, 257])
def test_no_map_one_element(lib, n_units):
    """no map, one CPE a frame: parse errors, moved blocks, another element in the slot, and noise bands with refuse_pns 0 and 1"""
    seen = set()
    for refuse_pns in (0, 1):
        rng = np.random.default_rng(10 * n_units + refuse_pns)
        B = Batch(rng, 1, 2)
        kinds = {}
        for f in range(n_units):
            kind = ["ok", "error", "stale error", "moved", "other element", "pns", "ok"][f % 7] if n_units > 1 else "ok"
            kinds[f] = kind
            B.frame([1] if kind == "other element" else [2], status=PARSE_ERROR if "error" in kind else 0, stale=kind == "stale error")
            if kind == "pns":
                B.frames[f]["flags"][0] |= R.HAS_PNS
        B.finish([(f, 0) for f in range(n_units)])
        for f, kind in kinds.items():
            if kind == "moved":
                B.move(f, 0, "meta_offset" if f % 2 else "coef_offset")
            if kind == "other element":
                B.units["d"]["n_ch"][f] = 2
        want_u, _, refused, taken = check(lib, B, refuse_pns=refuse_pns)
        for f, kind in kinds.items():
            assert taken[f] == (kind == "ok" or (kind == "pns" and not refuse_pns)), (f, kind)
            seen.add((kind, bool(taken[f])))
        assert refused == int((~taken).sum())
        assert_silent(want_u[~taken])
        if taken.sum() > 8:
            assert want_u["d"]["flags"][taken].any()
    if n_units >= 255:
        assert seen == {("ok", True), ("error", False), ("stale error", False), ("moved", False), ("other element", False), ("pns", True), ("pns", False)}


def test_no_map_two_slots(lib):
    """no map, max_units 2, layout (SCE, CPE): frames with n_units 1 whose slot 1 is garbage — 0xFF, or a stale record that would
    match — and is refused for its own sake while slot 0 is taken; a frame whose elements are the other way round"""
    rng = np.random.default_rng(3)
    B = Batch(rng, 2, 3)
    kinds = {}
    for f in range(140):
        kind = ["ok", "one unit", "one unit, stale", "swapped", "ok", "none, stale"][f % 6]
        kinds[f] = kind
        if kind == "swapped":
            B.frame([2, 1])
        else:
            B.frame([1, 2], n_units=0 if "none" in kind else 1 if "one unit" in kind else 2, stale="stale" in kind)
    B.finish([(f, e) for f in range(140) for e in range(2)])
    for f, kind in kinds.items():
        if kind == "swapped":                                   # the plan was made for (SCE, CPE) in channels 0 and 1..2
            B.units["d"]["n_ch"][2 * f:2 * f + 2] = [1, 2]
            B.units["d"]["channel"][2 * f:2 * f + 2] = [0, 1]
    want_u, _, refused, taken = check(lib, B)
    assert len(B.units) == 280
    seen = set()
    for f, kind in kinds.items():
        a, b = bool(taken[2 * f]), bool(taken[2 * f + 1])
        assert (a, b) == {"ok": (True, True), "one unit": (True, False), "one unit, stale": (True, False), "swapped": (False, False), "none, stale": (False, False)}[kind], (f, kind)
        seen.add(kind)
    assert len(seen) == 5 and refused == int((~taken).sum())
    assert_silent(want_u[~taken])


FIVE = [1, 2, 2, 2, 1]          # five elements in eight channels


def five_batch(rng, faults):
    """52 frames of FIVE = 260 plan units through a map, max_units 8.  faults: frame -> "element k" (that element's blocks moved in
    the plan), "error" (a parse error, records 0xFF), "stale error" (records that would match), "fewer" / "more" (n_units 4 / 6,
    every listed element matching), "pns k" (noise bands in element k)"""
    B = Batch(rng, 8, 8)
    for f in range(52):
        ft = faults.get(f, "")
        B.frame(FIVE, status=PARSE_ERROR if "error" in ft else 0, n_units=4 if ft == "fewer" else 6 if ft == "more" else 5, stale=ft in ("stale error", "fewer", "more"))
        if ft.startswith("pns"):
            B.frames[f]["flags"][int(ft[-1])] |= R.HAS_PNS
    B.finish([(f, e) for f in range(52) for e in range(5)], want=5, listed=rng.integers(0, 2, 260) * 5)      # listed: 0 = all, or 5
    for f, ft in faults.items():
        if ft.startswith("element"):
            B.move(f, int(ft[-1]), ["coef_offset", "meta_offset", "channel", "n_ch"][f % 4])
    return B


@pytest.mark.parametrize("where", [0, 2, 4], ids=["first", "middle", "last"])
def test_map_whole_frames(lib, where):
    """map, five elements in eight channels, 52 frames = 260 units: frame 51 starts at lane 255, so its first lane and its other
    four are in different workgroups.  A fault in one element only — the first, a middle or the last — in frame 0, 50, 51 (= the
    last): the whole frame silent, counted once, LAYOUT; a parse-error frame keeps its status and is counted once; a wrong element
    count refuses a frame whose listed elements all match"""
    rng = np.random.default_rng(50 + where)
    faults = {0: "element %d" % where, 50: "element %d" % where, 51: "element %d" % where, 7: "error", 8: "stale error", 20: "fewer", 21: "more", 30: "pns %d" % where}
    B = five_batch(rng, faults)
    assert 51 * 5 == 255 and len(B.units) == 260
    want_u, want_r, refused, taken = check(lib, B)
    per_frame = taken.reshape(52, 5)
    assert (per_frame.all(axis=1) | ~per_frame.any(axis=1)).all(), "a frame is taken or refused as a whole"
    assert sorted(np.nonzero(~per_frame[:, 0])[0]) == sorted(faults) and refused == len(faults)
    for f in range(52):
        ft = faults.get(f, "")
        assert int(want_r["status"][f]) == (PARSE_ERROR if "error" in ft else R.PARSE_LAYOUT if ft else 0)
    assert_silent(want_u[~taken])
    # the same with noise bands taken (a PNS_SPEC stages plan): frame 30 is accepted
    _, r2, n2, t2 = check(lib, B, refuse_pns=0)
    assert n2 == len(faults) - 1 and t2.reshape(52, 5)[30].all() and r2["status"][30] == 0


def test_map_fault_free_and_all_refused(lib):
    """the two ends: nothing refused (no result changes, the counter stays), and every frame refused"""
    rng = np.random.default_rng(60)
    B = five_batch(rng, {})
    _, r, n, taken = check(lib, B)
    assert n == 0 and taken.all() and r.tobytes() == B.res.tobytes()
    B = five_batch(rng, {f: "element %d" % (f % 5) for f in range(52)})
    _, r, n, taken = check(lib, B)
    assert n == 52 and not taken.any() and (r["status"] == R.PARSE_LAYOUT).all()


def test_map_listed_fewer_than_wanted(lib):
    """map, SCE + CPE + CPE in four channels, two of three listed (the reference drops the elements beyond the channel count): a
    mismatch in the unlisted third element does not refuse the frame; n_units == 2 refuses it although both listed elements match
    (and so does 4); a mismatch in a listed element refuses it"""
    rng = np.random.default_rng(70)
    B = Batch(rng, 4, 5)
    kinds = {}
    for f in range(130):
        kind = ["ok", "third differs", "two units", "four units", "second moved", "third garbage", "ok"][f % 7]
        kinds[f] = kind
        B.frame([1, 2, 2], n_units={"two units": 2, "four units": 4}.get(kind, 3), stale=kind in ("two units", "four units"))
        if kind == "third differs":                             # an LFE where the plan's stream has a CPE: nobody listed it
            B.frames[f]["n_ch"][2] = 1
            B.frames[f]["coef_offset"][2] += 7
        if kind == "third garbage":
            B.frames[f][2:3] = np.frombuffer(b"\xff" * 64, aacgpu.UNIT_DTYPE)
    B.finish([(f, e) for f in range(130) for e in range(2)], want=3, listed=2, n_out_ch=4)
    for f, kind in kinds.items():
        if kind == "second moved":
            B.move(f, 1)
    assert len(B.units) == 260
    want_u, want_r, refused, taken = check(lib, B)
    seen = set()
    for f, kind in kinds.items():
        ok = kind in ("ok", "third differs", "third garbage")
        assert taken[2 * f] == taken[2 * f + 1] == ok, (f, kind)
        assert int(want_r["status"][f]) == (0 if ok else R.PARSE_LAYOUT)
        seen.add(kind)
    assert len(seen) == 6 and refused == sum(k in ("two units", "four units", "second moved") for k in kinds.values())


def test_map_out_of_order(lib):
    """a map whose parsed_index is out of order: two streams of different layouts (CPE; SCE + CPE + CPE + LFE), the plan lists them
    stream after stream while the parser's frames alternate; faults in both streams"""
    rng = np.random.default_rng(80)
    B = Batch(rng, 4, 6)
    lay = {0: [2], 1: [1, 2, 2, 1]}
    for f in range(80):
        B.frame(lay[f % 2], status=PARSE_ERROR if f in (6, 33) else 0, n_units=3 if f == 41 else None, stale=f == 41)
    picks, want = [], []
    for s in (0, 1):
        for f in range(s, 80, 2):
            picks += [(f, e) for e in range(len(lay[s]))]
            want += [len(lay[s])] * len(lay[s])
    B.finish(picks, want=np.array(want), listed=0)
    B.move(10, 0)
    B.move(79, 3)
    B.move(1, 2, "channel")
    assert len(B.units) == 40 + 160 and (np.diff(B.map["parsed_index"].astype(np.int64)) < 0).any()
    want_u, want_r, refused, taken = check(lib, B)
    bad = {6, 33, 41, 10, 79, 1}
    assert refused == len(bad)
    for (f, e), t in zip(picks, taken):
        assert t == (f not in bad)
    assert {int(want_r["status"][f]) for f in (41, 10, 79, 1)} == {R.PARSE_LAYOUT} and int(want_r["status"][6]) == PARSE_ERROR


@pytest.mark.parametrize("keep_tns", [0, 1])
def test_keep_tns(lib, keep_tns):
    """records that carry AACG_CHAN_TNS_PRESENT and a non-zero tns_offset, with and without a map: the flag and the offset stay with
    keep_tns and go without it; a refused unit has neither"""
    rng = np.random.default_rng(90 + keep_tns)
    for mapped in (False, True):
        B = Batch(rng, 2, 3)
        for f in range(40):
            B.frame([1, 2], status=PARSE_ERROR if f == 5 else 0)
            if f != 5:
                B.frames[f]["ch"]["flags"][:, :] = [[0xff, 0x01], [0x01, 0xfe]] if f % 2 else [[0x01, 0x00], [0x03, 0x01]]
                B.frames[f]["tns_offset"] = [0x80000001 + f, 3 * f + 1]
        B.finish([(f, e) for f in range(40) for e in range(2)], want=2 if mapped else None, listed=0)
        B.move(9, 1)
        want_u, _, _, taken = check(lib, B, keep_tns=keep_tns)
        assert taken.sum() == (76 if mapped else 77)
        flags = want_u["d"]["ch"]["flags"][taken]
        if keep_tns:
            assert (flags == B.parsed["ch"]["flags"][B.index()][taken]).all() and (flags & R.TNS_PRESENT).any()
            assert (want_u["d"]["tns_offset"][taken] == B.parsed["tns_offset"][B.index()][taken]).all() and (want_u["d"]["tns_offset"][taken] != 0).all()
        else:
            assert not (flags & R.TNS_PRESENT).any() and (flags == B.parsed["ch"]["flags"][B.index()][taken] & 0xfe).all() and (flags & 0xfe).any()
            assert (want_u["d"]["tns_offset"] == 0).all()
        assert_silent(want_u[~taken])


def test_group_maps(lib):
    """all 128 ways to cut eight windows into groups, in CPEs and in SCEs whose unused second channel claims EIGHT_SHORT too
    (gmap[1] stays 0); group lengths that sum past eight windows and short of them; long windows with short-looking groups"""
    rng = np.random.default_rng(100)
    cuts = R.cuts()
    assert len(cuts) == 128 and len({tuple(c) for c in cuts}) == 128 and all(sum(c) == 8 for c in cuts)
    extra = [[3, 4, 5, 2], [8, 8], [2] * 8, [7, 7, 7, 7, 7, 7, 7, 7], [3, 2], [1], [255, 1]]
    B = Batch(rng, 2, 3)
    for k, lens in enumerate(cuts + extra):
        B.frame([1, 2], window=R.EIGHT_SHORT, groups=lens)
    for k in range(4):                                          # ONLY_LONG .. LONG_STOP with grouping bytes of a short frame
        f = B.frame([1, 2], window=[0, 1, 3, 0][k])
        B.frames[f]["ch"]["group_count"] = 3
        B.frames[f]["ch"]["group_len"][..., :3] = [3, 4, 1]
    n = len(B.frames)
    B.finish([(f, e) for f in range(n) for e in range(2)], want=2, listed=2)
    want_u, _, refused, taken = check(lib, B)
    assert refused == 0 and taken.all()
    for k, lens in enumerate(cuts):
        group_of = np.repeat(np.arange(len(lens)), lens)
        word = int(sum(int(g) << (4 * w) for w, g in enumerate(group_of)))
        assert want_u["gmap"][2 * k].tolist() == [word, 0], "an SCE's second channel has no group map"
        assert want_u["gmap"][2 * k + 1].tolist() == [word, word]
        assert (want_u["d"]["ch"]["window_sequence"][2 * k] == R.EIGHT_SHORT).all()
    assert len({int(g) for g in want_u["gmap"][1:256:2, 0]}) == 128
    assert want_u["gmap"][2 * 128 + 1, 0] == 0x21111000 and want_u["gmap"][2 * 129 + 1, 0] == 0 and want_u["gmap"][2 * 130 + 1, 0] == 0x33221100
    assert want_u["gmap"][2 * 132 + 1, 0] == 0x00011000 and want_u["gmap"][2 * 133 + 1, 0] == 0
    assert (want_u["gmap"][2 * (n - 4):] == 0).all()


def test_refresh_under_sanitizers(tmp_path):
    """the same driver as a program of its own, built with -fsanitize=address,undefined and run as a child process: the map cases —
    260 units across the workgroup edge, two of three elements listed, group lengths that sum past eight windows — over heap blocks
    of exactly n_units records, n_frames * max_units parsed records and n_frames results.  The sanitizers' runtimes are linked into
    the program: nothing is preloaded."""
    exe = str(tmp_path / "refresh_emu_san")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fno-strict-aliasing", "-DAACG_EMU_BUILD", "-DREFRESH_EMU_MAIN", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-I", os.path.join(HERE, "emu"), "-pthread", "-Wall", "-Wno-unused-function",
           "-Wno-unknown-pragmas", "-o", exe, os.path.join(HERE, "emu", "refresh_emu.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "refresh_emu: ok" in r.stdout, r.stdout + r.stderr
