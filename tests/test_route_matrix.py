"""The route matrix: every registered run kernel (aacgpu.run_kernels(): 14 sets of switches x both input seams) and every helper
launch of a route, each reached by a small batch recipe whose route is asserted, decoded, and held to the per-block gate against
the exact-roots oracle (tests/parity.py) as well as the batch rms() against the reference's oracle.

A recipe names the input seam, the output kind, the layout, streams x frames, the optional stages (TNS, PNS: add_tns, add_pns),
coupling elements (add_cce: points), the debug route, serial or pipelined, and the route that takes.  How a switch is reached
(aacg_pick_route, aac.js_amd/csrc/aacg_routes.cpp):
  _nt   at least half of the units are in frames of more than two channels (WIDE: 7 channels)
  _rv   a chain longer than 16 frames, or any pipelined launch
  _dd   a later run of 16 frames (T >= 32) with DEBUG_ROUTE_RECOMPUTE, or in a batch with coupling elements
  _ex   TNS or (int16 seam) PNS on an f32-output engine
  _cpl  independent coupling (point 2), fused
The table is minimal: every recipe is the only one to reach some kernel (test_every_recipe_is_needed), so that a kernel
registered later without a recipe, or a recipe deleted, fails test_every_kernel_is_reached_on_the_device.  A kernel counts where
it runs the batch's channels: the plain kernel's pass over the coupling elements does not.

The same recipes run through the lane emulator in the CPU suite: the keys it dispatched by are the route's, and between them
they are every registered key, the non-temporal bit included.

Each recipe also runs on the edge workload (tests/edge_cases.py: the side info and coefficients of the same skeleton rewritten
to the format's corners) at every distinct band table: on the device all of them at every SAMPLE_INDICES entry, in the emulator
each once with the sample index rotating and one recipe per optional stage at all of them."""
import collections
import functools

import numpy as np
import pytest

import aacgpu as A
import aacgpu_workload as W
import edge_cases as E
import parity

Q, F = "q", "f"
O32, O16 = "f32", "i16"
ST, WIDE = ("cpe",), ("cpe", "cpe", "cpe", "sce")
RECOMP, UNFUSED = A.DEBUG_ROUTE_RECOMPUTE, A.DEBUG_ROUTE_UNFUSED_COUPLING
HELPERS = {"copy", "aacg_spectral_ex_quant", "aacg_spectral_ex_f32", "aacg_couple_spec", "aacg_couple_pcm"}
S = 3
S_INDEX = 3                     # the sample index of the make_batch workload (48 kHz)

Recipe = collections.namedtuple("Recipe", "name seam out layout T tns pns cce debug piped route")
_R = "aacg_imdct_run_"
RECIPES = [
    Recipe("quant", Q, O32, ST, 8, False, False, (), 0, False, _R + "quant"),
    Recipe("f32", F, O32, ST, 8, False, False, (), 0, False, _R + "f32"),
    Recipe("quant_nt_unfused", Q, O32, WIDE, 8, False, False, (2,), UNFUSED, False,
           _R + "quant_nt + " + _R + "quant (coupling elements) + aacg_couple_pcm"),
    Recipe("f32_nt", F, O32, WIDE, 8, False, False, (), 0, False, _R + "f32_nt"),
    Recipe("quant_rv", Q, O32, ST, 40, False, False, (), 0, False, _R + "quant_rv"),
    Recipe("f32_rv_piped", F, O32, ST, 8, False, False, (), 0, True, _R + "f32_rv"),
    Recipe("quant_rv_nt_piped", Q, O32, WIDE, 8, False, False, (), 0, True, _R + "quant_rv_nt"),
    Recipe("f32_rv_nt", F, O32, WIDE, 24, False, False, (), 0, False, _R + "f32_rv_nt"),
    Recipe("quant_i16", Q, O16, ST, 8, False, False, (), 0, False, _R + "quant_i16"),
    Recipe("quant_tns_i16", Q, O16, ST, 8, True, False, (), 0, False, "aacg_spectral_ex_quant + " + _R + "f32_i16"),
    Recipe("quant_i16_nt", Q, O16, WIDE, 8, False, False, (), 0, False, _R + "quant_i16_nt"),
    Recipe("f32_i16_nt", F, O16, WIDE, 8, False, False, (), 0, False, _R + "f32_i16_nt"),
    Recipe("quant_rv_i16_piped", Q, O16, ST, 8, False, False, (), 0, True, _R + "quant_rv_i16"),
    Recipe("f32_rv_i16", F, O16, ST, 24, False, False, (), 0, False, _R + "f32_rv_i16"),
    Recipe("quant_rv_i16_nt", Q, O16, WIDE, 20, False, False, (), 0, False, _R + "quant_rv_i16_nt"),
    Recipe("f32_rv_i16_nt_piped", F, O16, WIDE, 8, False, False, (), 0, True, _R + "f32_rv_i16_nt"),
    Recipe("quant_dd", Q, O32, ST, 32, False, False, (), RECOMP, False, _R + "quant_dd"),
    Recipe("quant_dd_i16", Q, O16, ST, 32, False, False, (), RECOMP, False, _R + "quant_dd_i16"),
    Recipe("f32_dd_i16_wide", F, O16, WIDE, 32, False, False, (), RECOMP, False, _R + "f32_dd_i16"),
    Recipe("quant_ex", Q, O32, ST, 8, True, True, (), 0, False, _R + "quant_ex"),
    Recipe("f32_ex_wide", F, O32, WIDE, 8, True, False, (), 0, False, _R + "f32_ex"),
    Recipe("quant_ex_rv", Q, O32, ST, 24, False, True, (), 0, False, _R + "quant_ex_rv"),
    Recipe("f32_ex_rv_piped", F, O32, ST, 8, True, False, (), 0, True, _R + "f32_ex_rv"),
    Recipe("quant_cpl", Q, O32, ST, 8, False, False, (2,), 0, False, _R + "quant (coupling elements) + " + _R + "quant_cpl"),
    Recipe("f32_cpl", F, O32, ST, 8, False, False, (2,), 0, False, _R + "f32 (coupling elements) + " + _R + "f32_cpl"),
    Recipe("quant_cpl_nt", Q, O32, WIDE, 8, False, False, (2,), 0, False, _R + "quant (coupling elements) + " + _R + "quant_cpl_nt"),
    Recipe("f32_cpl_nt", F, O32, WIDE, 8, False, False, (2,), 0, False, _R + "f32 (coupling elements) + " + _R + "f32_cpl_nt"),
    Recipe("f32_dd_dependent_coupling_tns", F, O32, ST, 32, True, False, (0, 1), 0, False,
           "copy + aacg_couple_spec + aacg_spectral_ex_f32 + " + _R + "f32_dd + aacg_couple_pcm"),
]
BY_NAME = {r.name: r for r in RECIPES}
I16 = [r.name for r in RECIPES if r.out == O16]


def launches(route, side=False):
    """the kernel names of a route; side: the coupling elements' pass of the plain kernel too"""
    out = []
    for k in route.split(" + "):
        if k.endswith(" (coupling elements)"):
            if side:
                out.append(k[:-len(" (coupling elements)")])
            continue
        out.append(k)
    return out


# ---- the batches of a recipe ------------------------------------------------------------------------------------------------
MAKE, EDGE = "make", "edge"     # the workloads: make_batch(mix=True, intensity=True) at sample index 3, or tests/edge_cases.py


def _spectra(oracle, units, q, meta, n_pcm, H, si=3):
    """The f32 seam's input: the spectra every element (coupling elements too) dequantises to, before TNS and coupling."""
    cce = (units["flags"] & A.UNIT_CCE) != 0
    _, spec = oracle.decode_batch(units[~cce], q, meta, n_pcm, np.zeros((S, H, 1024), np.float32), sample_index=si, want_spec=True)
    if cce.any():
        mono = units[cce].copy()
        mono["flags"], mono["n_out_ch"], mono["channel"] = 0, 1, 0
        mono["pcm_offset"] = np.arange(len(mono)) * 1024
        _, s2 = oracle.decode_batch(mono, q, meta, len(mono) * 1024, np.zeros((S, 1, 1024), np.float32), sample_index=si,
                                    want_spec=True)
        spec = spec + s2
    return spec.astype(np.float32)


def nan_frames(r, b):
    """The frames (per stream) of batch b that the NaN variant poisons: the last of the first run of 16 (its overlap crosses
    into the next run) in chains longer than a run, else the last frame of batch 0 (its overlap crosses into the next launch
    or decode) and the middle one of batch 1 — never the last frame of batch 1, whose overlap is the state checked."""
    if r.T > 16:
        return 15
    return r.T - 1 if b == 0 else r.T // 2


@functools.lru_cache(maxsize=None)
def batches(name, saturate=False, workload=MAKE, si=S_INDEX, nan=False):
    """Two consecutive batches of the recipe's streams: the records of the first (units, meta, TNS, coupling) carry on with new
    coefficients in the second (so that one plan serves both).  Returns (dict of the records, [coefficients of batch 0, 1])
    with the f32 seam's spectra made by the oracle.  saturate: every third frame far beyond full scale (scalefactor index 300:
    2^25), both signs.  workload EDGE: the side info and coefficients of tests/edge_cases.py at sample index si on the same
    skeleton (TNS, PNS and coupling elements added after the rewrite, so they see its window info); nan: |q| = 8191 or -32768
    in one frame per stream of each batch (nan_frames)."""
    import orc
    oracle = orc.load()
    r = BY_NAME[name]
    seed = 9000 + 17 * [x.name for x in RECIPES].index(name)
    wl = W.make_batch(n_streams=S, n_frames=r.T, layout=r.layout, mix=True, intensity=True, seed=seed)
    if workload == EDGE:
        units, meta = E.edge_side_info(wl, si, oracle, seed + 5)
        q, at = E.edge_coeffs(units, meta, si, oracle, seed + 6)
        q1, _ = E.edge_coeffs(units, meta, si, oracle, seed + 7, start=at)
        if nan:
            L = len(r.layout)
            q, q1 = [E.edge_nan(x, units, meta, L, si, oracle, [s * r.T + nan_frames(r, b) for s in range(S)])
                     for b, x in enumerate((q, q1))]
        wl = dict(wl, units=units, meta=meta, q=q)
    else:
        assert si == S_INDEX and not nan
        q1 = W.make_batch(n_streams=S, n_frames=r.T, layout=r.layout, mix=True, intensity=True, seed=seed + 3, frame_base=r.T)["q"]
    units, q, meta, tns, cce = wl["units"], wl["q"], wl["meta"], None, None
    if r.tns:
        units, tns = W.add_tns(wl, seed=seed + 1)
    if r.pns:
        units, meta = W.add_pns(dict(wl, units=units), seed=seed + 2)
        if workload == EDGE:
            meta = E.level_noise(units, meta, si, oracle)
    qs = [q, q1]
    if r.cce:
        blocks = q.shape[0]
        units, qc, meta, cce = W.add_cce(dict(wl, units=units, meta=meta), points=r.cce, seed=seed + 4)
        qs = [qc, np.concatenate([q1, qc[blocks:]])]
    if saturate:
        meta = meta.copy()
        qs = [x.copy() for x in qs]
        for i, u in enumerate(units):
            f = int(u["pcm_offset"]) // (1024 * int(u["n_out_ch"]))
            if f % 3 != 1:
                continue
            for c in range(int(u["n_ch"])):
                blk = int(u["coef_offset"]) + c
                nb = int(u["ch"]["group_count"][c]) * int(u["ch"]["max_sfb"][c])
                meta[blk, :nb] = (1 << 12) | 300
                for x in qs:
                    x[blk] = 8190 if (f + c) % 2 else -8190
    H = wl["C"] + len(r.cce)
    rec = dict(units=units, meta=meta, tns=tns, cce=cce, H=H, n_pcm=wl["n_pcm"])
    if r.seam == F:
        coeffs = [_spectra(oracle, units, x, meta, wl["n_pcm"], H, si) for x in qs]
        rec["meta"] = None
    else:
        coeffs = qs
    return rec, coeffs


@functools.lru_cache(maxsize=None)
def references(name, saturate=False, workload=MAKE, si=S_INDEX, nan=False):
    """Per batch: (the exact-roots oracle's PCM, the reference oracle's PCM), and the overlap state after both of the reference
    oracle and of the exact-roots oracle."""
    import orc
    oracle = orc.load()
    r = BY_NAME[name]
    rec, coeffs = batches(name, saturate, workload, si, nan)
    ov, ov_x = np.zeros((S, rec["H"], 1024), np.float32), np.zeros((S, rec["H"], 1024), np.float32)
    kw = dict(tns=rec["tns"], pns=r.pns, cce=rec["cce"], sample_index=si)
    out = []
    for c in coeffs:
        exact = parity.exact_reference(oracle, rec["units"], c, rec["meta"], rec["n_pcm"], ov_x, **kw)
        out.append((exact, oracle.decode_batch(rec["units"], c, rec["meta"], rec["n_pcm"], ov, **kw)))
    return out, ov, ov_x


def check(name, outs, state, what, workload=MAKE, si=S_INDEX, nan=False):
    """the per-block gate and the old gates on both batches of a recipe; returns the worst per-block ratios.  nan: NaN (int16:
    -32768) in exactly the samples where the exact-roots oracle has NaN, and the gates on the rest (the batch rms() left out)."""
    from test_gpu_parity import rms
    r = BY_NAME[name]
    rec, _ = batches(name, False, workload, si, nan)
    refs, ov, ov_x = references(name, False, workload, si, nan)
    stages = r.tns or r.pns or bool(r.cce)
    tau_rms, tau_max = (parity.TAU_RMS_STAGES, parity.TAU_MAX_STAGES) if stages else (parity.TAU_RMS, parity.TAU_MAX)
    worst = [0.0, 0.0]
    for b, (got, (exact, ref)) in enumerate(zip(outs, refs)):
        tag = "%s %s (%s workload, sample index %d) batch %d:" % (what, name, workload, si, b)
        holes = np.isnan(exact)
        assert holes.any() == nan and np.array_equal(holes, np.isnan(ref)), tag
        if r.out == O16:
            assert got.dtype == np.int16
            if nan:
                assert np.all(got[holes] == -32768), tag + " NaN stored as -32768"
                got, exact, ref = np.where(holes, 0, got), np.where(holes, 0.0, exact), np.where(holes, 0.0, ref)
            parity.assert_blocks_int16(got, exact, rec["units"], tau_max=tau_max, what=tag)
            # edge frames reach several times full scale, where the reference's float32 roots alone are steps off: there
            # against the exact-roots oracle
            d = got.astype(np.int32) - parity.pcm16(ref if workload == MAKE else exact)
            assert np.abs(d).max() <= 1 and np.count_nonzero(d) <= 1e-2 * d.size, tag
        else:
            assert np.array_equal(np.isnan(got), holes), tag + " NaN where the oracle has NaN, nowhere else"
            w = parity.assert_blocks(got, exact, rec["units"], tau_rms, tau_max, what=tag)
            worst = [max(worst[0], w[0]), max(worst[1], w[1])]
            if not nan:
                assert rms(got, ref) < 1e-5
    if workload == MAKE:
        assert np.abs(state - ov).max() <= 1e-5 * max(1.0, float(np.abs(ov).max())), "%s %s: overlap state" % (what, name)
    else:
        # frames far louder than their neighbours (escape values, TNS gains): against the exact-roots state, channel by channel
        # (the reference's float32 roots alone are 6e-5 of a channel's peak off there)
        peak = np.maximum(1.0, np.abs(ov_x).max(axis=2, keepdims=True))
        assert np.all(np.abs(state - ov_x) <= 1e-5 * peak), "%s %s: overlap state" % (what, name)
    return worst


# ---- CPU: the table itself -------------------------------------------------------------------------------------------------------
def test_every_recipe_is_needed(engine_lib):
    """the routes the recipes name are every registered kernel and every helper launch, and without any one recipe they are not"""
    want = set(A.run_kernels()) | HELPERS
    named = [set(launches(r.route)) for r in RECIPES]
    assert set().union(*named) == want
    for i, r in enumerate(RECIPES):
        rest = set().union(*(n for j, n in enumerate(named) if j != i))
        assert rest != want, "recipe %s reaches nothing the others do not" % r.name


@pytest.mark.parametrize("name", [r.name for r in RECIPES])
def test_the_route_decision_names_the_recipes_route(engine_lib, name):
    """aacg_debug_route over the recipe's flags: the same string the device test asserts through aacg_plan_kernels_ex"""
    r = BY_NAME[name]
    flags = 0
    if r.layout == WIDE:
        flags |= A.ROUTE_PLAN_WIDE_FRAMES
    if r.T > 16:
        flags |= A.ROUTE_PLAN_LONG_CHAINS | (A.ROUTE_PLAN_FULL_LATER_RUNS if r.T >= 32 else 0)
    if r.tns:
        flags |= A.ROUTE_PLAN_TNS
    if r.pns:
        flags |= A.ROUTE_PLAN_PNS
    if 2 in r.cce:
        flags |= A.ROUTE_PLAN_CCE_INDEPENDENT
    if 0 in r.cce or 1 in r.cce:
        flags |= A.ROUTE_PLAN_CCE_DEPENDENT
    got = A.debug_route(A.INPUT_QUANT_I16 if r.seam == Q else A.INPUT_SPEC_F32, A.OUTPUT_I16 if r.out == O16 else A.OUTPUT_F32,
                        flags, r.piped, r.debug)
    assert got == r.route


# ---- CPU: the recipes through the lane emulator --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _emu():
    import emu_lib
    return emu_lib.Emu()


@functools.lru_cache(maxsize=None)
def emu_run(name, saturate=False, out=None, workload=MAKE, si=S_INDEX, nan=False):
    """both batches through the emulator (out: another output kind than the recipe's): ([PCM of batch 0, 1], overlap state,
    [keys dispatched per batch])"""
    import emu_lib
    r = BY_NAME[name]
    i16 = (out or r.out) == O16
    rec, coeffs = batches(name, saturate, workload, si, nan)
    emu = _emu()
    pool, par = emu_lib.new_pool(S, rec["H"])
    outs, keys = [], []
    for c in coeffs:
        outs.append(emu.decode(rec["units"], c, rec["meta"], rec["n_pcm"], pool, par, sample_index=si, tns=rec["tns"], pns=r.pns,
                               cce=rec["cce"], int16_out=i16, unfused=bool(r.debug & UNFUSED), rv=0 if r.debug & RECOMP else 1,
                               pipelined=r.piped, poison=0x7F7F if i16 else None))
        keys.append(emu.last_keys())
    return outs, emu_lib.pool_current(pool, par), keys


@pytest.mark.parametrize("name", [r.name for r in RECIPES])
def test_recipe_in_the_emulator(oracle, engine_lib, name):
    r = BY_NAME[name]
    outs, state, keys = emu_run(name)
    reg = A.run_kernels()
    want = [reg[k] for k in launches(r.route, side=True) if k not in HELPERS]
    assert keys == [want, want], (keys, want)
    check(name, outs, state, "emulator")


def test_the_emulator_dispatches_by_every_registered_key(engine_lib):
    reached = set()
    for r in RECIPES:
        for k in emu_run(r.name)[2]:
            reached |= set(k)
    assert reached == set(A.run_kernels().values())
    assert any(k & A.RK_NT for k in reached)


@pytest.mark.parametrize("name", I16)
def test_int16_is_the_f32_pcm_rounded_in_the_emulator(oracle, name):
    """the int16 recipe's PCM equals the same batch through the f32-output route, rounded (dp_pcm16_pair on the float the f32
    route stores) — bit for bit"""
    a, b = emu_run(name)[0], emu_run(name, out=O32)[0]
    for x, y in zip(a, b):
        assert np.array_equal(x, parity.pcm16(y))


@pytest.mark.parametrize("name", I16)
def test_int16_saturates_in_the_emulator(oracle, name):
    outs = emu_run(name, saturate=True)[0]
    refs = references(name, saturate=True)[0]
    _saturation(outs, refs, name)


def _saturation(outs, refs, name):
    """far beyond full scale: exactly +32767 / -32768 wherever the reference is more than a step beyond it, both signs seen"""
    ends = [False, False]
    for got, (exact, _) in zip(outs, refs):
        x = exact.astype(np.float64) * 32768.0
        hi, lo = x > 32768.0 * 1.001, x < -32768.0 * 1.001
        assert np.all(got[hi] == 32767) and np.all(got[lo] == -32768), name
        ends = [ends[0] or bool(hi.any()), ends[1] or bool(lo.any())]
    assert ends == [True, True], "%s: the saturating frames reach both ends" % name


# ---- CPU: the recipes at the edges of the format, every band table ----------------------------------------------------------
STAGES = ["quant_ex", "f32_ex_wide", "quant_cpl", "f32_dd_dependent_coupling_tns"]   # one recipe per optional stage
WIDE_SHORT = 8                  # a sample index with 15 short bands (8 x 15 = 120 band records) for the int16 twins
NAN = [r.name for r in RECIPES if r.seam == Q]
ROTATION = {r.name: E.SAMPLE_INDICES[i % len(E.SAMPLE_INDICES)] for i, r in enumerate(RECIPES)}


def test_the_other_sample_indices_share_the_band_tables(oracle):
    """SAMPLE_INDICES stand for all twelve: the band tables of 1, 7, 9, 10 are those of 0, 6, 8, 8 (and kTnsMaxBandsLong/Short
    of aacg_plan.cpp agree on each pair), while the eight differ from each other in a long table, a short table or the TNS limits"""
    for si, same in E.SAME_TABLES.items():
        for is_long in (True, False):
            assert np.array_equal(oracle.swb_offsets(si, is_long), oracle.swb_offsets(same, is_long)), (si, is_long)
    assert sorted(set(E.SAMPLE_INDICES) | set(E.SAME_TABLES)) == list(range(12))
    assert set(ROTATION.values()) == set(E.SAMPLE_INDICES)


@pytest.mark.parametrize("si", E.SAMPLE_INDICES)
def test_the_edge_workload_reaches_the_edges(oracle, si):
    """Over the recipes' batches at sample index si: the seam sweep and +-8190 at live codebook positions of every recipe, and
    between them every window-sequence transition, every (shape, previous shape) pair, split and common windows, max_sfb 0, 1 and
    the table's top (long and short; 8 one-window groups with the top short count), every MS mask mode, both intensity books
    with and without the flip, junk beyond the live band words, and the NaN variant's holes"""
    lo, so = E.tables(oracle, si)
    trans, pairs, tops, flags, is_books = set(), set(), set(), set(), set()
    for r in RECIPES:
        rec, qs = batches(r.name, False, EDGE, si)
        u = rec["units"][(rec["units"]["flags"] & A.UNIT_CCE) == 0]
        if r.seam == Q:                                     # (the f32 recipes' spectra are the oracle's of the same sweep)
            seen = E.covered(u, rec["meta"], qs, si, oracle)
            assert set(E.SEAM.tolist()) | {E.ESCAPE, -E.ESCAPE} <= seen, r.name
        ch = u["ch"]
        for c in range(2):
            live = u["n_ch"] > c
            seq = ch["window_sequence"][live, c].astype(int)
            st = u["stream"][live]
            trans |= {(a, b) for a, b, x, y in zip(seq[:-1], seq[1:], st[:-1], st[1:]) if x == y}
            pairs |= set(zip(ch["window_shape"][live, c].tolist(), ch["window_shape_prev"][live, c].tolist()))
            short = seq == 2
            tops |= {("long", int(m)) for m in ch["max_sfb"][live, c][~short]}
            tops |= {("short", int(m), int(g)) for m, g in zip(ch["max_sfb"][live, c][short], ch["group_count"][live, c][short])}
        flags |= set((u["flags"][u["n_ch"] == 2] & 3).tolist())
        if rec["meta"] is not None:
            for x in u[u["n_ch"] == 2]:
                nb = int(x["ch"]["group_count"][1]) * int(x["ch"]["max_sfb"][1])
                ml, mr = rec["meta"][int(x["meta_offset"])], rec["meta"][int(x["meta_offset"]) + 1]
                for b in range(nb):
                    if mr[b] >> 12 in (14, 15):
                        is_books.add((int(mr[b] >> 12), bool(x["flags"] & 2) and bool(ml[b] & 0x400)))
    nl, ns = len(lo) - 1, len(so) - 1
    assert len(trans) == 16 and pairs == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {("long", 0), ("long", 1), ("long", nl), ("short", ns, 8), ("short", 0, 8), ("short", 1, 8)} <= tops, sorted(tops)
    assert flags == {0, 1, 3}                               # split, common without a mask, common with one
    assert is_books == {(14, False), (14, True), (15, False), (15, True)}
    for name in NAN:
        rec, qs = batches(name, False, EDGE, si, True)
        assert all((x == 8191).any() or (x == -32768).any() for x in qs), name


@pytest.mark.parametrize("name", [r.name for r in RECIPES])
def test_recipe_in_the_emulator_at_the_edges(oracle, engine_lib, name):
    """every recipe on the edge workload once, the sample index rotating through SAMPLE_INDICES: same keys (the route), the
    per-block gate, the overlap state"""
    r, si = BY_NAME[name], ROTATION[name]
    outs, state, keys = emu_run(name, workload=EDGE, si=si)
    reg = A.run_kernels()
    want = [reg[k] for k in launches(r.route, side=True) if k not in HELPERS]
    assert keys == [want, want], (keys, want)
    w = check(name, outs, state, "emulator", EDGE, si)
    print("per-block worst %s si %d: rms %.3e max %.3e" % (name, si, w[0], w[1]))


@pytest.mark.parametrize("si", E.SAMPLE_INDICES)
@pytest.mark.parametrize("name", STAGES)
def test_optional_stages_in_the_emulator_at_every_table(oracle, engine_lib, name, si):
    """TNS (TNS_MAX_BANDS by sample index), PNS and dependent and independent coupling walk the bands of the rate"""
    outs, state, _ = emu_run(name, workload=EDGE, si=si)
    w = check(name, outs, state, "emulator", EDGE, si)
    print("per-block worst %s si %d: rms %.3e max %.3e" % (name, si, w[0], w[1]))


@pytest.mark.parametrize("name", ["quant_rv", "quant_rv_nt_piped", "quant_i16", "quant_ex"])
def test_nan_in_the_emulator_at_the_edges(oracle, engine_lib, name):
    """|q| = 8191 / -32768: NaN (int16: -32768) in exactly the oracle's samples, across a run or a launch boundary"""
    outs, state, _ = emu_run(name, workload=EDGE, si=WIDE_SHORT, nan=True)
    check(name, outs, state, "emulator", EDGE, WIDE_SHORT, nan=True)


@pytest.mark.parametrize("name", I16)
def test_int16_is_the_f32_pcm_rounded_in_the_emulator_at_the_edges(oracle, name):
    a, b = emu_run(name, workload=EDGE, si=WIDE_SHORT)[0], emu_run(name, out=O32, workload=EDGE, si=WIDE_SHORT)[0]
    for x, y in zip(a, b):
        assert np.array_equal(x, parity.pcm16(y))


@pytest.mark.parametrize("name", I16)
def test_int16_saturates_in_the_emulator_at_the_edges(oracle, name):
    outs = emu_run(name, saturate=True, workload=EDGE, si=WIDE_SHORT)[0]
    refs = references(name, saturate=True, workload=EDGE, si=WIDE_SHORT)[0]
    _saturation(outs, refs, name)


@pytest.mark.parametrize("si", range(12))
def test_spectral_stage_bit_exact_at_every_sample_index_in_the_emulator(oracle, si):
    """the dequantisation, MS and intensity of the edge workload (seam sweep, 120 band records, 51 long bands) against the
    oracle's spectra, bit for bit"""
    import emu_lib
    for name in ("quant_rv", "quant_i16_nt"):
        rec, qs = batches(name, False, EDGE, E.SAME_TABLES.get(si, si))
        for q in qs:
            _, want = oracle.decode_batch(rec["units"], q, rec["meta"], rec["n_pcm"], np.zeros((S, rec["H"], 1024), np.float32),
                                          sample_index=si, want_spec=True)
            got = _emu().spectral(rec["units"], q, rec["meta"], sample_index=si)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, si)


# ---- GPU: the recipes on the device --------------------------------------------------------------------------------------------
def _engine(r, H, out=None, si=S_INDEX):
    kw = dict(max_streams=S, max_channels=H, output_kind=A.OUTPUT_I16 if (out or r.out) == O16 else A.OUTPUT_F32, sample_index=si)
    if r.tns:
        kw["tns_mode"] = A.TNS_SPEC
    if r.pns:
        kw["pns_mode"] = A.PNS_SPEC
    if r.cce:
        kw["cce_mode"] = A.CCE_SPEC
    eng = A.Engine(A.INPUT_QUANT_I16 if r.seam == Q else A.INPUT_SPEC_F32, **kw)
    eng.debug_set_route(r.debug)
    return eng


def device_run(r, saturate=False, out=None, workload=MAKE, si=S_INDEX, nan=False, host=False):
    """both batches of recipe r through the device path (one plan; aacg_decode_device or aacg_decode_pipelined) into buffers
    poisoned first (NaN, int16 0x7F7F), out: another output kind than the recipe's: ([PCM of batch 0, 1], overlap state, the
    plan's route).  host: through the host-buffer path instead (Engine.decode_batch: aacg_decode_batch / _tns / _ex, so
    aacg_submit_ex; no plan, the route None), for recipes that are not pipelined"""
    import torch
    i16 = (out or r.out) == O16
    rec, coeffs = batches(r.name, saturate, workload, si, nan)
    eng = _engine(r, rec["H"], out, si)
    if host:
        assert not r.piped
        outs = [eng.decode_batch(rec["units"], c, rec["meta"], rec["n_pcm"], tns=rec["tns"], cce=rec["cce"]) for c in coeffs]
        state = np.stack([[eng.get_overlap(s, ch) for ch in range(rec["H"])] for s in range(S)])
        eng.close()
        return outs, state, None
    plan = eng.plan(rec["units"], tns=rec["tns"], cce=rec["cce"])
    route = eng.plan_kernels(plan, pipelined=r.piped)
    d_meta = torch.from_numpy(rec["meta"].view(np.int16)).cuda() if rec["meta"] is not None else None
    outs = []
    for c in coeffs:
        d_in = torch.from_numpy(np.ascontiguousarray(c)).cuda()
        if i16:
            d_pcm = torch.full((rec["n_pcm"],), 0x7F7F, dtype=torch.int16, device="cuda")
        else:
            d_pcm = torch.full((rec["n_pcm"],), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        mp = d_meta.data_ptr() if d_meta is not None else None
        if r.piped:
            eng.decode_pipelined(plan, d_in.data_ptr(), mp, d_pcm.data_ptr())
        else:
            eng.decode_device(plan, d_in.data_ptr(), mp, d_pcm.data_ptr(), 0)
        eng.synchronize()
        torch.cuda.synchronize()
        outs.append(d_pcm.cpu().numpy())
    state = np.stack([[eng.get_overlap(s, ch) for ch in range(rec["H"])] for s in range(S)])
    plan.destroy()
    eng.close()
    return outs, state, route


@pytest.mark.gpu
@pytest.mark.parametrize("name,host", [pytest.param(r.name, h, id=r.name + ("-host" if h else ""))
                                       for r in RECIPES for h in ((False,) if r.piped else (False, True))])
def test_recipe_on_the_device(oracle, name, host):
    """host: the recipe's batches through the host-buffer path as well (every table of the batch through the engine's slot
    buffers): the PCM of both batches and the overlap state bit for bit what the plan gives"""
    r = BY_NAME[name]
    outs, state, route = device_run(r)
    assert route == r.route
    w = check(name, outs, state, "device")
    print("per-block worst %s: rms %.3e max %.3e" % (name, w[0], w[1]))
    if host:
        h_outs, h_state, _ = device_run(r, host=True)
        for b, (x, y) in enumerate(zip(h_outs, outs)):
            assert x.dtype == y.dtype, name
            same = np.array_equal(x, y) if r.out == O16 else np.array_equal(x.view(np.uint32), y.view(np.uint32))
            assert same, "%s batch %d: the host-buffer path's PCM" % (name, b)
        assert np.array_equal(h_state.view(np.uint32), state.view(np.uint32)), "%s: the host-buffer path's overlap state" % name


@pytest.mark.gpu
def test_every_kernel_is_reached_on_the_device(oracle):
    """the launches the engine makes for the recipes' plans are every registered run kernel and the five helper launches"""
    reached = set()
    for r in RECIPES:
        rec, _ = batches(r.name)
        eng = _engine(r, rec["H"])
        plan = eng.plan(rec["units"], tns=rec["tns"], cce=rec["cce"])
        reached |= set(launches(eng.plan_kernels(plan, pipelined=r.piped)))
        plan.destroy()
        eng.close()
    assert reached == set(A.run_kernels()) | HELPERS


@pytest.mark.gpu
@pytest.mark.parametrize("name", I16)
def test_int16_is_the_f32_pcm_rounded_on_the_device(oracle, name):
    """AACG_OUTPUT_I16: dp_pcm16_pair applied to the float the f32 route would store, so the int16 engine's PCM is exactly
    clip(rint(x * 32768)) of the f32 engine's on the same batch, wherever both take the same route apart from the store.

    quant_tns_i16 is the exception: its int16 engine runs the optional stages as a launch of their own (aacg_spectral_ex_quant,
    then f32_i16 on the spectra it leaves in HBM), the f32 engine inside the run kernel (quant_ex).  In the lane emulator the two
    are the same bits; on the device, where the compiler schedules and contracts the two instantiations' multiply-adds each its
    own way, their float PCM differs by rounding — so there the bound is: the rounded f32 PCM, or its neighbour at a sample that
    lies within the optional stages' gate (parity.TAU_MAX_STAGES x s_peak) of a rounding boundary.  (Measured on the MI355X: 2
    of 49152 samples one step apart, both within 1e-3 of a step of the boundary.)"""
    r = BY_NAME[name]
    a, _, _ = device_run(r)
    b, _, route = device_run(r, out=O32)
    assert "_i16" not in route
    rec, _ = batches(name)
    for x, y in zip(a, b):
        ok = ~np.isnan(y)
        if name == "quant_tns_i16":
            assert route == _R + "quant_ex"
            parity.assert_blocks_int16(x, y, rec["units"], tau_max=parity.TAU_MAX_STAGES, what="%s against %s" % (name, route))
            d = x.astype(np.int32) - parity.pcm16(y)
            print("%s against %s: %d of %d samples one step apart" % (name, route, np.count_nonzero(d), d.size))
        else:
            assert np.array_equal(x[ok], parity.pcm16(y[ok])), "%s against %s" % (name, route)


@pytest.mark.gpu
@pytest.mark.parametrize("name", I16)
def test_int16_saturates_on_the_device(oracle, name):
    outs, _, route = device_run(BY_NAME[name], saturate=True)
    assert route == BY_NAME[name].route
    refs = references(name, saturate=True)[0]
    _saturation(outs, refs, name)


# ---- GPU: the recipes at the edges of the format, every band table ----------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("si", E.SAMPLE_INDICES)
@pytest.mark.parametrize("name", [r.name for r in RECIPES])
def test_recipe_on_the_device_at_the_edges(oracle, name, si):
    r = BY_NAME[name]
    outs, state, route = device_run(r, workload=EDGE, si=si)
    assert route == r.route
    w = check(name, outs, state, "device", EDGE, si)
    print("per-block worst %s si %d: rms %.3e max %.3e" % (name, si, w[0], w[1]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAN)
def test_nan_on_the_device_at_the_edges(oracle, name):
    r = BY_NAME[name]
    outs, state, route = device_run(r, workload=EDGE, si=WIDE_SHORT, nan=True)
    assert route == r.route
    check(name, outs, state, "device", EDGE, WIDE_SHORT, nan=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", I16)
def test_int16_is_the_f32_pcm_rounded_on_the_device_at_the_edges(oracle, name):
    """test_int16_is_the_f32_pcm_rounded_on_the_device on the edge workload at a 15-band rate"""
    r = BY_NAME[name]
    a, _, _ = device_run(r, workload=EDGE, si=WIDE_SHORT)
    b, _, route = device_run(r, out=O32, workload=EDGE, si=WIDE_SHORT)
    assert "_i16" not in route
    rec, _ = batches(name, False, EDGE, WIDE_SHORT)
    for x, y in zip(a, b):
        ok = ~np.isnan(y)
        if name == "quant_tns_i16":
            parity.assert_blocks_int16(x, y, rec["units"], tau_max=parity.TAU_MAX_STAGES, what="%s against %s" % (name, route))
        else:
            assert np.array_equal(x[ok], parity.pcm16(y[ok])), "%s against %s" % (name, route)


@pytest.mark.gpu
@pytest.mark.parametrize("name", I16)
def test_int16_saturates_on_the_device_at_the_edges(oracle, name):
    outs, _, route = device_run(BY_NAME[name], saturate=True, workload=EDGE, si=WIDE_SHORT)
    assert route == BY_NAME[name].route
    refs = references(name, saturate=True, workload=EDGE, si=WIDE_SHORT)[0]
    _saturation(outs, refs, name)


@pytest.mark.gpu
@pytest.mark.parametrize("si", range(12))
def test_spectral_stage_bit_exact_at_every_sample_index_on_the_device(oracle, si):
    """Engine.spectral_device on the edge workload (seam sweep, 120 band records, 51 long bands) against the oracle's spectra,
    bit for bit"""
    import torch
    for name in ("quant_rv", "quant_i16_nt"):
        r = BY_NAME[name]
        rec, qs = batches(name, False, EDGE, E.SAME_TABLES.get(si, si))
        eng = A.Engine(A.INPUT_QUANT_I16, max_streams=S, max_channels=rec["H"], sample_index=si)
        plan = eng.plan(rec["units"])
        dm = torch.from_numpy(rec["meta"].view(np.int16)).cuda()
        for q in qs:
            _, want = oracle.decode_batch(rec["units"], q, rec["meta"], rec["n_pcm"], np.zeros((S, rec["H"], 1024), np.float32),
                                          sample_index=si, want_spec=True)
            dq = torch.from_numpy(np.ascontiguousarray(q)).cuda()
            ds = torch.full(dq.shape, float("nan"), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            eng.spectral_device(plan, dq.data_ptr(), dm.data_ptr(), ds.data_ptr(), 0)
            eng.synchronize()
            got = ds.cpu().numpy()
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, si, r.route)
        plan.destroy()
        eng.close()
