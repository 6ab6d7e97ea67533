"""Forced wave and workgroup schedules on the run kernels' hand-offs (imdct_run_body): the LDS flags between the waves of a
workgroup (tails flag, and the slot ring of the eight-wave body), the rendezvous cell between the workgroups of a chain, and the
cross-launch cells of aacg_decode_pipelined.  The lane emulator's schedule-controlled mode (tests/emu/devport_emu.h) runs ONE
wave at a time and picks the next by a policy, all linked workgroups resident together:

  natural         lowest (launch, workgroup, wave) first
  reversed        highest first: consumers before producers, every wait really blocks
  straggler(k)    wave k of every workgroup only when nobody else can run: the producer as late as the protocol allows
  sprinter(k)     wave k first whenever it can run: a second task as far ahead as the flags allow
  random(seed, d) seeded priorities, d priority drops at random turns (probabilistic concurrency testing)
  cell(a, v)      at rendezvous cell a: v = 1 both sides load the state word, the publisher swaps first; 2 both load, the consumer
                  swaps first; 3 the consumer's whole visit between the publisher's payload stores and its swap; 4 publisher, then
                  consumer; 5 consumer, then publisher

Reference in every case: the same batch through the emulator in its default mode on the serial route (one decode after the
other, sixteen-wave kernels), which is held to the exact-roots oracle block by block here as well (parity.assert_blocks), so that a
schedule can never agree with a wrong reference.  Under EVERY schedule the PCM and the final overlap state equal the reference
bit for bit, the output holds no poison, and no decode ends in a deadlock report (emu_lib.EmuDeadlock names who waited for what).

Random schedules: SEEDS per shape, d = 1 + seed % 3 (so each of d = 1, 2, 3 at least five times); every named policy always.

test_the_explorer_sees_each_fault breaks an emulated primitive (emu_set_fault: the kernel source carries no switch) and states
which policy sees it.  Every decode runs in a child process under a time limit, like tests/test_half_runs_emu.py: a fault in the
emulator itself fails one test instead of taking the run down."""
import os
import pickle
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aac.js_amd", "python"))
import aacgpu_workload as W  # noqa: E402
import emu_lib  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
HALF = "libaacg_emu_half.so"    # tests/emu/half_emu.cpp: the rendezvous kernels of f32 PCM on the eight-wave body (tests/emu/Makefile)
WIDE = ("cpe", "cpe", "cpe", "sce")
SEEDS = 16
RK_QUANT, RK_RV = 1, 32         # AACG_RK_* (aacg_routes.h)
CHILD_LIMIT_S = 900


@pytest.fixture(scope="module")
def libs():
    return emu_lib.Emu(), emu_lib.Emu(HALF)       # built once, before the children load them


def _in_child(fn_name, *args):
    """Runs this module's fn_name(*args) in a fresh Python process under a time limit and returns its result."""
    with tempfile.TemporaryDirectory() as d:
        a, r = os.path.join(d, "args.pkl"), os.path.join(d, "result.pkl")
        with open(a, "wb") as f:
            pickle.dump((fn_name, args), f)
        code = ("import pickle, sys; sys.path.insert(0, %r); import test_schedules_emu as m; "
                "fn, args = pickle.load(open(%r, 'rb')); pickle.dump(getattr(m, fn)(*args), open(%r, 'wb'))") % (HERE, a, r)
        try:
            subprocess.run([sys.executable, "-c", code], check=True, timeout=CHILD_LIMIT_S, cwd=HERE)
        except subprocess.TimeoutExpired:
            pytest.fail("%s%r did not finish in %d s" % (fn_name, args, CHILD_LIMIT_S))
        with open(r, "rb") as f:
            return pickle.load(f)


def _bits(a):
    a = np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _randoms(n=SEEDS):
    return [("random", seed, 1 + seed % 3) for seed in range(1, n + 1)]


def _sweep(emu, schedules, decode, want, what):
    """decode() under every schedule: the outputs (a list of arrays) bit for bit `want`, no deadlock.  The natural schedule runs
    first; its number of turns is the span the random schedules draw their change points from.  Returns turns per schedule."""
    failures, turns, span = [], {}, 0
    for sch in [("natural",)] + [s for s in schedules if s != ("natural",)]:
        emu.set_schedule(sch, span)
        try:
            got = decode()
        except emu_lib.EmuDeadlock as e:
            failures.append("%r: %s" % (sch, e))
            continue
        finally:
            emu.set_schedule(None)
        turns[sch] = emu.sched_steps()
        if sch == ("natural",):
            span = turns[sch]
        assert len(got) == len(want)
        for i, (g, w) in enumerate(zip(got, want)):
            if not _same(g, w):
                g, w = np.asarray(g).ravel(), np.asarray(w).ravel()
                bad = np.flatnonzero(_bits(g) != _bits(w))
                failures.append("%r: output %d differs in %d values, the first at %d (block %d); %d NaN" %
                                (sch, i, len(bad), bad[0], bad[0] // 1024, int(np.isnan(g.astype(np.float64)).sum())))
                break
    assert not failures, "%s:\n%s" % (what, "\n".join(failures))
    return turns


def _reference(full, units, coeffs_list, meta, n_pcm, S, C, si=3, exact_of=None, **kw):
    """The serial route in the emulator's default mode, one decode after the other: [PCM of every batch] + [final overlap state].
    exact_of: the quantised coefficients and band words of the batches, to hold the reference to the exact-roots oracle"""
    import orc
    import parity
    pool, par = emu_lib.new_pool(S, C)
    out = [full.decode(units, c, meta, n_pcm, pool, par, sample_index=si, **kw) for c in coeffs_list]
    if exact_of is not None:
        oracle = orc.load()
        ov = np.zeros((S, C, 1024), np.float32)
        for pcm, (q, m) in zip(out, exact_of):
            exact = parity.exact_reference(oracle, units, q, m, n_pcm, ov, sample_index=si)
            assert not np.isnan(exact).any()
            if pcm.dtype == np.int16:
                parity.assert_blocks_int16(pcm, exact, units, what="the reference of the schedules")
            else:
                assert not np.isnan(pcm).any()
                parity.assert_blocks(pcm, exact, units, what="the reference of the schedules")
    return out + [emu_lib.pool_current(pool, par)]


def _make(layout, S, T, seam, seed, edge_si=None):
    """(units, coefficients of the seam, band words of the seam, quantised coefficients, band words, n_pcm, C, sample index)"""
    import orc
    oracle = orc.load()
    wl = W.make_batch(n_streams=S, n_frames=T, layout=layout, mix=True, intensity=True, seed=seed)
    units, q, meta, si = wl["units"], wl["q"], wl["meta"], 3
    if edge_si is not None:
        import edge_cases as E
        si = edge_si
        units, meta = E.edge_side_info(wl, si, oracle, seed + 1)
        q, _ = E.edge_coeffs(units, meta, si, oracle, seed + 2)
    if seam == "q":
        return units, q, meta, q, meta, wl["n_pcm"], wl["C"], si
    ov = np.zeros((S, wl["C"], 1024), np.float32)
    spec = oracle.decode_batch(units, q, meta, wl["n_pcm"], ov, sample_index=si, want_spec=True)[1].astype(np.float32)
    return units, spec, None, q, meta, wl["n_pcm"], wl["C"], si


# ---- the eight-wave body: tails flags, the ring of seven slots, the rendezvous -----------------------------------------------------
EIGHT = ([("natural",), ("reversed",)] + [("straggler", k) for k in range(8)] + [("sprinter", k) for k in range(8)])
# chains of 1, 8, 9, 15, 16 frames: one run, the ring alone (the rendezvous kernel as a pipelined launch takes it); 17, 33, 48: the
# rendezvous too.  Stereo (make_batch: common windows), mono, mixed and wide layouts, both seams; split windows: the edge batch
HALF_SHAPES = [(("cpe",), 2, 1, "q"), (("cpe",), 1, 8, "f"), (("sce",), 2, 9, "q"), (("cpe",), 1, 15, "q"), (("cpe",), 2, 16, "q"),
               (("sce",), 1, 16, "f"), (("sce", "cpe"), 1, 17, "f"), (("cpe",), 1, 33, "q"), (("sce",), 1, 48, "q"), (("cpe",), 1, 48, "f"),
               (WIDE, 1, 20, "q"), (WIDE, 1, 9, "f")]


@pytest.mark.parametrize("layout,S,T,seam", HALF_SHAPES)
def test_eight_wave_body_under_every_schedule(libs, layout, S, T, seam):
    _in_child("_check_eight", layout, S, T, seam, None)


def test_eight_wave_body_under_every_schedule_at_the_edges(libs):
    """the edge workload (tests/edge_cases.py) at a 15-band rate: short windows, split-window pairs, 120 band records, the
    dequantisation's big-value path"""
    _in_child("_check_eight", ("cpe",), 2, 20, "q", 8)


def _check_eight(layout, S, T, seam, edge_si):
    full, half = emu_lib.Emu(), emu_lib.Emu(HALF)
    units, coeffs, meta, q, qmeta, n_pcm, C, si = _make(layout, S, T, seam, 83 + T, edge_si)
    want = _reference(full, units, [coeffs], meta, n_pcm, S, C, si, exact_of=[(q, qmeta)])

    def decode():
        pool, par = emu_lib.new_pool(S, C)
        pcm = half.decode(units, coeffs, meta, n_pcm, pool, par, sample_index=si, pipelined=True)
        assert all(k & RK_RV for k in half.last_keys()), half.last_keys()       # the kernels half_emu.cpp runs on eight waves
        return [pcm, emu_lib.pool_current(pool, par)]
    return _sweep(half, EIGHT + _randoms(), decode, want, "eight-wave body %r S=%d T=%d seam %s" % (layout, S, T, seam))


# ---- the sixteen-wave body: one recipe per family with a hand-off of its own -------------------------------------------------------
SIXTEEN = [("natural",), ("reversed",), ("straggler", 0), ("straggler", 1), ("straggler", 15)]
FAMILIES = ["quant", "quant_rv", "quant_dd", "quant_ex_rv", "quant_cpl", "f32_rv_i16"]       # recipes of tests/test_route_matrix.py


@pytest.mark.parametrize("name", FAMILIES)
def test_sixteen_wave_body_under_every_schedule(libs, name):
    _in_child("_check_sixteen", name)


def _check_sixteen(name):
    import test_route_matrix as RM
    full = emu_lib.Emu()
    r = RM.BY_NAME[name]
    rec, coeffs = RM.batches(name)
    outs, state, _ = RM.emu_run(name)                  # default mode ...
    RM.check(name, outs, state, "the reference of the schedules")      # ... held to the exact-roots oracle block by block
    want = list(outs) + [state]

    def decode():
        pool, par = emu_lib.new_pool(RM.S, rec["H"])
        got = [full.decode(rec["units"], c, rec["meta"], rec["n_pcm"], pool, par, tns=rec["tns"], pns=r.pns, cce=rec["cce"],
                           int16_out=r.out == RM.O16, unfused=bool(r.debug & RM.UNFUSED), rv=0 if r.debug & RM.RECOMP else 1,
                           pipelined=r.piped, poison=0x7F7F if r.out == RM.O16 else None) for c in coeffs]
        return got + [emu_lib.pool_current(pool, par)]
    return _sweep(full, SIXTEEN + _randoms(), decode, want, "sixteen-wave body, recipe %s" % name)


# ---- the rendezvous between the runs of a chain: every order at every cell ---------------------------------------------------------
@pytest.mark.parametrize("body,int16", [("sixteen", False), ("sixteen", True), ("eight", False)])      # (the eight-wave body stores f32 only)
@pytest.mark.parametrize("layout,T", [(("cpe",), 40), (WIDE, 20)])
def test_every_order_at_every_rendezvous_cell(libs, layout, T, body, int16):
    _in_child("_check_cells", layout, T, body, int16)


def _check_cells(layout, T, body, int16):
    full = emu_lib.Emu()
    emu = full if body == "sixteen" else emu_lib.Emu(HALF)
    S = 1
    units, coeffs, meta, q, qmeta, n_pcm, C, si = _make(layout, S, T, "q", 61)
    want = _reference(full, units, [coeffs], meta, n_pcm, S, C, si, exact_of=[(q, qmeta)], int16_out=int16, rv=0)

    def decode():
        pool, par = emu_lib.new_pool(S, C)
        pcm = emu.decode(units, coeffs, meta, n_pcm, pool, par, int16_out=int16)
        return [pcm, emu_lib.pool_current(pool, par)]
    emu.set_schedule(("natural",))
    decode()
    emu.set_schedule(None)
    cells, chains = emu.sched_cells()
    assert cells == chains * ((T + 15) // 16 - 1) and cells >= 2
    return _sweep(emu, [("cell", a, v) for a in range(cells) for v in (1, 2, 3, 4, 5)], decode, want,
                  "rendezvous cells %r T=%d %s-wave body int16=%r" % (layout, T, body, int16))


# ---- cross-launch cells: overlapped launches of one plan ------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,S,T,n,seam", [(("cpe",), 2, 16, 5, "q"), (("cpe",), 1, 37, 4, "q"), (("sce", "cpe"), 1, 18, 3, "f")])
def test_overlapped_launches_under_every_schedule(libs, layout, S, T, n, seam):
    _in_child("_check_launches", layout, S, T, n, seam, False)


def test_window_switching_across_the_launch_boundary_under_every_schedule(libs):
    """EIGHT_SHORT / START / STOP frames at the ends of the chains, as tests/test_xl_emu.py has them"""
    _in_child("_check_launches", ("cpe",), 2, 8, 4, "q", True)


def _check_launches(layout, S, T, n, seam, switching):
    import orc
    oracle = orc.load()
    full, half = emu_lib.Emu(), emu_lib.Emu(HALF)
    base = W.make_batch(n_streams=S, n_frames=T, layout=layout, mix=True, intensity=switching, seed=91 if switching else 97)
    C = base["C"]
    rng = np.random.default_rng(5)
    qs = [base["q"] if j == 0 else np.roll(base["q"], 5 * j, axis=0) if switching else
          (np.roll(base["q"], 37 * j, axis=0) * rng.choice([-1, 1])).astype(np.int16) for j in range(n)]
    ov = np.zeros((S, C, 1024), np.float32)
    if seam == "q":
        coeffs, metas = qs, [base["meta"]] * n
    else:
        coeffs = [oracle.decode_batch(base["units"], x, base["meta"], base["n_pcm"], ov, want_spec=True)[1].astype(np.float32) for x in qs]
        metas = None
    want = _reference(full, base["units"], coeffs, base["meta"] if seam == "q" else None, base["n_pcm"], S, C,
                      exact_of=[(x, base["meta"]) for x in qs])

    def decode():
        pool, par = emu_lib.new_pool(S, C)
        cells = np.full((S, C, emu_lib.OV_BUFFERS, 4), 0x5a5a5a5a5a5a5a5a, np.uint64)
        heads = np.full((S, C, emu_lib.OV_BUFFERS, 1024), np.nan, np.float32)
        got, _ = half.decode_pipelined(base["units"], coeffs, metas, base["n_pcm"], pool, par, cells, heads)
        return got + [emu_lib.pool_current(pool, par)]
    half.set_schedule(("natural",))
    decode()
    half.set_schedule(None)
    chains = half.sched_cells()[1]
    assert chains == S * len(layout)
    # every order at every launch boundary, the chain rotating
    at = [("cell", b * chains + (b + v) % chains, v) for b in range(n - 1) for v in (1, 2, 3, 4, 5)]
    return _sweep(half, [("reversed",)] + at + _randoms(), decode, want,
                  "%d overlapped launches %r S=%d T=%d seam %s" % (n, layout, S, T, seam))


# ---- the profiling build's work-skipping paths must finish ---------------------------------------------------------------------------
@pytest.mark.parametrize("ablate", [2, 8, 10, 32, 64, 128])
def test_eight_wave_profiling_paths_finish_under_forced_schedules(libs, ablate):
    """the AACG_ABL switches of tests/test_half_runs_emu.py under reversed and straggler(0): no deadlock report; their PCM is not
    the product's and is not compared"""
    _in_child("_check_ablate", ablate)


def _check_ablate(ablate):
    half = emu_lib.Emu(HALF)
    wl = W.make_batch(n_streams=2, n_frames=40, layout=("cpe",), mix=True, seed=5)
    half.lib.emu_half_set_ablate(ablate)
    try:
        for sch in (("reversed",), ("straggler", 0)):
            half.set_schedule(sch)
            pool, par = emu_lib.new_pool(2, wl["C"])
            half.decode(wl["units"], wl["q"], wl["meta"], wl["n_pcm"], pool, par)
            pool, par = emu_lib.new_pool(2, wl["C"])
            cells = np.full((2, wl["C"], emu_lib.OV_BUFFERS, 4), 0x5a5a5a5a5a5a5a5a, np.uint64)
            heads = np.full((2, wl["C"], emu_lib.OV_BUFFERS, 1024), np.nan, np.float32)
            half.decode_pipelined(wl["units"], [wl["q"]] * 3, [wl["meta"]] * 3, wl["n_pcm"], pool, par, cells, heads)
    finally:
        half.set_schedule(None)
        half.lib.emu_half_set_ablate(0)
    return True


# ---- teeth: a broken hand-off is seen ----------------------------------------------------------------------------------------------------
def test_the_same_schedule_makes_the_same_choices(libs):
    assert _in_child("_check_repeatable")


def _check_repeatable():
    half = emu_lib.Emu(HALF)
    units, coeffs, meta, _, _, n_pcm, C, si = _make(("cpe",), 1, 33, "q", 7)
    turns = []
    for sch in [("random", 3, 3), ("random", 3, 3), ("random", 4, 3), ("reversed",), ("reversed",)]:
        half.set_schedule(sch, 600)
        pool, par = emu_lib.new_pool(1, C)
        half.decode(units, coeffs, meta, n_pcm, pool, par, pipelined=True)
        half.set_schedule(None)
        n = half.lib.emu_sched_trace(None, 0)
        t = np.zeros(n, np.int64)
        half.lib.emu_sched_trace(t.ctypes.data, n)
        turns.append(t)
    assert len(turns[0]) > 100
    assert np.array_equal(turns[0], turns[1]) and np.array_equal(turns[3], turns[4])     # the same (policy, seed): the same turns
    assert not np.array_equal(turns[0], turns[2]) and not np.array_equal(turns[0], turns[3])
    return True


def test_the_explorer_sees_each_fault(libs):
    """A fault in an emulated primitive, and the policy that sees it (different bits, poison in the PCM or a deadlock report),
    while `natural` on the mended primitive passes:
      (a) the slot-ring wait of the eight-wave body skipped for task 8 (it works in slot 1 without waiting for task 2 to have read
          task 1's tails there)                                   seen by sprinter(0): wave 0 starts task 8 before wave 1 runs
      (b) the tails flag of task 3 seen early by its consumer, task 4 (wave 4)
                                                                  seen by straggler(3): task 3's tails are not there yet
      (c) blind_cas: the swap on the rendezvous word a plain store that reports success
                                                                  seen by cell(0, 1) and cell(0, 2): both sides believe they won
      (d) the tails flag of task 3 never raised                   every policy: a deadlock report that names task 4's wait"""
    seen = _in_child("_check_faults")
    assert seen == {"a": True, "b": True, "c1": True, "c2": True, "d": True}, seen


def _check_faults():
    full, half = emu_lib.Emu(), emu_lib.Emu(HALF)
    out = {}

    def notices(emu, decode, want, sch):
        emu.set_schedule(sch)
        try:
            got = decode()
        except emu_lib.EmuDeadlock:
            return True
        finally:
            emu.set_schedule(None)
        return not all(_same(g, w) for g, w in zip(got, want)) or bool(np.isnan(got[0]).any())

    # (a), (b), (d): one run of 16 stereo frames on the eight-wave body
    units, coeffs, meta, q, qmeta, n_pcm, C, si = _make(("cpe",), 1, 16, "q", 83)
    want = _reference(full, units, [coeffs], meta, n_pcm, 1, C, si, exact_of=[(q, qmeta)])

    def one_run():
        pool, par = emu_lib.new_pool(1, C)
        return [half.decode(units, coeffs, meta, n_pcm, pool, par, pipelined=True), emu_lib.pool_current(pool, par)]
    flags = half.flags_offset(quant=True, half=True)
    ring_wait_of_task_8 = flags + 4 * (16 + 8 - 7 + 1)          # flags[AACG_WG_WAVES + task - AACG_HALF_SLOTS + 1]
    assert not notices(half, one_run, want, ("natural",))
    half.set_fault("skip_wait", ring_wait_of_task_8, ring_wait_of_task_8 + 4)
    out["a"] = notices(half, one_run, want, ("sprinter", 0))
    half.set_fault("early_set", flags + 4 * 3, flags + 4 * 4, wave=4)
    out["b"] = notices(half, one_run, want, ("straggler", 3))
    half.set_fault("lost_set", flags + 4 * 3, flags + 4 * 4)
    half.set_schedule(("natural",))
    try:
        one_run()
        out["d"] = False
    except emu_lib.EmuDeadlock as e:
        out["d"] = "workgroup 0 wave 4 task 4: dp_flag_wait on the flag at LDS byte %d (flags[3]) for value 1, it holds 0" % (flags + 12) in str(e)
    half.set_schedule(None)
    half.set_fault(None)
    assert not notices(half, one_run, want, ("sprinter", 0)) and not notices(half, one_run, want, ("straggler", 3))

    # (c): a chain of 40 stereo frames, two rendezvous cells
    units, coeffs, meta, q, qmeta, n_pcm, C, si = _make(("cpe",), 1, 40, "q", 61)
    want = _reference(full, units, [coeffs], meta, n_pcm, 1, C, si, exact_of=[(q, qmeta)])

    def chain():
        pool, par = emu_lib.new_pool(1, C)
        return [half.decode(units, coeffs, meta, n_pcm, pool, par), emu_lib.pool_current(pool, par)]
    assert not notices(half, chain, want, ("natural",))
    half.set_fault("blind_cas")
    out["c1"] = notices(half, chain, want, ("cell", 0, 1))
    out["c2"] = notices(half, chain, want, ("cell", 0, 2))
    half.set_fault(None)
    assert not notices(half, chain, want, ("cell", 0, 1)) and not notices(half, chain, want, ("cell", 0, 2))
    return out
