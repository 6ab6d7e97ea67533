"""The eight-wave run body (imdct_run_body<..., NW = AACG_HALF_WAVES>, behind aacg_imdct_run_quant_rv): a run of 16 frames on 8 waves,
wave w taking frame w and then frame w + 8, seven LDS slots for sixteen frames.  In the lane emulator (tests/emu/half_emu.cpp: the
unchanged emulator with its f32-PCM rendezvous kernels on that body) it must give the same BITS — PCM and overlap state — as the
16-wave body: chains of 1 to 48 frames, every window sequence (mixed batches), both seams, both workgroup orders of the rendezvous,
and overlapped launches meeting in cross-launch cells in several orders.  Lanes run as threads, so the waves interleave as the OS
schedules them.  The emulator's waits spin without a bound, so every decode here runs in a child process under a time limit: a
wait that could never be met fails the test instead of hanging it.  The profiling build's work-skipping paths (AACG_ABL) of the
body must finish too."""
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
LIB = "libaacg_emu_half.so"
SRC = ["tests/emu/half_emu.cpp", "aac.js_amd/csrc/aacg_tables.cpp", "aac.js_amd/csrc/aacg_plan.cpp",
       "aac.js_amd/csrc/aacg_routes.cpp", "aac.js_amd/csrc/aacg_parse_host.cpp"]


@pytest.fixture(scope="module")
def emus():
    emu_lib.build_driver("aacg_emu_half", SRC, os.path.join(HERE, "emu"))
    return emu_lib.Emu(), emu_lib.Emu(LIB)      # (make finds the half library up to date)


CHILD_LIMIT_S = 600


def _in_child(fn_name, *args):
    """Runs this module's fn_name(*args) in a fresh Python process under a time limit and returns its result."""
    with tempfile.TemporaryDirectory() as d:
        a, r = os.path.join(d, "args.pkl"), os.path.join(d, "result.pkl")
        with open(a, "wb") as f:
            pickle.dump((fn_name, args), f)
        code = ("import pickle, sys; sys.path.insert(0, %r); import test_half_runs_emu as m; "
                "fn, args = pickle.load(open(%r, 'rb')); pickle.dump(getattr(m, fn)(*args), open(%r, 'wb'))") % (HERE, a, r)
        try:
            subprocess.run([sys.executable, "-c", code], check=True, timeout=CHILD_LIMIT_S, cwd=HERE)
        except subprocess.TimeoutExpired:
            pytest.fail("%s did not finish in %d s: a wait in the eight-wave body was never met" % (fn_name, CHILD_LIMIT_S))
        with open(r, "rb") as f:
            return pickle.load(f)


def _cells(S, C):
    cells = np.full((S, C, emu_lib.OV_BUFFERS, 4), 0x5a5a5a5a5a5a5a5a, np.uint64)
    heads = np.full((S, C, emu_lib.OV_BUFFERS, 1024), np.nan, np.float32)
    return cells, heads


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


@pytest.mark.parametrize("layout,S,T,seam", [(("cpe",), 2, 1, "q"), (("cpe",), 1, 5, "q"), (("cpe",), 2, 16, "q"), (("cpe",), 1, 17, "q"),
                                             (("cpe",), 1, 40, "q"), (("sce",), 1, 48, "q"), (("cpe",), 1, 48, "f"), (("sce", "cpe"), 1, 17, "f"),
                                             (("cpe", "cpe", "cpe", "sce"), 1, 20, "q")])
def test_eight_wave_runs_equal_sixteen_wave_runs_bit_for_bit(emus, layout, S, T, seam):
    _in_child("_check_runs", layout, S, T, seam)


def _check_runs(layout, S, T, seam):
    import orc
    oracle = orc.load()
    full, half = emu_lib.Emu(), emu_lib.Emu(LIB)
    wl = W.make_batch(n_streams=S, n_frames=T, layout=layout, mix=True, intensity=True, seed=83 + T)
    C = wl["C"]
    ov = np.zeros((S, C, 1024), np.float32)
    ref, spec = oracle.decode_batch(wl["units"], wl["q"], wl["meta"], wl["n_pcm"], ov, want_spec=True)
    coeffs, meta = (wl["q"], wl["meta"]) if seam == "q" else (spec.astype(np.float32), None)
    pool, par = emu_lib.new_pool(S, C)
    want = full.decode(wl["units"], coeffs, meta, wl["n_pcm"], pool, par, rv=1)
    want_state = emu_lib.pool_current(pool, par)
    d = want.astype(np.float64) - ref
    assert float(np.sqrt(np.mean(d * d))) < 1e-5 and not np.isnan(want).any()
    for rv in (1, 2):                                  # the publishing run first, or the consuming one
        pool, par = emu_lib.new_pool(S, C)
        got = half.decode(wl["units"], coeffs, meta, wl["n_pcm"], pool, par, rv=rv)
        assert _same(got, want), rv
        assert _same(emu_lib.pool_current(pool, par), want_state), rv


@pytest.mark.parametrize("layout,S,T,n,seam", [(("cpe",), 2, 16, 5, "q"), (("cpe",), 1, 37, 4, "q"), (("sce", "cpe"), 1, 18, 3, "f")])
def test_eight_wave_runs_through_cross_launch_cells_bit_for_bit(emus, layout, S, T, n, seam):
    _in_child("_check_cells", layout, S, T, n, seam)


def _check_cells(layout, S, T, n, seam):
    import orc
    oracle = orc.load()
    full, half = emu_lib.Emu(), emu_lib.Emu(LIB)
    base = W.make_batch(n_streams=S, n_frames=T, layout=layout, mix=True, seed=97)
    C = base["C"]
    ov = np.zeros((S, C, 1024), np.float32)
    rng = np.random.default_rng(5)
    coeffs, metas = [], []
    for j in range(n):
        q = base["q"] if j == 0 else (np.roll(base["q"], 37 * j, axis=0) * rng.choice([-1, 1])).astype(np.int16)
        if seam == "q":
            coeffs.append(q)
        else:
            coeffs.append(oracle.decode_batch(base["units"], q, base["meta"], base["n_pcm"], ov, want_spec=True)[1].astype(np.float32))
        metas.append(base["meta"])
    metas = metas if seam == "q" else None
    pool, par = emu_lib.new_pool(S, C)
    serial = [full.decode(base["units"], coeffs[j], metas[j] if metas else None, base["n_pcm"], pool, par) for j in range(n)]
    serial_state = emu_lib.pool_current(pool, par)
    for order in (0, 1, 2, 7):                         # launch after launch, the last of every round first, random interleavings
        pool, par = emu_lib.new_pool(S, C)
        cells, heads = _cells(S, C)
        got, _ = half.decode_pipelined(base["units"], coeffs, metas, base["n_pcm"], pool, par, cells, heads, order=order)
        for j in range(n):
            assert _same(got[j], serial[j]), (order, j)
        assert _same(emu_lib.pool_current(pool, par), serial_state), order


@pytest.mark.parametrize("si,T,nan", [(8, 20, False), (5, 17, False), (6, 20, True)])
def test_eight_wave_runs_at_the_edges(emus, si, T, nan):
    """The edge workload (tests/edge_cases.py: every q of -520..520 across the IQ table's LDS cut at +-256, +-8190, 120 band
    records at 15-band rates, 51 long bands at sample index 5; nan: |q| = 8191 / -32768 in the last frame of the first run)
    through the eight-wave body in both rendezvous orders: the sixteen-wave body's bits, and the exact-roots oracle block by
    block"""
    _in_child("_check_edges", si, T, nan)


def _edge_batch(oracle, si, T, S=2, seed=71):
    import edge_cases as E
    wl = W.make_batch(n_streams=S, n_frames=T, layout=("cpe",), mix=True, intensity=True, seed=seed)
    units, meta = E.edge_side_info(wl, si, oracle, seed + 1)
    q, _ = E.edge_coeffs(units, meta, si, oracle, seed + 2)
    return wl, units, meta, q


def _check_edges(si, T, nan):
    import edge_cases as E
    import orc
    import parity
    oracle = orc.load()
    full, half = emu_lib.Emu(), emu_lib.Emu(LIB)
    S = 2
    wl, units, meta, q = _edge_batch(oracle, si, T, S)
    if nan:
        q = E.edge_nan(q, units, meta, 1, si, oracle, [s * T + 15 for s in range(S)])
    assert set(E.SEAM.tolist()) <= E.covered(units, meta, [q], si, oracle)
    C = wl["C"]
    exact = parity.exact_reference(oracle, units, q, meta, wl["n_pcm"], np.zeros((S, C, 1024), np.float32), sample_index=si)
    assert np.isnan(exact).any() == nan
    pool, par = emu_lib.new_pool(S, C)
    want = full.decode(units, q, meta, wl["n_pcm"], pool, par, sample_index=si, rv=1)
    want_state = emu_lib.pool_current(pool, par)
    parity.assert_blocks(want, exact, units, what="sixteen waves, sample index %d" % si)
    for rv in (1, 2):
        pool, par = emu_lib.new_pool(S, C)
        got = half.decode(units, q, meta, wl["n_pcm"], pool, par, sample_index=si, rv=rv)
        assert _same(got, want), rv
        assert _same(emu_lib.pool_current(pool, par), want_state), rv
    return True


def test_eight_wave_runs_through_cross_launch_cells_at_the_edges(emus):
    """three overlapped launches of one plan on the edge workload at a 15-band rate, meeting in cross-launch cells in a random
    interleaving: the serial sixteen-wave decode's bits"""
    _in_child("_check_edge_cells", 8, 18, 3)


def _check_edge_cells(si, T, n):
    import edge_cases as E
    import orc
    oracle = orc.load()
    full, half = emu_lib.Emu(), emu_lib.Emu(LIB)
    S = 1
    wl, units, meta, q = _edge_batch(oracle, si, T, S, seed=73)
    C = wl["C"]
    qs, at = [q], 0
    for j in range(1, n):
        x, at = E.edge_coeffs(units, meta, si, oracle, 80 + j, start=at)
        qs.append(x)
    pool, par = emu_lib.new_pool(S, C)
    serial = [full.decode(units, x, meta, wl["n_pcm"], pool, par, sample_index=si) for x in qs]
    serial_state = emu_lib.pool_current(pool, par)
    pool, par = emu_lib.new_pool(S, C)
    cells, heads = _cells(S, C)
    got, _ = half.decode_pipelined(units, qs, [meta] * n, wl["n_pcm"], pool, par, cells, heads, order=7, sample_index=si)
    for j in range(n):
        assert _same(got[j], serial[j]), j
    assert _same(emu_lib.pool_current(pool, par), serial_state)
    return True


@pytest.mark.parametrize("ablate", [2, 8, 10, 32, 64, 128])
def test_eight_wave_profiling_paths_finish(emus, ablate):
    """tools/floor.sh and tools/timeline.py run the headline route with these switches (profiling build): no epilogue (2), no
    dequantisation arithmetic (8), both, flat or two-level priorities (64, 32), every wave loading early (128).  Their PCM is not
    the product's; the decode must only finish, chains longer than a run and overlapped launches included."""
    _in_child("_check_ablate", ablate)


def _check_ablate(ablate):
    half = emu_lib.Emu(LIB)
    half.lib.emu_half_set_ablate(ablate)
    wl = W.make_batch(n_streams=2, n_frames=40, layout=("cpe",), mix=True, seed=5)
    pool, par = emu_lib.new_pool(2, wl["C"])
    half.decode(wl["units"], wl["q"], wl["meta"], wl["n_pcm"], pool, par, rv=2)
    pool, par = emu_lib.new_pool(2, wl["C"])
    cells, heads = _cells(2, wl["C"])
    half.decode_pipelined(wl["units"], [wl["q"]] * 3, [wl["meta"]] * 3, wl["n_pcm"], pool, par, cells, heads, order=2)
    half.lib.emu_half_set_ablate(0)
    return True
