"""aacg_units_refresh on the GPU, through the ABI, over MADE records: no parser.  The "parsed" records, the results and the map are
tensors the test fills; the spectra come from aacgpu_workload.make_batch(mix=True) — all four window sequences, grouped shorts,
both shapes, M/S — so that a wrong field of a record changes the PCM; a skeleton plan carries structure only.

Each test: aacg_plan_refresh_from_parse(_ex), then aacg_decode_device on one stream; the results and the counter read back are
those of the rule (tests/refresh_rule.py, the numpy statement tests/test_units_refresh_emu.py holds the kernel's source to), and
the PCM is the oracle's decode of the RULE's records — parity.exact_reference, per frame block at the project's TAU_RMS / TAU_MAX
(parity.assert_blocks), so that one wrong frame cannot hide in a batch mean.  The faults are the emulator test's, frame 51 across
the edge of the first workgroup of 256 lanes included.  Every wait for the GPU is the engine's bounded one (WAIT_MS)."""
import numpy as np
import pytest

import aacgpu
import aacgpu_workload
import parity
import refresh_rule as R

pytestmark = pytest.mark.gpu

WAIT_MS = 20000         # aacg_set_wait_limit_ms: every synchronize below fails with AACG_ERR_TIMEOUT instead of hanging
PARSE_ERROR = 4         # AACG_PARSE_SCALEFACTOR
ERR_UNSUPPORTED = -5
NCH = {"sce": 1, "cpe": 2}


class Made:
    """A batch as the parser would have left it, made on the host.  layout: the elements the plan lists (the workload's);
    parsed_layout: the elements the parser found per frame (the plan's first, then unlisted ones); U / Cp: the parser's max_units /
    max_channels; n_out_ch: the stream's interleave stride (>= the listed channels)."""

    def __init__(self, S, F, layout, parsed_layout=None, U=None, n_out_ch=None, seed=0xAAC0F5):
        parsed_layout = list(parsed_layout or layout)
        E, C = len(layout), sum(NCH[e] for e in layout)
        assert parsed_layout[:E] == list(layout)
        self.S, self.F, self.E, self.C, self.n = S, F, E, C, S * F
        self.want = len(parsed_layout)
        self.U = U or self.want
        self.Cp = sum(NCH[e] for e in parsed_layout)
        self.out_ch = n_out_ch or C
        wl = aacgpu_workload.make_batch(S, F, layout=tuple(layout), mix=True, seed=seed)
        n, Cp, U = self.n, self.Cp, self.U
        f = np.repeat(np.arange(n), E)
        true = wl["units"].copy()
        true["coef_offset"] = true["meta_offset"] = f * Cp + true["channel"]
        true["n_out_ch"] = self.out_ch
        true["pcm_offset"] = f * 1024 * self.out_ch
        self.n_pcm = n * 1024 * self.out_ch
        rng = np.random.default_rng(seed)
        # the spectra in the parser's blocks (frame * Cp + channel); the blocks of unlisted elements and two frames' worth behind the batch hold garbage
        self.q = rng.integers(-300, 300, ((n + 2) * Cp, 1024)).astype(np.int16)
        self.meta = rng.integers(0, 1 << 16, ((n + 2) * Cp, 120)).astype(np.uint16)
        blocks = (np.arange(n)[:, None] * Cp + np.arange(C)[None, :]).ravel()
        self.q[blocks], self.meta[blocks] = wl["q"], wl["meta"]
        # the parser's records: what it fills per element; stream, pcm_offset and n_out_ch are the caller's (garbage here)
        self.parsed = np.frombuffer(b"\xff" * (n * U * 64), aacgpu.UNIT_DTYPE).copy()
        chan = np.concatenate([[0], np.cumsum([NCH[e] for e in parsed_layout])])
        for e in range(self.want):
            if e < E:
                rec = true[e::E].copy()
            else:                                                # an element nobody lists: a valid record all the same
                rec = np.frombuffer(rng.integers(0, 256, n * 64, dtype=np.uint8).tobytes(), aacgpu.UNIT_DTYPE).copy()
                rec["n_ch"], rec["channel"] = NCH[parsed_layout[e]], chan[e]
                rec["coef_offset"] = rec["meta_offset"] = np.arange(n) * Cp + chan[e]
                rec["flags"] &= 0xff ^ R.HAS_PNS
            rec["stream"], rec["pcm_offset"], rec["n_out_ch"] = 0xEEEEEEEE, 0xEEEEEEEE, 0xEEEE
            self.parsed[e::U] = rec
        self.results = np.zeros(n, R.RESULT_DTYPE)
        self.results["n_units"], self.results["n_channels"] = self.want, Cp
        # the plan's skeleton: structure only
        self.skel = true.copy()
        self.skel["flags"] = 0
        self.skel["ch"] = np.zeros((), true.dtype["ch"])
        self.skel["ch"]["group_count"] = 1
        self.skel["ch"]["group_len"][..., 0] = 1
        self.picks = f * U + np.tile(np.arange(E), n)
        self.map = None

    def with_map(self):
        self.map = np.zeros(len(self.skel), R.MAP_DTYPE)
        self.map["parsed_index"] = self.picks
        self.map["frame_units"] = self.want | ((self.E if self.E < self.want else 0) << 8)
        return self

    # -- the faults (frame: index in the batch's packed order) --
    def error(self, frame):
        self.results["status"][frame] = PARSE_ERROR
        self.parsed[frame * self.U:(frame + 1) * self.U] = np.frombuffer(b"\xff" * (self.U * 64), aacgpu.UNIT_DTYPE)

    def elsewhere(self, frame, element):
        """the parser put the element's channels into other blocks than the plan's run tables say (spare ones behind the batch)"""
        rec = self.parsed[frame * self.U + element:frame * self.U + element + 1]
        rec["coef_offset"] = rec["meta_offset"] = self.n * self.Cp + int(rec["channel"][0])

    def noise(self, frame, element):
        self.parsed["flags"][frame * self.U + element] |= R.HAS_PNS

    def count(self, frame, n_units):
        self.results["n_units"][frame] = n_units

    def rule(self, refuse_pns=1, keep_tns=0):
        units = np.zeros(len(self.skel), R.DEV_UNIT_DTYPE)
        units["d"] = self.skel
        return R.refresh(units, self.parsed, self.results, self.map, self.U, refuse_pns, keep_tns)


def run(made, oracle, sets=1, set_index=0, then=None):
    """plan(skeleton) -> refresh -> decode_device on one stream; the rule's results, counter and PCM.  then(eng, plan): called
    between the refresh and the launch.  -> (rule's records, rule's results, refused, accepted?)"""
    import torch
    want_u, want_r, want_n, taken = made.rule()
    ov = np.zeros((made.S, made.out_ch, 1024), np.float32)
    exact = parity.exact_reference(oracle, want_u["d"], made.q, made.meta, made.n_pcm, ov)
    assert np.isfinite(exact).all()
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)
    d_parsed, d_res, d_q, d_meta = t(made.parsed), t(made.results), t(made.q), t(made.meta)
    d_map = t(made.map) if made.map is not None else None
    d_pcm = torch.full((made.n_pcm,), float("nan"), dtype=torch.float32, device=dev)
    d_refused = torch.full((4,), 1000, dtype=torch.int32, device=dev)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    eng = aacgpu.Engine(aacgpu.INPUT_QUANT_I16, max_streams=made.S, max_channels=made.out_ch)
    try:
        eng.set_wait_limit_ms(WAIT_MS)
        plan = eng.plan(made.skel)
        if sets > 1:
            eng._check(eng.lib.aacg_plan_set_unit_sets(eng.handle, plan.handle, sets))
        if made.map is None and sets == 1:
            eng.plan_refresh_from_parse(plan, d_parsed.data_ptr(), d_res.data_ptr(), made.U, d_refused.data_ptr(), side.cuda_stream)
        else:
            eng._check(eng.lib.aacg_plan_refresh_from_parse_ex(eng.handle, plan.handle, d_parsed.data_ptr(), d_res.data_ptr(), made.U,
                                                               d_map.data_ptr() if d_map is not None else None, set_index, d_refused.data_ptr(), side.cuda_stream))
        if then:
            then(eng, plan)
        eng.decode_device(plan, d_q.data_ptr(), d_meta.data_ptr(), d_pcm.data_ptr(), side.cuda_stream)
        eng.synchronize(side.cuda_stream)
        got_r = np.frombuffer(d_res.cpu().numpy().tobytes(), R.RESULT_DTYPE)
        counter = d_refused.cpu().numpy()
        pcm = d_pcm.cpu().numpy()
        plan.destroy()
    finally:
        eng.close()
    assert got_r.tobytes() == want_r.tobytes(), "the results differ from the rule's at frames %s" % np.nonzero(got_r["status"] != want_r["status"])[0][:8]
    assert counter.tolist() == [1000 + want_n, 1000, 1000, 1000], "refused: %d counted, the rule has %d" % (counter[0] - 1000, want_n)
    assert np.isfinite(pcm).all(), "samples nobody wrote"
    print("refused %d of %d units / frames; worst block: RMS %.3e x s, max %.3e x s_peak" % (
        (want_n, len(taken)) + tuple(np.max(x) for x in parity.block_errors(pcm, exact, want_u["d"]))))
    parity.assert_blocks(pcm, exact, want_u["d"], parity.TAU_RMS, parity.TAU_MAX, what="refreshed records")
    return want_u, want_r, want_n, taken, pcm, exact


def test_no_map_stereo(oracle):
    """(a) no map: stereo, 2 streams x 129 frames = 258 units in two workgroups; parse errors, frames the parser put into other
    blocks, noise flags on a PNS_REFERENCE engine — each refused for its own sake, silent, counted; the results untouched"""
    m = Made(2, 129, ["cpe"])
    assert len(m.skel) == 258
    errors, moved, noisy = [0, 77, 128, 129, 255], [3, 130, 256], [9, 254, 257]
    for f in errors:
        m.error(f)
    for f in moved:
        m.elsewhere(f, 0)
    for f in noisy:
        m.noise(f, 0)
    want_u, want_r, n, taken, _, _ = run(m, oracle)
    assert n == 11 and sorted(np.nonzero(~taken)[0]) == sorted(errors + moved + noisy) and want_r.tobytes() == m.results.tobytes()
    seqs = set(want_u["d"]["ch"]["window_sequence"][taken].ravel())
    assert seqs == {0, 1, 2, 3} and (want_u["gmap"][taken] == 0x21111000).any() and set(want_u["d"]["ch"]["window_shape"][taken].ravel()) == {0, 1}


FIVE = ["sce", "cpe", "cpe", "cpe", "sce"]


def test_map_five_elements_across_the_workgroup_edge(oracle):
    """(b) map: five elements in eight channels, 52 frames = 260 units, max_units 8; frame 51's first lane is lane 255 of the first
    workgroup, its other four lanes are in the second.  A fault in element 0 only, in a middle element only, in the last element
    only, in frames 0, 50 and 51 (the last) in turn; a parse error; a wrong element count.  The whole frame goes silent — in the
    rule its PCM is the tail of the frame before it —, is counted once, and its status becomes LAYOUT"""
    seen = 0
    for k, where in enumerate([0, 2, 4]):
        m = Made(1, 52, FIVE, U=8, seed=0xAAC0F6 + k).with_map()
        assert len(m.skel) == 260 and m.picks[255] == 51 * 8
        faults = {0: where, 50: (where + 1) % 5, 51: where, 23: where}
        for f, e in faults.items():
            m.elsewhere(f, e)
        m.error(7)
        m.count(30, 4)
        m.count(31, 6)
        m.noise(40, where)
        want_u, want_r, n, taken, pcm, exact = run(m, oracle)
        silent = sorted(list(faults) + [7, 30, 31, 40])
        per_frame = taken.reshape(52, 5)
        assert n == len(silent) and sorted(np.nonzero(~per_frame.any(axis=1))[0]) == silent and per_frame[[f for f in range(52) if f not in silent]].all()
        assert [int(want_r["status"][f]) for f in silent] == [PARSE_ERROR if f == 7 else R.PARSE_LAYOUT for f in silent]
        # a silent frame behind a decoded one is that frame's tail, not silence; behind a silent one it is silence
        blocks = exact.reshape(52, 1024, 8)
        assert np.abs(blocks[23]).max() > 1e-3 and np.abs(blocks[51]).max() == 0 and np.abs(blocks[31]).max() == 0
        seen += 1
    assert seen == 3


def test_map_two_of_three_listed(oracle):
    """(c) map with listed < want: SCE + CPE + CPE parsed into five channels, a four-channel engine whose plan lists the first two
    elements.  Channel 3 is exactly zero; the unlisted element's garbage — another element kind, other blocks, 0xFF — has no effect;
    n_units 2 or 4 refuses a frame whose listed elements match; a moved listed element refuses it"""
    m = Made(2, 65, ["sce", "cpe"], parsed_layout=["sce", "cpe", "cpe"], U=3, n_out_ch=4).with_map()
    assert len(m.skel) == 260 and (m.map["frame_units"] == 0x203).all()
    for f in (1, 64, 127):                                       # the unlisted third element: anything
        m.parsed["n_ch"][f * 3 + 2] = 1
    for f in (2, 66):
        m.parsed["coef_offset"][f * 3 + 2] += 9
    for f in (5, 128):
        m.parsed[f * 3 + 2:f * 3 + 3] = np.frombuffer(b"\xff" * 64, aacgpu.UNIT_DTYPE)
    m.noise(6, 2)
    m.count(10, 2)
    m.count(70, 4)
    m.elsewhere(20, 1)
    m.elsewhere(129, 0)
    m.error(100)
    want_u, want_r, n, taken, pcm, exact = run(m, oracle)
    silent = [10, 20, 70, 100, 129]
    assert n == 5 and sorted(np.nonzero(~taken.reshape(130, 2).any(axis=1))[0]) == silent and taken.sum() == 250
    assert [int(want_r["status"][f]) for f in silent] == [R.PARSE_LAYOUT, R.PARSE_LAYOUT, R.PARSE_LAYOUT, PARSE_ERROR, R.PARSE_LAYOUT]
    assert (pcm.reshape(-1, 4)[:, 3] == 0).all() and (exact.reshape(-1, 4)[:, 3] == 0).all(), "channel 3 has no element: exactly zero"
    assert np.abs(pcm.reshape(-1, 4)[:, :3]).max(axis=0).min() > 1e-3


def test_host_refresh_refused_with_unit_sets(oracle):
    """aacg_plan_refresh_units on a plan with more than one set of unit records: a kept plan, aacg_plan_set_unit_sets(3), a device
    refresh of set 2, then the host refresh — which would rewrite set 0, which no launch reads.  It is refused (AACG_ERR_UNSUPPORTED,
    the reason in aacg_last_error), and the plan still decodes set 2 as refreshed"""
    m = Made(2, 20, ["cpe"], seed=0xAAC0F9)
    m.error(4)
    m.elsewhere(25, 0)
    other = aacgpu_workload.make_batch(2, 20, mix=True, seed=77)["units"]     # the same structure, other content: a host refresh would take it

    def then(eng, plan):
        with pytest.raises(aacgpu.AacgError) as e:
            eng.plan_refresh_units(plan, other)
        assert e.value.code == ERR_UNSUPPORTED
        assert "aacg_plan_refresh_units" in str(e.value) and "more than one set" in str(e.value) and "aacg_plan_set_unit_sets" in str(e.value)

    _, _, n, taken, _, _ = run(m, oracle, sets=3, set_index=2, then=then)
    assert n == 2 and taken.sum() == 38
