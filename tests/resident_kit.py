"""What the resident route's GPU tests share (test_pipeline_gpu.py, test_ragged_pipeline_gpu.py, test_device_plans_gpu.py,
test_resident_stages_gpu.py, test_resident_shape_gpu.py, test_output_edges.py, test_parse_device.py, test_mp4a_resident_gpu.py,
test_tns_records_emu.py): the committed streams and the corpus, the scripts of batches and what runs them, the host-planned
yardstick, the project's tolerances, and the fixtures — a test file that uses one imports it by name.  A plain module like orc.py;
torch is imported where a GPU is used, so the CPU tests can import it too."""
import base64
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import aacgpu
import emu_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAMS = os.path.join(ROOT, "tests", "golden", "streams")
CASES = json.load(open(os.path.join(STREAMS, "manifest.json")))
CORPUS = json.load(open(os.path.join(ROOT, "tests", "golden", "corpus.json")))["streams"]
NODE = shutil.which("node")
ERR_INVALID_ARG, ERR_CAPACITY, ERR_UNSUPPORTED = -1, -4, -5          # AACG_ERR_* (include/aacgpu.h)
PARSE_TNS_ORDER, PARSE_LAYOUT = 8, 16                                # AACG_PARSE_*
PLAIN = aacgpu.PARSE_REFERENCE_QUIRKS
OPTIONS = aacgpu.PARSE_APPLY_PULSES | aacgpu.PARSE_REFERENCE_QUIRKS
EX_RV = "aacg_imdct_run_quant_ex_rv"
# the streams of tests/js/stage_cases.js and shape_cases.js: (names, channels, sample index)
GROUPS = [("mono48", 1, 3), ("stereo48+split48", 2, 3), ("five1_48", 6, 3), ("mono16", 1, 8), ("stereo16+split16", 2, 8), ("five1_16", 6, 8)]


# ---- streams ---------------------------------------------------------------------------------------------------------------------
def adts_frame_table(data):
    out, off = [], 0
    while off + 7 <= len(data):
        assert data[off] == 0xFF and (data[off + 1] & 0xF0) == 0xF0
        length = ((int(data[off + 3]) & 3) << 11) | (int(data[off + 4]) << 3) | (int(data[off + 5]) >> 5)
        out.append((off, length))
        off += length
    return np.array(out, aacgpu.PARSE_FRAME_DTYPE)


def load(case):
    data = np.fromfile(os.path.join(STREAMS, case["name"] + ".aac"), np.uint8)
    table = adts_frame_table(data)
    assert len(table) == case["frames"]
    return data, table, np.fromfile(os.path.join(STREAMS, case["name"] + ".refpcm"), np.float32)


@pytest.fixture(scope="module")
def corpus_streams(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("corpus"))
    r = subprocess.run([NODE or "node", os.path.join(ROOT, "tests", "js", "corpus_cases.js"), d], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return {e["name"]: np.fromfile(os.path.join(d, e["name"] + ".aac"), np.uint8) for e in CORPUS}


def case_streams(d, script):
    """{name: (manifest entry, bytes, frame table)} of the streams tests/js/<script> writes into d"""
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", script), d], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = {}
    for c in json.load(open(os.path.join(d, "manifest.json"))):
        data = np.fromfile(os.path.join(d, c["name"] + ".aac"), np.uint8)
        out[c["name"]] = (c, data, adts_frame_table(data))
    return out


@pytest.fixture(scope="module")
def stage_streams(tmp_path_factory):
    out = case_streams(str(tmp_path_factory.mktemp("stage_cases")), "stage_cases.js")
    for c, data, table in out.values():
        assert len(table) == c["frames"] == c["parsed"] == 12, "the JavaScript front end parses every frame of the chosen seeds"
    return out


@pytest.fixture(scope="module")
def shape_streams(tmp_path_factory):
    out = case_streams(str(tmp_path_factory.mktemp("shape_cases")), "shape_cases.js")
    for c, data, table in out.values():
        assert len(table) == c["frames"] == c["parsed"] == 12 and c["pnsUnits"] == 0 and c["bothWays"] and c["kbdAtBoundary"], c
    return out


def members_of(streams, names, copies):
    """[(bytes, table)] for the pipeline: `copies` slots per named stream, each at a starting frame of its own where noted"""
    return [(streams[n][1], streams[n][2]) for n in names for _ in range(copies)]


# ---- tolerances and comparisons --------------------------------------------------------------------------------------------------
def close_to(pcm, ref):
    """the project's tolerances: RMS error < 1e-5 absolute and <= 5e-6 of the signal RMS, on a signal that is one"""
    assert np.isfinite(pcm).all() and np.isfinite(ref).all()
    d = pcm.astype(np.float64) - ref
    err, sig = float(np.sqrt(np.mean(d * d))), float(np.sqrt(np.mean(ref.astype(np.float64) ** 2)))
    print("rms error %.3e, signal rms %.3e" % (err, sig))
    assert sig > 1e-3 and err < 1e-5 and err <= 5e-6 * sig, (err, sig)


def check_corpus_pcm(e, pcm):
    p = e["pcm"]
    assert pcm.size == p["n"] and np.isfinite(pcm).all(), e["name"]
    probes = np.frombuffer(base64.b64decode(p["probes"]), np.float32)
    idx = [((k * 7919 + 13) * 104729) % p["n"] for k in range(64)]
    rms = (p["sumsq"] / p["n"]) ** 0.5
    assert np.abs(pcm[idx].astype(np.float64) - probes).max() <= 1e-5 * max(1.0, 4.0 * rms), (e["name"], float(np.abs(pcm[idx] - probes).max()), rms)
    x = pcm.astype(np.float64)
    assert abs(float(x.sum()) - p["sum"]) <= 2e-6 * p["n"] ** 0.5 * max(rms, 1e-3) + 1e-9 * p["n"], (e["name"], float(x.sum()), p["sum"])
    assert abs(float((x * x).sum()) - p["sumsq"]) <= 2e-5 * p["sumsq"] + 1e-12, (e["name"], float((x * x).sum()), p["sumsq"])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint16),
                                                                         b.view(np.uint32 if b.dtype.itemsize == 4 else np.uint16))


# ---- batches ---------------------------------------------------------------------------------------------------------------------
def packed(tables, bases, at, counts):
    """the batch's frame table: stream s's frames at[s] .. at[s] + counts[s] - 1, packed stream after stream"""
    out = np.concatenate([tables[s][at[s]:at[s] + counts[s]] for s in range(len(counts))]).copy()
    out["byte_offset"] += np.repeat(np.asarray(bases, np.uint32), counts)
    return out


def ragged_script(tables, max_frames, rng):
    """the batches of tests/test_ragged_pipeline_gpu.py's ragged_run, drawn once so that every pipeline of a test decodes the same ones:
    random counts (1..max_frames, at most what is left), streams that are done drop out -> [(live slots, counts, first frames)]"""
    S = len(tables)
    at = [0] * S
    out = []
    while any(at[s] < len(tables[s]) for s in range(S)):
        live = [s for s in range(S) if at[s] < len(tables[s])]
        counts = [int(rng.integers(1, min(max_frames, len(tables[s]) - at[s]) + 1)) for s in live]
        out.append((live, counts, [at[s] for s in live]))
        for s, c in zip(live, counts):
            at[s] += c
    return out


def rect_script(S, F, n_frames):
    return [(list(range(S)), [F] * S, [a] * S) for a in range(0, n_frames, F)]


def run_script(members, script, C_, si, max_frames, device_plans, **kw):
    """-> (per-stream PCM, per-stream statuses, refusals in all, plan builds, launch counts)"""
    S = len(members)
    data = np.concatenate([m[0] for m in members])
    bases = np.cumsum([0] + [len(m[0]) for m in members])[:-1]
    tables = [m[1] for m in members]
    p = aacgpu.Pipeline(channels=C_, max_streams=S, max_frames=max_frames, sample_index=si, device_plans=device_plans, **kw)
    got, status, refusals = [[] for _ in range(S)], [[] for _ in range(S)], 0
    per = 1024 * C_
    for live, counts, at in script:
        fr = packed([tables[s] for s in live], [bases[s] for s in live], at, counts)
        pcm, res, refused = p.decode(data, fr, np.array(live, np.uint32), np.array(counts, np.uint32))
        refusals += refused
        first = np.concatenate([[0], np.cumsum(counts)])
        for k, s in enumerate(live):
            got[s].append(pcm[first[k] * per:first[k + 1] * per])
            status[s].append(res["status"][first[k]:first[k + 1]].copy())
    builds, counts_ = p.plan_builds(), p.launch_counts()
    p.close()
    return [np.concatenate(g) for g in got], [np.concatenate(x) for x in status], refusals, builds, counts_


def steady(data, table, S, B, period, device_plans, odd_at=None, **kw):
    """the same shape B times (S stereo streams x 2 frames, the streams fed round and round: batch b starts at frame 2 b mod period),
    submitted ahead on five lanes; batch odd_at, if any, has three streams fewer -> (launch counts, PCM of every batch)"""
    p = aacgpu.Pipeline(channels=2, max_streams=S, max_frames=2, lanes=5, device_plans=device_plans, **kw)
    pcm, pending = [], []
    for b in range(B):
        k = S - 3 if b == odd_at else S
        fr = packed([table] * k, [0] * k, [(2 * b) % period] * k, [2] * k)
        pending.append(p.submit(data, fr, np.arange(k), np.full(k, 2, np.uint32), pcm=p.pinned(k * 2 * 2048, np.float32)))
        if len(pending) == 5:
            pcm.append(p.collect(pending.pop(0))[0].copy())
    pcm += [p.collect(t)[0].copy() for t in pending]
    counts = p.launch_counts()
    p.close()
    assert counts["launches"] == B
    return counts, pcm


# ---- the host-planned yardstick --------------------------------------------------------------------------------------------------
def parse_dims(C_):
    """what the pipeline allows the parser per frame: (elements, channel blocks)"""
    return (8, 8) if C_ > 2 else (1, C_)


def silent(units):
    """what the refresh makes of a refused frame's unit: ONLY_LONG, sine, nothing coded; the planner's part stays"""
    units["flags"] = 0
    units["tns_offset"] = 0
    units["ch"] = np.zeros((), aacgpu.UNIT_DTYPE["ch"].base)
    units["ch"]["group_count"], units["ch"]["group_len"][..., 0] = 1, 1


@pytest.fixture(scope="module")
def oracle():
    import orc
    return orc.load()


class HostRoute:
    """the yardstick: host parse (spec: with TNS side info, for an engine with the spec-correct stages and host-made TNS records) ->
    window_shape_prev by the rule (carry) or 0, what the parser writes -> a plan per batch -> decode_pipelined; and the oracle.
    every_frame_parses: a frame the parser refuses fails the test instead of going silent."""

    def __init__(self, S, C_, si, oracle=None, carry=True, spec=False, options=PLAIN, every_frame_parses=False):
        import torch
        self.torch, self.S, self.C, self.si, self.carry, self.spec, self.options = torch, S, C_, si, carry, spec, options
        self.every_frame_parses = every_frame_parses
        self.U, self.Cp = parse_dims(C_)
        self.parser = aacgpu.Parser(sample_index=si)
        modes = dict(tns_mode=aacgpu.TNS_SPEC, pns_mode=aacgpu.PNS_SPEC) if spec else {}
        self.eng = aacgpu.Engine(aacgpu.INPUT_QUANT_I16, max_streams=S, max_channels=C_, sample_index=si, **modes)
        self.oracle, self.ov = oracle, np.zeros((S, C_, 1024), np.float32)
        self.W = np.zeros((S, C_), np.uint8)                  # the rule's state
        self.shapes = [[] for _ in range(S)]                  # per stream: per frame, (shape of every channel, shape_prev it was given)
        self.routes, self.refused = set(), 0
        self.tns_channels = self.channel_frames = self.units = self.pns_units = 0

    def reset(self, s):
        self.eng.reset_stream(s)
        self.W[s] = 0
        self.ov[s] = 0

    def decode(self, data, fr, live, counts):
        """-> (PCM of the batch, packed stream after stream like the pipeline's; the oracle's or None; the parser's outputs)"""
        torch = self.torch
        out = self.parser.parse_batch(data, fr, self.U, self.Cp, self.options, self.spec)
        if self.every_frame_parses:
            assert not out["results"]["status"].any(), "every frame parses"
        n, per = len(fr), 1024 * self.C
        units = []
        first = np.concatenate([[0], np.cumsum(counts)])
        for k, s in enumerate(live):
            for i in range(first[k], first[k + 1]):
                shape, prev = np.zeros(self.C, np.uint8), self.W[s].copy()
                if int(out["results"]["status"][i]) or (self.C <= 2 and int(out["results"]["n_units"][i]) != 1):
                    # a refused frame (a parse error, or not the one element the plan lists): what the refresh makes of it — a silent
                    # unit on the planner's record (one element: C <= 2)
                    assert self.C <= 2
                    u = np.zeros((), aacgpu.UNIT_DTYPE)
                    u["n_ch"], u["coef_offset"], u["meta_offset"] = self.C, i * self.Cp, i * self.Cp
                    silent(u)
                    u["stream"], u["n_out_ch"], u["pcm_offset"] = s, self.C, i * per
                    frame_units = [u]
                    self.refused += 1
                else:
                    frame_units, chan = [], 0
                    for e in range(int(out["results"]["n_units"][i])):
                        u = out["units"][i * self.U + e].copy()
                        if chan + int(u["n_ch"]) > self.C:
                            break                               # decoder.js:233: elements beyond chanConfig channels are dropped
                        u["stream"], u["n_out_ch"], u["pcm_offset"] = s, self.C, i * per
                        self.units += 1
                        self.pns_units += bool(int(u["flags"]) & aacgpu.UNIT_HAS_PNS)
                        self.channel_frames += int(u["n_ch"])
                        for c in range(int(u["n_ch"])):
                            shape[chan + c] = u["ch"]["window_shape"][c]
                        chan += int(u["n_ch"])
                        frame_units.append(u)
                for u in frame_units:
                    for c in range(int(u["n_ch"])):
                        u["ch"]["window_shape_prev"][c] = prev[int(u["channel"]) + c] if self.carry else 0
                units += frame_units
                self.shapes[s].append((shape, prev))
                self.W[s] = shape                               # (every channel of these streams has a unit in every frame)
        units = np.array(units, aacgpu.UNIT_DTYPE)
        tns = out["tns"] if self.spec else None
        plan = self.eng.plan(units, tns=tns) if self.spec else self.eng.plan(units)
        self.routes.add(self.eng.plan_kernels(plan, pipelined=True))
        d_q, d_meta = torch.from_numpy(out["q"]).cuda(), torch.from_numpy(out["meta"].view(np.int16)).cuda()
        d_pcm = torch.zeros(n * per, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        self.eng.decode_pipelined(plan, d_q.data_ptr(), d_meta.data_ptr(), d_pcm.data_ptr())
        self.eng.synchronize()
        pcm = d_pcm.cpu().numpy()
        plan.destroy()
        ref = None
        if self.oracle is not None:
            kw = dict(tns=tns, pns=True) if self.spec else {}
            ref = self.oracle.decode_batch(units, out["q"], out["meta"], n * per, self.ov, sample_index=self.si, **kw)
        return pcm, ref, out

    def close(self):
        self.eng.close()
        self.parser.close()


# ---- aacg_tns_prepare on the host, next to the records kernel's source (tests/emu/tnsprep_emu.cpp) ---------------------------------
@pytest.fixture(scope="module")
def emu_tns(tmp_path_factory):
    L = emu_lib.build_driver("tnsprep_emu", ["tests/emu/tnsprep_emu.cpp", "aac.js_amd/csrc/aacg_plan.cpp", "aac.js_amd/csrc/aacg_tables.cpp"],
                             tmp_path_factory.mktemp("tnsprep_emu"))
    L.emu_tnsprep_layout.restype = C.c_uint64
    L.emu_tnsprep_layout.argtypes = [C.c_uint32, C.c_void_p]
    L.emu_tns_records.argtypes = [C.c_int] + [C.c_void_p] * 3 + [C.c_uint32] * 4 + [C.c_void_p]
    L.emu_tns_host.argtypes = [C.c_int] + [C.c_void_p] * 3 + [C.c_uint32] * 3 + [C.c_void_p]
    sizes = np.zeros(6, np.uint32)
    L.emu_tnsprep_sizes(sizes.ctypes.data_as(C.c_void_p))
    assert list(sizes[:5]) == [aacgpu.DEV_TNS_DTYPE.itemsize, aacgpu.TNS_DTYPE.itemsize, aacgpu.UNIT_DTYPE.itemsize, aacgpu.PARSE_RESULT_DTYPE.itemsize,
                               aacgpu.TNS_M_DOUBLES]
    return L


def records_layout(lib, n):
    total = C.c_uint64()
    m_off = int(lib.emu_tnsprep_layout(n, C.byref(total)))
    assert m_off % 256 == 0 and m_off >= n * 512 and int(total.value) == m_off + n * aacgpu.TNS_M_DOUBLES * 8
    return m_off, int(total.value)

