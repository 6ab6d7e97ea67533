"""ctypes wrapper for tests/emu/libaacg_emu.so — the kernels' source run lane-by-lane on CPU threads
(test infrastructure; see tests/emu/devport_emu.h)."""
import ctypes as C
import os
import subprocess

import numpy as np

import orc

HERE = os.path.dirname(os.path.abspath(__file__))
RUN_DTYPE = np.dtype([("pred_unit", "<i4"), ("n_units", "<i4"), ("is_last", "<i4"), ("wave_nch", "<u4"),
                      ("ov0", "<i4", (2,)), ("rot", "<i4", (2,)), ("unit", "<i4", (16,)),
                      ("wave_unit", "<i4", (16,)), ("wave_coef", "<u4", (16,)), ("wave_meta", "<u4", (16,))])     # aacg_run, aacg_device.h


OV_BUFFERS = 16         # AACG_OV_BUFFERS: rotating overlap buffers per channel (aacg_device.h)


def new_pool(streams, channels):
    """An engine's overlap pool, zeroed: [stream][channel][OV_BUFFERS][1024], and the live-buffer index per (stream, channel)."""
    return np.zeros((streams, channels, OV_BUFFERS, 1024), np.float32), np.zeros(streams * channels, np.uint8)


POLICIES = {"natural": 1, "reversed": 2, "straggler": 3, "sprinter": 4, "random": 5, "cell": 6}     # emu_set_schedule (tests/emu/emu_lib.cpp)
FAULTS = {"skip_wait": 1, "early_set": 2, "blind_cas": 3, "lost_set": 4}                                             # emu_set_fault
ERR_DEADLOCK = -9001


class EmuDeadlock(RuntimeError):
    """A decode in schedule-controlled mode in which no wave could run any more: the text names who waited for what."""


def _build_locked(cmd, **kw):
    import fcntl
    with open(os.path.join(HERE, "emu", ".build.lock"), "w") as lock:      # one build at a time (pytest-xdist workers)
        fcntl.flock(lock, fcntl.LOCK_EX)
        subprocess.run(cmd, check=True, **kw)


def build_driver(name, sources, out_dir):
    """A driver under tests/emu/ and the host sources it links (paths from the repository's root) compiled as tests/emu/Makefile
    compiles the emulator, into out_dir/lib<name>.so; returns the loaded library.  The caller sets its argtypes."""
    so = os.path.join(str(out_dir), "lib%s.so" % name)
    _build_locked(["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-fno-strict-aliasing", "-DAACG_EMU_BUILD", "-I", os.path.join(HERE, "emu"),
                   "-pthread", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-shared", "-Wl,--no-undefined", "-o", so]
                  + [os.path.join(os.path.dirname(HERE), s) for s in sources])
    return C.CDLL(so)


class Emu:
    def __init__(self, target="libaacg_emu.so"):
        _build_locked(["make", "-C", os.path.join(HERE, "emu"), target], stdout=subprocess.DEVNULL)
        self.lib = L = C.CDLL(os.path.join(HERE, "emu", target))
        L.emu_last_error.restype = C.c_char_p
        L.emu_decode.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.emu_decode_tns.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.emu_decode_ex.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.emu_decode_cce.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.emu_spectral.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.emu_plan.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        L.emu_plan_refresh.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int]
        L.emu_decode_pipelined.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_int]
        L.emu_get_windows.argtypes = [C.c_int, C.c_void_p]
        L.emu_get_iq_sf.argtypes = [C.c_void_p, C.c_void_p]
        L.emu_last_keys.argtypes = [C.c_void_p, C.c_int]
        L.emu_set_schedule.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_int]
        L.emu_sched_steps.restype = C.c_long
        L.emu_sched_trace.argtypes = [C.c_void_p, C.c_int]
        L.emu_sched_cells.argtypes = [C.c_void_p, C.c_void_p]
        L.emu_set_fault.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
        L.emu_flags_offset.argtypes = [C.c_int, C.c_int]

    def error(self):
        return self.lib.emu_last_error().decode()

    def set_schedule(self, schedule, span=0):
        """Schedule-controlled mode for the run kernels of later decodes (tests/emu/devport_emu.h): one wave at a time, the next
        one picked by the policy.  schedule: None (off: the default), ("natural",), ("reversed",), ("straggler", k), ("sprinter", k),
        ("random", seed, d) — span: the turns of a run of the same decode (sched_steps), from which the d change points are
        drawn —, ("cell", a, variant) with variant 1..5 (emu_set_schedule in tests/emu/emu_lib.cpp)."""
        if schedule is None:
            self.lib.emu_set_schedule(0, 0, 0, 0, 0)
        elif schedule[0] == "random":
            self.lib.emu_set_schedule(POLICIES["random"], 0, schedule[2], schedule[1], span)
        else:
            a, b = (list(schedule[1:]) + [0, 0])[:2]
            self.lib.emu_set_schedule(POLICIES[schedule[0]], a, b, 0, span)

    def sched_steps(self):
        """turns the controller granted in the last decode"""
        return int(self.lib.emu_sched_steps())

    def sched_cells(self):
        """(in-launch rendezvous cells, chains) of the last decode's plan: cell(a, .) takes a below the first for decode(), below
        chains * (launches - 1) for decode_pipelined()"""
        a, b = C.c_int(0), C.c_int(0)
        self.lib.emu_sched_cells(C.byref(a), C.byref(b))
        return a.value, b.value

    def set_fault(self, kind=None, lo=0, hi=0, wave=-1):
        """Breaks an emulated primitive for later decodes (None: mends it).  "skip_wait": dp_flag_wait on flags in LDS bytes
        [lo, hi) returns at once; "early_set": the same for waiting wave `wave` only (the flag counts as set from the start for
        that waiter); "lost_set": dp_flag_set on such a flag does nothing; "blind_cas": dp_g_cas_u64 stores without comparing
        and reports success."""
        self.lib.emu_set_fault(FAULTS[kind] if kind else 0, lo, hi, wave)

    def flags_offset(self, quant, half):
        """LDS byte offset of the run body's flags (flags[task], then — eight-wave body — flags[16 + task])"""
        return int(self.lib.emu_flags_offset(1 if quant else 0, 1 if half else 0))

    def _raise(self, what, rc):
        if rc == ERR_DEADLOCK:
            raise EmuDeadlock(self.error())
        raise RuntimeError("%s rc=%d: %s" % (what, rc, self.error()))

    def decode(self, units, coeffs, meta, n_pcm, pool, parity, sample_index=3, tns=None, pns=False, int16_out=False, cce=None, staged=False, unfused=False, rv=1,
               pipelined=False, poison=None):
        """staged: the optional stages (TNS, PNS) as a launch of their own even where the engine would run them inside the run kernel.
        unfused: independent coupling as the separate pass over the PCM (what plans with double-duty runs take) even where the
        engine applies it in the targets' epilogues.  pipelined: the route aacg_decode_pipelined takes for the plan (the rendezvous
        kernels for plain batches and batches with optional stages), as one launch.  poison: what the output holds before the
        decode (default NaN, int16 -32768)."""
        units = np.ascontiguousarray(units)
        coeffs = np.ascontiguousarray(coeffs)
        kind = 1 if coeffs.dtype == np.int16 else 0
        meta = np.ascontiguousarray(meta, np.uint16) if meta is not None else None
        if poison is None:
            poison = -32768 if int16_out else np.nan
        pcm = np.full(n_pcm, poison, np.int16 if int16_out else np.float32)
        tns = np.ascontiguousarray(tns) if tns is not None else None
        self.lib.emu_set_output_kind(1 if int16_out else 0)
        self.lib.emu_set_staged(1 if staged else 0)
        self.lib.emu_set_unfused(1 if unfused else 0)
        self.lib.emu_set_rv(rv)           # 1: chains longer than a run through the run-to-run rendezvous (the engine's route); 2: blocks in reverse; 0: recomputed frames
        self.lib.emu_set_pipelined(1 if pipelined else 0)
        cce = np.ascontiguousarray(cce) if cce is not None else None
        rc = self.lib.emu_decode_cce(kind, sample_index, pool.shape[0], pool.shape[1], units.ctypes.data, len(units),
                                     coeffs.ctypes.data, meta.ctypes.data if meta is not None else None,
                                     tns.ctypes.data if tns is not None else None, len(tns) if tns is not None else 0,
                                     1 if pns else 0, cce.ctypes.data if cce is not None else None, len(cce) if cce is not None else 0,
                                     pcm.ctypes.data, n_pcm, pool.ctypes.data, parity.ctypes.data)
        self.lib.emu_set_output_kind(0)
        self.lib.emu_set_staged(0)
        self.lib.emu_set_unfused(0)
        self.lib.emu_set_rv(1)
        self.lib.emu_set_pipelined(0)
        if rc:
            self._raise("emu_decode", rc)
        return pcm

    def last_keys(self):
        """The switches (AACG_RK_*, the non-temporal bit included) of every run kernel the last decode launched, in launch order:
        the keys the emulator dispatched by (a coupling elements' pass of the plain kernel included)."""
        n = self.lib.emu_last_keys(None, 0)
        a = np.zeros(max(n, 1), np.uint32)
        self.lib.emu_last_keys(a.ctypes.data, n)
        return [int(k) for k in a[:n]]

    def spectral(self, units, q, meta, sample_index=3):
        units = np.ascontiguousarray(units)
        q = np.ascontiguousarray(q, np.int16)
        meta = np.ascontiguousarray(meta, np.uint16)
        spec = np.zeros(q.shape, np.float32)
        rc = self.lib.emu_spectral(sample_index, units.ctypes.data, len(units), q.ctypes.data, meta.ctypes.data, spec.ctypes.data)
        assert rc == 0
        return spec

    def plan_refresh(self, first, nxt, max_streams, max_channels, tns_spec=False, sample_index=3):
        """The host planner's refresh of a kept plan (aacg_plan_refresh_host): 0 or the AACG_ERR_* code."""
        first, nxt = np.ascontiguousarray(first), np.ascontiguousarray(nxt)
        assert len(first) == len(nxt)
        return self.lib.emu_plan_refresh(first.ctypes.data, nxt.ctypes.data, len(first), sample_index, max_streams, max_channels, 1 if tns_spec else 0)

    def decode_pipelined(self, units, coeffs_list, meta_list, n_pcm, pool, parity, cells, heads, order=0, epoch_in=0, sample_index=3, streams=0):
        """aacg_decode_pipelined for len(coeffs_list) consecutive launches of ONE plan, workgroup by workgroup in an order the
        engine's rules allow (order: 0 launch after launch, 1 the last launch of every round of streams first, >= 2 random interleaving
        with that seed; streams: how many the sequence takes in turn, 0 = the engine's choice for the plan).  cells: uint64 [S][C][OV_BUFFERS][4] (aacg_xl_cell), heads: like pool.  Returns (list of PCM arrays, epoch of the
        last launch: pass it as epoch_in to continue the sequence with the last launch 'still in flight')."""
        units = np.ascontiguousarray(units)
        n = len(coeffs_list)
        coeffs_list = [np.ascontiguousarray(c) for c in coeffs_list]
        kind = 1 if coeffs_list[0].dtype == np.int16 else 0
        meta_list = [np.ascontiguousarray(m, np.uint16) for m in meta_list] if meta_list is not None else None
        pcm = [np.full(n_pcm, np.nan, np.float32) for _ in range(n)]
        cp = (C.c_void_p * n)(*[c.ctypes.data for c in coeffs_list])
        mp = (C.c_void_p * n)(*[m.ctypes.data for m in meta_list]) if meta_list is not None else None
        pp = (C.c_void_p * n)(*[x.ctypes.data for x in pcm])
        last = C.c_uint64(0)
        rc = self.lib.emu_decode_pipelined(kind, sample_index, pool.shape[0], pool.shape[1], units.ctypes.data, len(units), n, cp, mp, pp, n_pcm,
                                           pool.ctypes.data, parity.ctypes.data, cells.ctypes.data, heads.ctypes.data, order, epoch_in, C.byref(last), streams)
        if rc:
            self._raise("emu_decode_pipelined", rc)
        return pcm, last.value

    def plan(self, units, max_streams, max_channels, parity=None, sample_index=3):
        units = np.ascontiguousarray(units)
        runs = np.zeros(len(units) + 8, RUN_DTYPE)
        info = np.zeros(4, np.int32)
        n = self.lib.emu_plan(units.ctypes.data, len(units), sample_index, max_streams, max_channels,
                              parity.ctypes.data if parity is not None else None, runs.ctypes.data, len(runs), info.ctypes.data)
        return n, runs[:max(n, 0)], info

    def windows(self, sample_index=3):
        a = np.zeros(2304, np.float32)
        assert self.lib.emu_get_windows(sample_index, a.ctypes.data) == 0
        return a[:1024], a[1024:2048], a[2048:2176], a[2176:]

    def iq_sf(self):
        iq = np.zeros(8192, np.float32); sf = np.zeros(428, np.float32)
        assert self.lib.emu_get_iq_sf(iq.ctypes.data, sf.ctypes.data) == 0
        return iq, sf


def pool_current(pool, parity):
    """[S][C][1024] copy of the live overlap buffers at the reference's scale (the pool is PCM-scaled, like the engine's:
    aacg_get_overlap multiplies by 32768 too)."""
    S, Cn = pool.shape[:2]
    out = np.empty((S, Cn, 1024), np.float32)
    for s in range(S):
        for c in range(Cn):
            out[s, c] = pool[s, c, parity[s * Cn + c]] * np.float32(32768.0)
    return out


def emu_parse(emu, sample_index, entries, counts, data, frames, max_units, max_channels, options, want_tns):
    """The device front end's kernel source (aacg_parse.h) run on the CPU: same outputs as aacgpu.Parser.parse_batch."""
    import aacgpu
    data = np.ascontiguousarray(data, np.uint8)
    frames = np.ascontiguousarray(frames)
    entries = np.ascontiguousarray(entries)
    counts = np.ascontiguousarray(counts, np.uint32)
    out = aacgpu.alloc_parse_outputs(len(frames), max_units, max_channels, want_tns)
    f = emu.lib.emu_parse
    f.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    rc = f(sample_index, entries.ctypes.data, counts.ctypes.data, data.ctypes.data, data.size, frames.ctypes.data, len(frames),
           max_units, max_channels, options, out["units"].ctypes.data, out["q"].ctypes.data, out["meta"].ctypes.data,
           out["tns"].ctypes.data if want_tns else None, out["results"].ctypes.data)
    if rc:
        raise RuntimeError("emu_parse rc=%d: %s" % (rc, emu.error()))
    return out
