"""The resident route's way out with a limiter between the mix and the resampler (aac.js_amd/csrc/aacg_pipe_exit.h: AACG_EXIT_LIMIT): every
row with the stage present — each destination, with and without mix, resampler and feature stage — against the table written out here
independently; that a pipeline WITHOUT the stage yields exactly the rows tests/test_pipe_exit_plan.py and tests/test_pipe_exit_features.py
pin, through the new driver too; and that what leaves, what a device buffer must hold and the host staging's capacity do not know the
stage.  Host code through tests/emu/exit_limit_emu.cpp; no GPU."""
import ctypes as C
import itertools

import numpy as np
import pytest

import emu_lib
import test_pipe_exit_features as feat
import test_pipe_exit_plan as base

NONE, LANE_PCM, LANE_MIX, LANE_RS, LANE_HOST, CALLER, LANE_FT, LANE_LIM = range(8)    # AACG_EXIT_BUF_NONE ..
PINNED, PAGEABLE, DEV_PACKED, DEV_PLANAR = range(4)
XFORM, MIX, RESAMPLE, TAIL, FEATURES, LIMIT = range(6)                                # AACG_EXIT_XFORM ..
TAIL_NONE, PLANAR_LAUNCH, COPY_DOWN = range(3)

# (dest, O, resampler, E, channels, stride, feature stage): the feature stage takes one channel, so it goes with a mix to 1 or mono
MATRIX = [c + (False,) for c in itertools.product((PINNED, PAGEABLE, DEV_PACKED, DEV_PLANAR), (0, 1, 2), (False, True), (2, 4), (1, 2, 6), (7,))]
MATRIX += [(d, O, rs, E, ch, 30, True) for d, (O, ch), rs, E in itertools.product((PINNED, PAGEABLE, DEV_PACKED, DEV_PLANAR), ((0, 1), (1, 2), (1, 6)), (False, True), (2, 4))]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    L = emu_lib.build_driver("exit_limit_emu", ["tests/emu/exit_limit_emu.cpp"], tmp_path_factory.mktemp("exit_limit_emu"))
    L.emu_exit_plan.argtypes = [C.c_void_p] * 3
    L.emu_exit_plan.restype = None
    L.emu_exit_host_capacity.argtypes, L.emu_exit_host_capacity.restype = [C.c_void_p], C.c_uint64
    return L


def pipe_words(channels, O, rs, E, ft, limited):
    return np.array(list(feat.pipe_words(channels, O, rs, E, features=ft)) + [1 if limited else 0], np.uint64)


def plan(lib, pipe, batch):
    out = np.zeros(37, np.uint64)
    lib.emu_exit_plan(pipe.ctypes.data, batch.ctypes.data, out.ctypes.data)
    o = [int(v) for v in out]
    stages = [tuple(o[7 + 5 * i:12 + 5 * i]) for i in range(o[0])]                    # (what, src, dst, tail, bytes)
    return {"stages": stages, "row": o[1], "xform_bytes": o[2], "out_bytes": o[3], "device_need": o[4], "collect_copy": bool(o[5]), "ft_row": o[6]}


def table(dest, O, rs, E, channels, stride, ft):
    """The issue's rows with the limiter present, every stage's source and destination stated on its own"""
    Oc = O or channels
    packed, planar, host = dest == DEV_PACKED, dest == DEV_PLANAR, dest in (PINNED, PAGEABLE)
    pcm_bytes = base.N * Oc * 1024 * E
    stages = [(XFORM, NONE, LANE_PCM, TAIL_NONE, base.N * channels * 1024 * E)]       # a lane buffer whatever the destination
    if O:
        stages.append((MIX, LANE_PCM, LANE_MIX, TAIL_NONE, base.N * O * 1024 * E))    # ... and so the mix
    stages.append((LIMIT, LANE_MIX if O else LANE_PCM, CALLER if packed and not rs and not ft else LANE_LIM, TAIL_NONE, pcm_bytes))
    if rs:
        stages.append((RESAMPLE, LANE_LIM, LANE_RS if host or ft else CALLER, TAIL_NONE, sum(base.N_OUT) * Oc * E))
    if ft:
        out_bytes = sum(feat.ft_out(rs)) * feat.N_MELS * 4
        stages.append((FEATURES, LANE_RS if rs else LANE_LIM, LANE_FT if host else CALLER, TAIL_NONE, out_bytes))
        need = len(base.FRAMES) * feat.N_MELS * stride * 4 if planar else out_bytes if packed else 0
    else:
        out_bytes = sum(base.N_OUT) * Oc * E if rs else pcm_bytes
        need = len(base.FRAMES) * Oc * stride * 1024 * E if planar else out_bytes if packed else 0
    last_lane = LANE_FT if ft else LANE_RS if rs else LANE_LIM
    if planar and not rs and not ft:
        stages.append((TAIL, LANE_LIM, CALLER, PLANAR_LAUNCH, out_bytes))
    elif host:
        stages.append((TAIL, last_lane, CALLER if dest == PINNED else LANE_HOST, COPY_DOWN, out_bytes))
    return {"stages": stages, "row": stride * 1024 if planar and rs and not ft else 0, "xform_bytes": base.N * channels * 1024 * E, "out_bytes": out_bytes,
            "device_need": need, "collect_copy": dest == PAGEABLE, "ft_row": stride if planar and ft else 0}


def test_plan_with_the_stage_is_the_table(lib):
    seen = set()
    for case in MATRIX:
        dest, O, rs, E, channels, stride, ft = case
        batch = feat.batch_words(dest, stride, rs, features=ft)
        got = plan(lib, pipe_words(channels, O, rs, E, ft, True), batch)
        assert got == table(*case), case
        st = got["stages"]
        for before, after in zip(st, st[1:]):
            assert after[1] == before[2], case                                        # a chain
        assert [i for i, s in enumerate(st) if s[2] == CALLER] == ([] if dest == PAGEABLE else [len(st) - 1]), case
        assert len(st) <= 6 and [s[0] for s in st].count(LIMIT) == 1, case
        seen.add((dest, bool(O), rs, ft))
        # the stage emits what it receives: what leaves and what a device buffer must hold are what they are without it
        bare = plan(lib, pipe_words(channels, O, rs, E, ft, False), batch)
        for key in ("row", "xform_bytes", "out_bytes", "device_need", "collect_copy", "ft_row"):
            assert got[key] == bare[key], (case, key)
        assert lib.emu_exit_host_capacity(pipe_words(channels, O, rs, E, ft, True).ctypes.data) == lib.emu_exit_host_capacity(pipe_words(channels, O, rs, E, ft, False).ctypes.data)
    assert len(seen) == 4 * 2 * 2 * 2                                                 # each destination with and without mix, resampler, features
    assert max(len(table(*c)["stages"]) for c in MATRIX) == 6                         # transform, mix, limit, resample, features, copy down


def test_plan_without_the_stage_is_what_it_was(lib):
    """the new field at zero: row for row the tables tests/test_pipe_exit_plan.py and tests/test_pipe_exit_features.py pin, for all of
    their cases"""
    for case in base.MATRIX:
        dest, O, rs, E, channels, stride = case
        got = plan(lib, pipe_words(channels, O, rs, E, False, False), feat.batch_words(dest, stride, rs, features=False))
        assert got.pop("ft_row") == 0 and got == base.table(*case), case
        assert all(s[0] != LIMIT and LANE_LIM not in s[1:3] for s in got["stages"]), case
    for case in feat.MATRIX:
        dest, O, rs, E, channels, stride = case
        got = plan(lib, pipe_words(channels, O, rs, E, True, False), feat.batch_words(dest, stride, rs))
        assert got == feat.table(*case), case
        assert all(s[0] != LIMIT and LANE_LIM not in s[1:3] for s in got["stages"]), case
