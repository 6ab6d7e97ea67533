"""The resident route's way out with a feature stage as its last stage (aac.js_amd/csrc/aacg_pipe_exit.h: AACG_EXIT_FEATURES): the rows with
the stage present, for host and both device layouts, with and without mix and resampler, against the table written out here
independently; that a pipeline WITHOUT the stage yields exactly the rows tests/test_pipe_exit_plan.py pins, through the new driver too;
the host staging's capacity; and the feature meaning of stride_frames in aacg_pipeline_submit_device's pure refusals.  Host code through
tests/emu/exit_features_emu.cpp; no GPU."""
import ctypes as C
import itertools

import numpy as np
import pytest

import emu_lib
import features_kit
import test_pipe_exit_plan as base

NONE, LANE_PCM, LANE_MIX, LANE_RS, LANE_HOST, CALLER, LANE_FT = range(7)         # AACG_EXIT_BUF_NONE ..
PINNED, PAGEABLE, DEV_PACKED, DEV_PLANAR = range(4)
XFORM, MIX, RESAMPLE, TAIL, FEATURES = range(5)                                  # AACG_EXIT_XFORM ..
TAIL_NONE, PLANAR_LAUNCH, COPY_DOWN = range(3)
INVALID_ARG, CAPACITY = -1, -4
PCM_PACKED, PCM_PLANAR = 0, 1

# the batch of test_pipe_exit_plan.py: two streams of 1 and 3 frames (resampled 1 / 3: 342 and 1024 samples); the stage is Whisper's
# (400 / 160, centred, 80 bands) and the slots' feature clocks stand at 0 and 1000
K, H, P, N_MELS = 400, 160, 200, 80
FT_CLOCKS = (0, 1000)
MAX_STREAMS, MAX_FRAMES = base.MAX_STREAMS, base.MAX_FRAMES


def ft_out(rs):
    samples = base.N_OUT if rs else [1024 * f for f in base.FRAMES]
    return [features_kit.count(c + n, K, H, P) - features_kit.count(c, K, H, P) for c, n in zip(FT_CLOCKS, samples)]


def ft_lane_elems(rs):
    most_samples = base.lane_elems(1, *base.LM) if rs else MAX_STREAMS * MAX_FRAMES * 1024
    return (most_samples // H + MAX_STREAMS) * N_MELS


MATRIX = list(itertools.product((PINNED, PAGEABLE, DEV_PACKED, DEV_PLANAR), (0, 1), (False, True), (2, 4), (1, 2, 6), (7, 30)))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    L = emu_lib.build_driver("exit_features_emu", ["tests/emu/exit_features_emu.cpp"], tmp_path_factory.mktemp("exit_features_emu"))
    L.emu_exit_plan.argtypes = [C.c_void_p] * 3
    L.emu_exit_plan.restype = None
    L.emu_exit_host_capacity.argtypes, L.emu_exit_host_capacity.restype = [C.c_void_p], C.c_uint64
    L.emu_exit_features_most.argtypes, L.emu_exit_features_most.restype = [C.c_uint32, C.c_uint64, C.c_uint32], C.c_uint64
    L.emu_exit_check.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int32, C.c_uint32, C.c_void_p, C.c_char_p, C.c_uint32]
    return L


def pipe_words(channels, O, rs, E, features=True):
    return np.array(list(base.pipe_words(channels, O, rs, E)) + ([N_MELS, ft_lane_elems(rs)] if features else [0, 0]), np.uint64)


def batch_words(dest, stride, rs, features=True, n_ft=None):
    n_ft = ft_out(rs) if n_ft is None else n_ft
    return np.array(list(base.batch_words(dest, stride, rs)) + ([max(n_ft), sum(n_ft)] if features else [0, 0]), np.uint64)


def plan(lib, pipe, batch):
    out = np.zeros(32, np.uint64)
    lib.emu_exit_plan(pipe.ctypes.data, batch.ctypes.data, out.ctypes.data)
    o = [int(v) for v in out]
    stages = [tuple(o[7 + 5 * i:12 + 5 * i]) for i in range(o[0])]               # (what, src, dst, tail, bytes)
    return {"stages": stages, "row": o[1], "xform_bytes": o[2], "out_bytes": o[3], "device_need": o[4], "collect_copy": bool(o[5]), "ft_row": o[6]}


def table(dest, O, rs, E, channels, stride):
    """The issue's rows with the stage present, every stage's source and destination stated on its own"""
    Oc = O or channels
    planar, host = dest == DEV_PLANAR, dest in (PINNED, PAGEABLE)
    out_bytes = sum(ft_out(rs)) * N_MELS * 4
    stages = [(XFORM, NONE, LANE_PCM, TAIL_NONE, base.N * channels * 1024 * E)]
    if O:
        stages.append((MIX, LANE_PCM, LANE_MIX, TAIL_NONE, base.N * O * 1024 * E))
    if rs:
        stages.append((RESAMPLE, LANE_MIX if O else LANE_PCM, LANE_RS, TAIL_NONE, sum(base.N_OUT) * Oc * E))      # LANE_RS even for a device batch
    stages.append((FEATURES, LANE_RS if rs else LANE_MIX if O else LANE_PCM, LANE_FT if host else CALLER, TAIL_NONE, out_bytes))
    if host:
        stages.append((TAIL, LANE_FT, CALLER if dest == PINNED else LANE_HOST, COPY_DOWN, out_bytes))             # and never a PLANAR_LAUNCH tail
    return {"stages": stages, "row": 0, "xform_bytes": base.N * channels * 1024 * E, "out_bytes": out_bytes,
            "device_need": len(base.FRAMES) * N_MELS * stride * 4 if planar else out_bytes if dest == DEV_PACKED else 0, "collect_copy": dest == PAGEABLE,
            "ft_row": stride if planar else 0}


def test_counts_are_the_formula_s():
    assert ft_out(False) == [6, 19] and ft_out(True) == [1, 6]                   # floor(824 / 160) + 1; count(4072) - count(1000) = 25 - 6; count(342); count(2024) - 6


def test_plan_with_the_stage_is_the_table(lib):
    for case in MATRIX:
        dest, O, rs, E, channels, stride = case
        got = plan(lib, pipe_words(channels, O, rs, E), batch_words(dest, stride, rs))
        assert got == table(*case), case
        st = got["stages"]
        for before, after in zip(st, st[1:]):
            assert after[1] == before[2], case                                   # a chain
        assert [i for i, s in enumerate(st) if s[2] == CALLER] == ([] if dest == PAGEABLE else [len(st) - 1]), case
        assert all(s[3] != PLANAR_LAUNCH for s in st) and len(st) <= 5, case


def test_plan_without_the_stage_is_what_it_was(lib):
    """the new fields at zero: row for row the table tests/test_pipe_exit_plan.py pins, for all of its cases"""
    for case in base.MATRIX:
        dest, O, rs, E, channels, stride = case
        got = plan(lib, pipe_words(channels, O, rs, E, features=False), batch_words(dest, stride, rs, features=False))
        assert got.pop("ft_row") == 0 and got == base.table(*case), case
        assert len(got["stages"]) <= 4 and all(s[0] != FEATURES and LANE_FT not in s[1:3] for s in got["stages"]), case


@pytest.mark.parametrize("rs", [False, True])
def test_host_staging_holds_the_largest_batch(lib, rs):
    """max_streams streams of max_frames frames at every feature clock: what leaves never exceeds h_pcm's capacity"""
    most_samples = base.lane_elems(1, *base.LM) if rs else MAX_STREAMS * MAX_FRAMES * 1024
    assert lib.emu_exit_features_most(MAX_STREAMS, most_samples, H) * N_MELS == ft_lane_elems(rs)
    pipe = pipe_words(1, 0, rs, 4)
    cap = lib.emu_exit_host_capacity(pipe.ctypes.data)
    assert cap == ft_lane_elems(rs) * 4
    per_stream = most_samples // MAX_STREAMS + 1
    worst = max(features_kit.count(c + per_stream, K, H, P) - features_kit.count(c, K, H, P) for c in range(0, 3 * K))
    b = batch_words(PINNED, 0, rs, n_ft=[worst] * MAX_STREAMS)
    assert plan(lib, pipe, b)["out_bytes"] <= cap


def check(lib, rs, layout, stride, d_pcm=0x10000, room=0, items=1):
    pipe = pipe_words(1, 0, rs, 4)
    batch = batch_words(DEV_PLANAR if layout == PCM_PLANAR else DEV_PACKED, stride, rs)
    need = plan(lib, pipe, batch)["device_need"]
    late, text = C.c_int(-1), C.create_string_buffer(256)
    code = lib.emu_exit_check(pipe.ctypes.data, batch.ctypes.data, d_pcm, max(need + room, 0), layout, items, C.byref(late), text, 256)
    return code, late.value, text.value.decode(), need


def test_stride_frames_counts_feature_frames(lib):
    """planar rows hold FEATURE frames: 19 is the batch's longest count (6 with the resampler) — far below a frame's 1024 samples, which
    is what the stride counts without the stage — and the planar launch's item limit has no part in it"""
    for rs, longest in ((False, 19), (True, 6)):
        assert check(lib, rs, PCM_PLANAR, longest, items=0)[:3] == (0, 0, "")
        assert check(lib, rs, PCM_PLANAR, 1 << 21)[0] == 0 and check(lib, rs, PCM_PACKED, 0)[0] == 0
        code, late, text, _ = check(lib, rs, PCM_PLANAR, longest - 1)
        assert (code, late) == (INVALID_ARG, 0) and "stride_frames is below a stream's count of feature frames" in text
        for stride in (0, (1 << 21) + 1):
            code, late, text, _ = check(lib, rs, PCM_PLANAR, stride)
            assert (code, late) == (INVALID_ARG, 0) and "stride_frames is not in 1..2^21" in text
        for layout, stride in ((PCM_PLANAR, longest), (PCM_PACKED, 0)):
            code, late, text, need = check(lib, rs, layout, stride, room=-1)
            assert (code, late) == (CAPACITY, 1) and "(%d bytes)" % need in text
        assert "not 16-byte aligned" in check(lib, rs, PCM_PLANAR, longest, d_pcm=0x10008)[2]
        assert "unknown layout" in check(lib, rs, 2, 0)[2] and "takes stride_frames 0" in check(lib, rs, PCM_PACKED, 3)[2]
