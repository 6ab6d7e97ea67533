"""The resident route's way out with a trim as its last PCM stage (aac.js_amd/csrc/aacg_pipe_exit.h: AACG_EXIT_TRIM): every row with the
stage present — four destinations, with and without mix, limiter, resampler and feature stage — against the table written out here
independently; batches that keep nothing; the planar refusals; and that a pipeline WITHOUT the stage yields exactly the rows the earlier
tests pin, through the new driver too.  Host code through tests/emu/exit_trim_emu.cpp; no GPU."""
import ctypes as C
import itertools

import numpy as np
import pytest

import emu_lib
import test_pipe_exit_features as feat
import test_pipe_exit_limit as lim
import test_pipe_exit_plan as base
import trim_kit

NONE, LANE_PCM, LANE_MIX, LANE_RS, LANE_HOST, CALLER, LANE_FT, LANE_LIM, LANE_TRIM = range(9)    # AACG_EXIT_BUF_NONE ..
PINNED, PAGEABLE, DEV_PACKED, DEV_PLANAR = range(4)
XFORM, MIX, RESAMPLE, TAIL, FEATURES, LIMIT, TRIM = range(7)                                      # AACG_EXIT_XFORM ..
TAIL_NONE, PLANAR_LAUNCH, COPY_DOWN = range(3)
PCM_PACKED, PCM_PLANAR = 0, 1
INVALID_ARG, CAPACITY = -1, -4

# the windows and positions of the batch's two streams: what they keep of what the stage receives, without and with the resampler
WINDOWS = [(0, 300, 500), (7, 2000, None)]                                                        # (Q, skip, keep)


def kept(rs, windows=WINDOWS):
    n_in = base.N_OUT if rs else [1024 * f for f in base.FRAMES]
    return [trim_kit.span(q, s, k, n)[1] for (q, s, k), n in zip(windows, n_in)]


# (dest, O, resampler, E, channels, stride, limiter)
MATRIX = list(itertools.product((PINNED, PAGEABLE, DEV_PACKED, DEV_PLANAR), (0, 1, 2), (False, True), (2, 4), (1, 2, 6), (2, 7), (False, True)))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    L = emu_lib.build_driver("exit_trim_emu", ["tests/emu/exit_trim_emu.cpp"], tmp_path_factory.mktemp("exit_trim_emu"))
    L.emu_exit_plan.argtypes = [C.c_void_p] * 3
    L.emu_exit_plan.restype = None
    L.emu_exit_host_capacity.argtypes, L.emu_exit_host_capacity.restype = [C.c_void_p], C.c_uint64
    L.emu_exit_check.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int32, C.c_uint32, C.c_void_p, C.c_char_p, C.c_uint32]
    return L


def pipe_words(channels, O, rs, E, ft, limited, trimmed):
    return np.array(list(lim.pipe_words(channels, O, rs, E, ft, limited)) + [1 if trimmed else 0], np.uint64)


def batch_words(dest, stride, rs, ft, n_keep, n_ft=None):
    return np.array(list(feat.batch_words(dest, stride, rs, features=ft, n_ft=n_ft)) + [max(n_keep), sum(n_keep)], np.uint64)


def plan(lib, pipe, batch):
    out = np.zeros(42, np.uint64)
    lib.emu_exit_plan(pipe.ctypes.data, batch.ctypes.data, out.ctypes.data)
    o = [int(v) for v in out]
    stages = [tuple(o[7 + 5 * i:12 + 5 * i]) for i in range(o[0])]                                # (what, src, dst, tail, bytes)
    return {"stages": stages, "row": o[1], "xform_bytes": o[2], "out_bytes": o[3], "device_need": o[4], "collect_copy": bool(o[5]), "ft_row": o[6]}


def table(dest, O, rs, E, channels, stride, limited, n_keep):
    """The issue's rows with the trim present and no feature stage, every stage's source and destination stated on its own"""
    Oc = O or channels
    planar, host = dest == DEV_PLANAR, dest in (PINNED, PAGEABLE)
    pcm_bytes = base.N * Oc * 1024 * E
    stages = [(XFORM, NONE, LANE_PCM, TAIL_NONE, base.N * channels * 1024 * E)]                   # lane buffers whatever the destination, as in front of a limiter
    if O:
        stages.append((MIX, LANE_PCM, LANE_MIX, TAIL_NONE, pcm_bytes))
    if limited:
        stages.append((LIMIT, LANE_MIX if O else LANE_PCM, LANE_LIM, TAIL_NONE, pcm_bytes))
    front = LANE_LIM if limited else LANE_MIX if O else LANE_PCM
    if rs:
        stages.append((RESAMPLE, front, LANE_RS, TAIL_NONE, sum(base.N_OUT) * Oc * E))
    out_bytes = sum(n_keep) * Oc * E
    stages.append((TRIM, LANE_RS if rs else front, LANE_TRIM if host else CALLER, TAIL_NONE, out_bytes))
    if host:                                                                                      # no PLANAR_LAUNCH tail: the trim wrote the tensor
        stages.append((TAIL, LANE_TRIM, CALLER if dest == PINNED else LANE_HOST, COPY_DOWN, out_bytes))
    need = len(base.FRAMES) * Oc * stride * 1024 * E if planar else out_bytes if dest == DEV_PACKED else 0
    return {"stages": stages, "row": stride * 1024 if planar else 0, "xform_bytes": base.N * channels * 1024 * E, "out_bytes": out_bytes,
            "device_need": need, "collect_copy": dest == PAGEABLE, "ft_row": 0}


def test_counts_are_the_rule_s():
    assert kept(False) == [500, 1079] and kept(True) == [42, 0]                                   # [300, 800) of 1024; [2000, 3079) of [7, 3079); [300, 342); nothing of [7, 1031)


def test_plan_with_the_stage_is_the_table(lib):
    seen = set()
    for case in MATRIX:
        dest, O, rs, E, channels, stride, limited = case
        n_keep = kept(rs)
        got = plan(lib, pipe_words(channels, O, rs, E, False, limited, True), batch_words(dest, stride, rs, False, n_keep))
        assert got == table(dest, O, rs, E, channels, stride, limited, n_keep), case
        st = got["stages"]
        assert st[0][1] == NONE and all(after[1] == before[2] for before, after in zip(st, st[1:])), case      # a chain
        assert [i for i, s in enumerate(st) if s[2] == CALLER] == ([] if dest == PAGEABLE else [len(st) - 1]), case
        assert len(st) <= 6 and [s[0] for s in st].count(TRIM) == 1 and all(s[3] != PLANAR_LAUNCH for s in st), case
        seen.add((dest, bool(O), rs, limited))
        # the staging's capacity does not know the stage: it never emits more than it receives
        assert lib.emu_exit_host_capacity(pipe_words(channels, O, rs, E, False, limited, True).ctypes.data) == \
            lib.emu_exit_host_capacity(pipe_words(channels, O, rs, E, False, limited, False).ctypes.data)
    assert len(seen) == 4 * 2 * 2 * 2                                                             # each destination with and without mix, resampler, limiter


def test_with_a_feature_stage_there_is_no_trim_row(lib):
    """the feature stage reads each stream's kept range where it lies: the plan is the one without the trim, with the ft_* the caller
    derived from the trimmed counts"""
    for dest, (O, channels), rs, E, limited, stride in itertools.product((PINNED, PAGEABLE, DEV_PACKED, DEV_PLANAR), ((0, 1), (1, 2), (1, 6)), (False, True), (2, 4), (False, True), (30,)):
        for n_ft in (feat.ft_out(rs), [2, 0], [0, 0]):
            n_keep = kept(rs)
            got = plan(lib, pipe_words(channels, O, rs, E, True, limited, True), batch_words(dest, stride, rs, True, n_keep, n_ft))
            bare = plan(lib, pipe_words(channels, O, rs, E, True, limited, False), batch_words(dest, stride, rs, True, [0, 0], n_ft))
            assert got == bare and all(s[0] != TRIM and LANE_TRIM not in s[1:3] for s in got["stages"]), (dest, O, rs, E, limited, n_ft)
            assert got["out_bytes"] == sum(n_ft) * feat.N_MELS * 4 and got["stages"][-1 if dest in (DEV_PACKED, DEV_PLANAR) else -2][0] == FEATURES
            if n_ft == feat.ft_out(rs):
                want = lim.table(dest, O, rs, E, channels, stride, True) if limited else feat.table(dest, O, rs, E, channels, stride)
                assert got == want, (dest, O, rs, E, limited)


def test_a_batch_that_keeps_nothing(lib):
    """out_bytes 0 in every row behind the stage; a planar destination still needs its whole block (its zeros)"""
    for dest, O, rs, E, channels, limited in itertools.product((PINNED, PAGEABLE, DEV_PACKED, DEV_PLANAR), (0, 2), (False, True), (2, 4), (1, 6), (False, True)):
        got = plan(lib, pipe_words(channels, O, rs, E, False, limited, True), batch_words(dest, 1, rs, False, [0, 0]))
        assert got == table(dest, O, rs, E, channels, 1, limited, [0, 0])
        assert got["out_bytes"] == 0 and all(s[4] == 0 for s in got["stages"] if s[0] in (TRIM, TAIL))
        assert got["device_need"] == (len(base.FRAMES) * (O or channels) * 1024 * E if dest == DEV_PLANAR else 0)
    # one stream keeps, the other does not
    got = plan(lib, pipe_words(2, 0, False, 4, False, False, True), batch_words(DEV_PACKED, 0, False, False, [0, 5]))
    assert got["out_bytes"] == got["device_need"] == 5 * 2 * 4


def check(lib, rs, layout, stride, n_keep, d_pcm=0x10000, room=0, items=1, trimmed=True):
    pipe = pipe_words(2, 0, rs, 4, False, False, trimmed)
    batch = batch_words(DEV_PLANAR if layout == PCM_PLANAR else DEV_PACKED, stride, rs, False, n_keep)
    need = plan(lib, pipe, batch)["device_need"]
    late, text = C.c_int(-1), C.create_string_buffer(256)
    code = lib.emu_exit_check(pipe.ctypes.data, batch.ctypes.data, d_pcm, max(need + room, 0), layout, items, C.byref(late), text, 256)
    return code, late.value, text.value.decode(), need


def test_planar_refusals(lib):
    """rows hold KEPT samples: stride_frames x 1024 at least every n_keep, in 1..2^21 — not the batch's frame counts, and the planar
    launch's item limit has no part in it"""
    for rs in (False, True):
        assert check(lib, rs, PCM_PLANAR, 1, [500, 1024], items=0)[:3] == (0, 0, "")              # below the largest frame count (3): the rows are the trim's
        assert check(lib, rs, PCM_PLANAR, 2, [500, 1079], items=0)[:3] == (0, 0, "") and check(lib, rs, PCM_PLANAR, 1 << 21, [0, 0])[0] == 0
        assert check(lib, rs, PCM_PLANAR, 1, [0, 0])[:3] == (0, 0, "") and check(lib, rs, PCM_PACKED, 0, [0, 0])[:3] == (0, 0, "")
        code, late, text, _ = check(lib, rs, PCM_PLANAR, 1, [500, 1025])
        assert (code, late) == (INVALID_ARG, 0) and "stride_frames x 1024 is below a stream's trimmed count" in text
        for stride in (0, (1 << 21) + 1):
            code, late, text, _ = check(lib, rs, PCM_PLANAR, stride, [0, 0])
            assert (code, late) == (INVALID_ARG, 0) and "stride_frames is not in 1..2^21" in text
        code, late, text, need = check(lib, rs, PCM_PLANAR, 2, [500, 1079], room=-1)
        assert (code, late) == (CAPACITY, 1) and "(%d bytes)" % need in text and need == 2 * 2 * 2 * 1024 * 4
        code, late, text, need = check(lib, rs, PCM_PACKED, 0, [500, 1079], room=-1)
        assert (code, late) == (CAPACITY, 1) and need == 1579 * 2 * 4
        assert check(lib, rs, PCM_PACKED, 3, [0, 0])[0] == INVALID_ARG and check(lib, rs, PCM_PACKED, 0, [1, 1], d_pcm=0x10008)[0] == INVALID_ARG
    # without the stage the parent's refusals stand: the stride counts frames
    code, late, text, _ = check(lib, False, PCM_PLANAR, 2, [0, 0], trimmed=False)
    assert code == INVALID_ARG and "below the batch's largest frame count" in text


def test_plan_without_the_stage_is_what_it_was(lib):
    """the new fields at zero: row for row the tables the earlier tests pin, for all of their cases — whatever tr_most and tr_total hold"""
    for tr in ([0, 0], [5, 9]):
        for case in base.MATRIX:
            dest, O, rs, E, channels, stride = case
            got = plan(lib, pipe_words(channels, O, rs, E, False, False, False), batch_words(dest, stride, rs, False, tr))
            assert got.pop("ft_row") == 0 and got == base.table(*case), case
        for case in feat.MATRIX:
            dest, O, rs, E, channels, stride = case
            assert plan(lib, pipe_words(channels, O, rs, E, True, False, False), batch_words(dest, stride, rs, True, tr)) == feat.table(*case), case
        for case in lim.MATRIX:
            dest, O, rs, E, channels, stride, ft = case
            got = plan(lib, pipe_words(channels, O, rs, E, ft, True, False), batch_words(dest, stride, rs, ft, tr))
            assert got == lim.table(*case), case
            assert all(s[0] != TRIM and LANE_TRIM not in s[1:3] for s in got["stages"]), case
