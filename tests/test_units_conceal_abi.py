"""The conceal stage's surface (include/aacgpu.h: aacg_plan_conceal_refused, aacg_pipeline_set_concealment): the header's text for the
rule, the symbols and the records, the ABI version, and the refusals that need no device.  No GPU."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import aacgpu
import conceal_kit as kit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = -1
SYMBOLS = ("aacg_conceal_state_bytes", "aacg_plan_conceal_refused", "aacg_pipeline_set_concealment", "aacg_pipeline_concealed")


def test_library_exports_the_new_symbols(engine_lib):
    for name in SYMBOLS:
        assert name in aacgpu.ABI_SYMBOLS and hasattr(engine_lib, name), name
    T = aacgpu.ConcealConfig
    assert [n for n, _ in T._fields_] == ["fade_steps", "hold_frames"] and (C.sizeof(T), T.hold_frames.offset) == (8, 4)
    assert engine_lib.aacg_abi_version() == 6                              # new symbols and one flag bit: no struct changed
    assert aacgpu.PARSE_CONCEALED == 0x8 and (aacgpu.CONCEAL_FADE_STEPS, aacgpu.CONCEAL_HOLD_FRAMES) == (2, 6)


def test_the_header_states_the_rule():
    text = open(os.path.join(ROOT, "include", "aacgpu.h")).read()
    assert re.search(r"#define AACG_ABI_VERSION\s+6\b", text) and re.search(r"#define AACG_PARSE_CONCEALED\s+0x8\b", text)
    flat = re.sub(r"\s+", " ", re.sub(r"\n \*", "\n", text))      # the comment's lines joined
    for phrase in ("THE RULE.", "r := min(r + 1, hold_frames + 1)", "If G exists and r <= hold_frames the frame is CONCEALED",
                   "max(0, sf - r * fade_steps)", "0, 13, 14 and 15 are copied unchanged", "bits 9..11 are kept", "status, n_units, bits_used and the refusal count are NOT changed",
                   "window_shape_prev is left to the carry stage", "never a concealed frame", "plan_mode 0", "fade_steps 0..64, hold_frames 1..255"):
        assert phrase in flat, phrase
    # the pipeline's configuration is what it was: the stage is set by a call, not by a field
    cfg = re.search(r"typedef struct aacg_pipeline_config \{(.*?)\} aacg_pipeline_config;", text, re.S).group(1)
    assert "conceal" not in cfg and "int32_t reserved[1];" in cfg


def test_record_layouts_match_the_header():
    src = r'''
    #include "include/aacgpu.h"
    #include <stddef.h>
    int sizes[] = { sizeof(aacg_conceal_stream), offsetof(aacg_conceal_stream, slot), offsetof(aacg_conceal_stream, state), sizeof(aacg_conceal_config),
                    sizeof(aacg_parse_result), sizeof(aacg_pipeline_config), AACG_PARSE_CONCEALED };
    '''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        so = os.path.join(d, "s.so")
        subprocess.run(["gcc", "-shared", "-fPIC", "-I", ROOT, "-o", so, os.path.join(d, "s.c")], check=True)
        arr = (C.c_int * 7).in_dll(C.CDLL(so), "sizes")
        assert list(arr) == [32, 16, 24, 8, 8, C.sizeof(aacgpu.PipelineConfig), 8]
    assert kit.STREAM_DTYPE.itemsize == 32 and kit.STREAM_DTYPE.fields["state"][1] == 24


def test_state_bytes(engine_lib):
    lib = aacgpu.load_library()
    for slots, cp in ((1, 1), (3, 2), (4096, 8)):
        assert lib.aacg_conceal_state_bytes(slots, cp) == slots * 2 * kit.side_bytes(cp)
    assert lib.aacg_conceal_state_bytes(3, 0) == 0 and lib.aacg_conceal_state_bytes(3, 9) == 0


def test_null_handle_refusals(engine_lib):
    """every call answers a null handle without a device, and writes nothing"""
    lib, n = aacgpu.load_library(), C.c_uint64(77)
    assert lib.aacg_pipeline_set_concealment(None, C.byref(aacgpu.ConcealConfig(2, 6))) == INVALID_ARG
    assert lib.aacg_pipeline_concealed(None, C.byref(n)) == INVALID_ARG and n.value == 77
    assert lib.aacg_plan_conceal_refused(None, None, 0, None, None, None, 2, None, 1, 1, None, 1, 2, 6, None) == INVALID_ARG
