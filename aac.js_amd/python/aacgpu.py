"""ctypes binding of the C ABI in include/aacgpu.h (aac.js_amd/csrc/libaacgpu.so).

Plumbing only: tests and bench.py drive the HIP path through exactly the entry points a
JavaScript host binds over N-API.  There is no CPU fallback here: if the
library is missing or no GPU is present, calls raise.
"""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
# AACGPU_LIB: A/B another build of the same ABI (tools/ab.sh); default is the in-tree build
LIB_PATH = os.environ.get("AACGPU_LIB") or os.path.join(ROOT, "aac.js_amd", "csrc", "libaacgpu.so")

INPUT_SPEC_F32, INPUT_QUANT_I16 = 0, 1
OUTPUT_F32, OUTPUT_I16 = 0, 1
ERR_NAMES = {0: "OK", -1: "INVALID_ARG", -2: "NO_DEVICE", -3: "OUT_OF_MEMORY", -4: "CAPACITY",
             -5: "UNSUPPORTED", -6: "LAYOUT_CHANGE", -7: "STALE_PLAN", -8: "TIMEOUT"}
ERR_TIMEOUT = -8

# every symbol include/aacgpu.h declares
ABI_SYMBOLS = ["aacg_create", "aacg_destroy", "aacg_last_error", "aacg_abi_version", "aacg_reset_stream",
               "aacg_get_overlap", "aacg_set_overlap", "aacg_decode_batch", "aacg_submit", "aacg_wait",
               "aacg_decode_batch_tns", "aacg_submit_tns", "aacg_plan_create_tns",
               "aacg_host_alloc", "aacg_host_free", "aacg_plan_create", "aacg_plan_destroy",
               "aacg_decode_device", "aacg_spectral_device", "aacg_synchronize", "aacg_get_table", "aacg_kernel_name",
               "aacg_parser_create", "aacg_parser_destroy", "aacg_parser_last_error", "aacg_parse_status_string",
               "aacg_parse_batch", "aacg_parse_device", "aacg_parse_kernel_name", "aacg_plan_refresh_from_parse", "aacg_standard_codebooks",
               "aacg_decode_batch_ex", "aacg_submit_ex", "aacg_plan_create_ex", "aacg_plan_kernels", "aacg_plan_kernels_ex", "aacg_plan_refresh_units",
               "aacg_decode_pipelined", "aacg_pipeline_fork", "aacg_pipeline_join",
               "aacg_pipeline_create", "aacg_pipeline_destroy", "aacg_pipeline_last_error", "aacg_pipeline_reset_stream", "aacg_pipeline_decode",
               "aacg_pipeline_submit", "aacg_pipeline_collect", "aacg_pipeline_set_wait_limit_ms", "aacg_pipeline_stream_layout",
               "aacg_set_wait_limit_ms", "aacg_parser_set_wait_limit_ms", "aacg_pipeline_info",
               "aacg_plan_set_unit_sets", "aacg_plan_refresh_from_parse_ex", "aacg_tns_records_bytes", "aacg_tns_records_from_parse", "aacg_plan_create_stages", "aacg_decode_pipelined_stages", "aacg_parse_walk", "aacg_parse_walk_device",
               "aacg_pipeline_walk_submit", "aacg_pipeline_walk_collect", "aacg_pipeline_decode_ragged", "aacg_pipeline_submit_ragged",
               "aacg_plan_create_shaped", "aacg_plan_create_shaped_stages", "aacg_plan_shape_table", "aacg_plan_shape_launch",
               "aacg_get_window_shape", "aacg_set_window_shape", "aacg_plan_carry_window_shape", "aacg_pipeline_stream_window_shape",
               "aacg_pipeline_submit_device", "aacg_pipeline_wait_device",
               "aacg_pipeline_set_mix", "aacg_pipeline_out_channels", "aacg_mix_standard",
               "aacg_pipeline_set_resample", "aacg_pipeline_out_samples", "aacg_resample_counts", "aacg_resample_design",
               "aacg_pipeline_set_features", "aacg_features_counts", "aacg_features_design",
               "aacg_pipeline_set_loudness", "aacg_pipeline_loudness_out", "aacg_pipeline_loudness_counts", "aacg_loudness_counts",
               "aacg_loudness_design", "aacg_loudness_integrate",
               "aacg_pipeline_set_limiter", "aacg_pipeline_set_gain", "aacg_pipeline_gain", "aacg_limiter_design",
               "aacg_pipeline_set_limiter_true_peak", "aacg_pipeline_limiter_delay", "aacg_trim_design_delay",
               "aacg_pipeline_set_true_peak", "aacg_pipeline_true_peak_out", "aacg_true_peak_design",
               "aacg_conceal_state_bytes", "aacg_plan_conceal_refused", "aacg_pipeline_set_concealment", "aacg_pipeline_concealed",
               "aacg_pipeline_set_trim", "aacg_pipeline_set_stream_trim", "aacg_pipeline_stream_trim", "aacg_trim_counts", "aacg_trim_design"]
# ... and include/aacgpu_tools.h (measurement and diagnostics: bench.py, tools/, tests)
TOOLS_SYMBOLS = ["aacg_calib_copy", "aacg_timer_create", "aacg_timer_record", "aacg_timer_elapsed_ms", "aacg_timer_destroy",
                 "aacg_pipeline_chained", "aacg_pipeline_concurrent", "aacg_decode_pipelined_timed", "aacg_debug_transform", "aacg_debug_set_route", "aacg_debug_route", "aacg_debug_run_kernel",
                 "aacg_debug_pipeline_order", "aacg_pipeline_streams_used", "aacg_debug_set_wait_mode", "aacg_debug_in_flight", "aacg_debug_stall",
                 "aacg_pipeline_plan_builds", "aacg_pipeline_launch_counts"]
WAIT_SPIN, WAIT_YIELD, WAIT_SLEEP, WAIT_BLOCK = 0, 1, 2, 3
# aacg_debug_set_route / aacg_debug_route flags
DEBUG_ROUTE_UNFUSED_COUPLING, DEBUG_ROUTE_RECOMPUTE = 1, 8
ROUTE_PLAN_TNS, ROUTE_PLAN_PNS, ROUTE_PLAN_LONG_CHAINS, ROUTE_PLAN_FULL_LATER_RUNS = 1, 2, 4, 8
ROUTE_PLAN_WIDE_FRAMES, ROUTE_PLAN_CCE_INDEPENDENT, ROUTE_PLAN_CCE_DEPENDENT, ROUTE_PLAN_NO_RUNS = 0x10, 0x20, 0x40, 0x80
ROUTE_PLAN_STAGES = 0x100
# switches of a run kernel (aacg_run_kernels.h), as aacg_debug_run_kernel returns them
RK_QUANT, RK_I16, RK_DD, RK_EX, RK_CPL, RK_RV, RK_NT = 1, 2, 4, 8, 16, 32, 64

UNIT_DTYPE = np.dtype([
    ("stream", "<u4"), ("pcm_offset", "<u4"), ("channel", "<u2"), ("n_out_ch", "<u2"),
    ("n_ch", "u1"), ("flags", "u1"), ("reserved0", "<u2"), ("coef_offset", "<u4"), ("meta_offset", "<u4"),
    ("ch", [("window_sequence", "u1"), ("window_shape", "u1"), ("window_shape_prev", "u1"), ("max_sfb", "u1"),
            ("group_count", "u1"), ("flags", "u1"), ("reserved", "u1", (2,)), ("group_len", "u1", (8,))], (2,)),
    ("tns_offset", "<u4"), ("reserved1", "<u4"),
])
assert UNIT_DTYPE.itemsize == 64

# aacg_tns_info: one per channel with CHAN_TNS_PRESENT (TNS_SPEC engines)
TNS_DTYPE = np.dtype([
    ("n_filt", "u1", (8,)),
    ("filt", [("length", "u1"), ("order", "u1"), ("direction", "u1"), ("reserved", "u1"), ("coef", "<f4", (12,))], (8,)),
])
assert TNS_DTYPE.itemsize == 424
# aacg_dev_tns: the device form of one channel's TNS side info (aacg_tns_records_from_parse; behind a buffer's records, 256-byte
# aligned, lie TNS_M_DOUBLES doubles of transition matrices per record)
DEV_TNS_DTYPE = np.dtype([("start", "<i4", (8,)), ("size", "<i4", (8,)), ("inc", "<i4", (8,)), ("order", "<i4", (8,)), ("lpc", "<f4", (8, 12))])
assert DEV_TNS_DTYPE.itemsize == 512
TNS_M_DOUBLES = 3 * 12 * 12
# aacg_cce_info: one per coupling channel element (CCE_SPEC engines; units flagged UNIT_CCE, reserved1 = its index)
CCE_DTYPE = np.dtype([("coupling_point", "u1"), ("n_targets", "u1"), ("reserved", "u1", (2,)),
                      ("target", [("channel", "u1"), ("gain_list", "u1")], (16,)), ("gain", "<f4", (16, 120))])
assert CCE_DTYPE.itemsize == 7716
CCE_REFERENCE, CCE_SPEC = 0, 1
CCE_BEFORE_TNS, CCE_AFTER_TNS, CCE_AFTER_IMDCT = 0, 1, 2
TNS_REFERENCE, TNS_SPEC = 0, 1
PIPELINE_STAGE_TNS, PIPELINE_STAGE_PNS = 1, 2        # aacg_pipeline_config.stages
PIPELINE_STAGE_WINDOW_SHAPE = 4                      # ... each channel's window shape carried from frame to frame (aacg_plan_carry_window_shape)
PNS_REFERENCE, PNS_SPEC = 0, 1
UNIT_COMMON_WINDOW, UNIT_MASK_PRESENT, UNIT_HAS_PNS, UNIT_CCE = 1, 2, 4, 8
CHAN_TNS_PRESENT = 0x01


class Config(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("device_ordinal", C.c_int32), ("sample_index", C.c_int32),
                ("max_streams", C.c_int32), ("max_channels", C.c_int32), ("max_batch_units", C.c_int32),
                ("input_kind", C.c_int32), ("tns_mode", C.c_int32), ("pns_mode", C.c_int32), ("output_kind", C.c_int32), ("cce_mode", C.c_int32)]


class PipelineConfig(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("device_ordinal", C.c_int32), ("sample_index", C.c_int32), ("max_streams", C.c_int32),
                ("channels", C.c_int32), ("max_frames", C.c_int32), ("output_kind", C.c_int32), ("parse_options", C.c_int32),
                ("lanes", C.c_int32), ("plan_mode", C.c_int32), ("stages", C.c_int32), ("reserved", C.c_int32 * 1)]


# aacg_pcm_device_out: where aacg_pipeline_submit_device leaves a batch's PCM on the device
PCM_PACKED, PCM_PLANAR = 0, 1                        # AACG_PCM_*: [frame][1024][channels] as the host call's / [stream][channel][stride_frames * 1024]
AACG_PCM_PACKED, AACG_PCM_PLANAR = PCM_PACKED, PCM_PLANAR


class PcmDeviceOut(C.Structure):
    _fields_ = [("d_pcm", C.c_void_p), ("d_pcm_bytes", C.c_size_t), ("layout", C.c_int32), ("stride_frames", C.c_uint32)]


# aacg_features_config: the feature stage's parameters and tables (aacg_pipeline_set_features)
class FeaturesConfig(C.Structure):
    _fields_ = [("frame_length", C.c_uint32), ("hop", C.c_uint32), ("pad_left", C.c_uint32), ("n_rows", C.c_uint32), ("n_mels", C.c_uint32),
                ("log", C.c_uint32), ("floor", C.c_float), ("basis", C.c_void_p), ("fb", C.c_void_p)]


# aacg_loudness_config: the meter's hop and its two biquad sections (aacg_pipeline_set_loudness)
class LoudnessConfig(C.Structure):
    _fields_ = [("hop", C.c_uint32), ("coeffs", (C.c_float * 5) * 2)]


# aacg_limiter_config: the limiter's ceiling (full-scale units) and release (the share of the way back per block of 64 samples)
# aacg_true_peak_config: the oversampling table's shape and the table (aacg_pipeline_set_true_peak)
class TruePeakConfig(C.Structure):
    _fields_ = [("phases", C.c_uint32), ("taps", C.c_uint32), ("table", C.c_void_p)]


class LimiterConfig(C.Structure):
    _fields_ = [("ceiling", C.c_float), ("release", C.c_float)]


# aacg_conceal_config: how a refused frame repeats its stream's last good frame (aacg_pipeline_set_concealment)
class ConcealConfig(C.Structure):
    _fields_ = [("fade_steps", C.c_uint32), ("hold_frames", C.c_uint32)]


CONCEAL_FADE_STEPS, CONCEAL_HOLD_FRAMES = 2, 6       # what conceal=True sets: 3 dB a lost frame, six frames in a row
# aacg_conceal_stream: one stream of a batch as aacg_plan_conceal_refused takes it
CONCEAL_STREAM_DTYPE = np.dtype([(n, "<u4") for n in ("frame_first", "frames", "unit_first", "frame_units", "slot", "nch", "state", "reserved")])


LIMIT_BLOCK = 64                                     # AACG_LIMIT_BLOCK: samples of a limiter block, and its delay


# aacg_trim_config: the window (skip, keep) every slot of a pipeline with a trim starts with (aacg_pipeline_set_trim)
class TrimConfig(C.Structure):
    _fields_ = [("skip", C.c_uint64), ("keep", C.c_uint64)]


TRIM_ALL = 2 ** 64 - 1                               # AACG_TRIM_ALL: a window without an end


# aacg_shape_stream: one stream of a batch in the table a plan made by aacg_plan_create_shaped is shaped from
SHAPE_STREAM_DTYPE = np.dtype([("frame_first", "<u4"), ("frames", "<u4"), ("unit_first", "<u4"), ("frame_units", "<u4"), ("slot", "<u4"),
                               ("run_first", "<u4"), ("link_first", "<u4"), ("rot", "<u4"), ("nch", "<u4"), ("reserved", "<u4", (3,))])
assert SHAPE_STREAM_DTYPE.itemsize == 48


class Batch(C.Structure):
    _fields_ = [("units", C.c_void_p), ("n_units", C.c_uint32), ("coeffs", C.c_void_p), ("n_coef_blocks", C.c_uint32),
                ("meta", C.c_void_p), ("n_meta", C.c_uint32), ("tns", C.c_void_p), ("n_tns", C.c_uint32),
                ("cce", C.c_void_p), ("n_cce", C.c_uint32), ("pcm_out", C.c_void_p), ("n_pcm_floats", C.c_size_t)]


# the sample rates of the format's sampling_frequency_index (sample_index)
SAMPLE_RATES = [96000, 88200, 64000, 48000, 44100, 32000, 24000, 22050, 16000, 12000, 11025, 8000, 7350]


class AacgError(RuntimeError):
    def __init__(self, code, msg):
        RuntimeError.__init__(self, "aacgpu: %s (%d): %s" % (ERR_NAMES.get(code, "?"), code, msg))
        self.code = code


_lib = None


def _share_hip_runtime_with_torch():
    """PyTorch wheels bundle their own libamdhip64.so.7.  One process must use ONE HIP runtime, or device
    pointers from torch are foreign to this library: if torch is installed (bench/tests use it for device
    memory and streams) map its runtime first, so that libaacgpu.so's NEEDED libamdhip64.so.7 resolves to
    the same copy whether torch is imported before or after.  Without torch the system ROCm runtime is used."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def load_library(path=LIB_PATH):
    """dlopen the C-ABI library.  Raises if it has not been built — never falls back."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise RuntimeError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(hipcc --offload-arch=gfx950); there is no CPU fallback" % path)
    _share_hip_runtime_with_torch()
    L = C.CDLL(path)
    L.aacg_abi_version.restype = C.c_int
    L.aacg_kernel_name.restype = C.c_char_p
    L.aacg_plan_kernels.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
    L.aacg_plan_kernels_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_char_p, C.c_size_t]
    L.aacg_decode_pipelined.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.aacg_decode_pipelined_timed.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.aacg_pipeline_fork.argtypes = [C.c_void_p, C.c_void_p]
    L.aacg_pipeline_join.argtypes = [C.c_void_p, C.c_void_p]
    L.aacg_pipeline_chained.argtypes = [C.c_void_p]
    L.aacg_pipeline_chained.restype = C.c_uint64
    L.aacg_pipeline_concurrent.argtypes = [C.c_void_p]
    L.aacg_pipeline_streams_used.argtypes = [C.c_void_p]
    L.aacg_debug_route.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_size_t]
    L.aacg_debug_run_kernel.argtypes = [C.c_int, C.c_char_p, C.c_size_t]
    L.aacg_plan_refresh_units.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    L.aacg_calib_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.aacg_timer_create.argtypes = [C.POINTER(C.c_void_p)]
    L.aacg_timer_record.argtypes = [C.c_void_p, C.c_void_p]
    L.aacg_timer_elapsed_ms.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
    L.aacg_timer_destroy.argtypes = [C.c_void_p]
    L.aacg_timer_destroy.restype = None
    L.aacg_debug_set_route.argtypes = [C.c_void_p, C.c_int]
    L.aacg_last_error.restype = C.c_char_p
    L.aacg_last_error.argtypes = [C.c_void_p]
    L.aacg_create.argtypes = [C.POINTER(Config), C.POINTER(C.c_void_p)]
    L.aacg_destroy.argtypes = [C.c_void_p]
    L.aacg_destroy.restype = None
    L.aacg_reset_stream.argtypes = [C.c_void_p, C.c_uint32]
    L.aacg_get_overlap.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    L.aacg_set_overlap.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    L.aacg_get_window_shape.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint8)]
    L.aacg_set_window_shape.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint8]
    L.aacg_plan_carry_window_shape.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    L.aacg_pipeline_stream_window_shape.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    L.aacg_decode_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                    C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t]
    L.aacg_submit.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                              C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)]
    L.aacg_decode_batch_tns.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                        C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t]
    L.aacg_submit_tns.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                  C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t,
                                  C.POINTER(C.c_uint64)]
    L.aacg_plan_create_tns.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]
    L.aacg_wait.argtypes = [C.c_void_p, C.c_uint64]
    L.aacg_host_alloc.restype = C.c_void_p
    L.aacg_host_alloc.argtypes = [C.c_size_t]
    L.aacg_host_free.restype = None
    L.aacg_host_free.argtypes = [C.c_void_p]
    L.aacg_plan_create.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]
    L.aacg_plan_destroy.argtypes = [C.c_void_p]
    L.aacg_plan_destroy.restype = None
    L.aacg_decode_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.aacg_spectral_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.aacg_synchronize.argtypes = [C.c_void_p, C.c_void_p]
    L.aacg_get_table.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    L.aacg_parser_create.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
    L.aacg_parser_destroy.argtypes = [C.c_void_p]
    L.aacg_parser_destroy.restype = None
    L.aacg_parser_last_error.argtypes = [C.c_void_p]
    L.aacg_parser_last_error.restype = C.c_char_p
    L.aacg_parse_status_string.argtypes = [C.c_int]
    L.aacg_parse_status_string.restype = C.c_char_p
    L.aacg_parse_kernel_name.restype = C.c_char_p
    L.aacg_parse_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.aacg_plan_refresh_from_parse.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    L.aacg_parse_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.aacg_standard_codebooks.argtypes = [C.c_void_p, C.c_void_p]
    L.aacg_parse_walk.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    L.aacg_parse_walk_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.aacg_decode_batch_ex.argtypes = [C.c_void_p, C.POINTER(Batch)]
    L.aacg_submit_ex.argtypes = [C.c_void_p, C.POINTER(Batch), C.POINTER(C.c_uint64)]
    L.aacg_plan_create_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]
    L.aacg_debug_transform.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.aacg_standard_codebooks.restype = C.c_uint32
    L.aacg_set_wait_limit_ms.argtypes = [C.c_void_p, C.c_uint32]
    L.aacg_parser_set_wait_limit_ms.argtypes = [C.c_void_p, C.c_uint32]
    L.aacg_pipeline_info.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.aacg_debug_set_wait_mode.argtypes = [C.c_void_p, C.c_int, C.c_double]
    L.aacg_debug_in_flight.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    L.aacg_plan_set_unit_sets.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    L.aacg_plan_refresh_from_parse_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    L.aacg_plan_create_stages.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]
    L.aacg_decode_pipelined_stages.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    L.aacg_tns_records_bytes.restype = C.c_size_t
    L.aacg_tns_records_bytes.argtypes = [C.c_uint32]
    L.aacg_tns_records_from_parse.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    L.aacg_pipeline_create.argtypes = [C.POINTER(PipelineConfig), C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
    L.aacg_pipeline_destroy.argtypes = [C.c_void_p]
    L.aacg_pipeline_destroy.restype = None
    L.aacg_pipeline_last_error.argtypes = [C.c_void_p]
    L.aacg_pipeline_last_error.restype = C.c_char_p
    L.aacg_pipeline_reset_stream.argtypes = [C.c_void_p, C.c_uint32]
    L.aacg_pipeline_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.aacg_pipeline_submit.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
    L.aacg_pipeline_collect.argtypes = [C.c_void_p, C.c_uint64]
    L.aacg_pipeline_decode_ragged.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.aacg_pipeline_submit_ragged.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.POINTER(C.c_uint64)]
    L.aacg_pipeline_submit_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(PcmDeviceOut), C.c_void_p,
                                              C.c_void_p, C.POINTER(C.c_uint64)]
    L.aacg_pipeline_wait_device.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    L.aacg_pipeline_plan_builds.argtypes = [C.c_void_p]
    L.aacg_pipeline_plan_builds.restype = C.c_uint64
    L.aacg_pipeline_launch_counts.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.aacg_plan_create_shaped.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
    L.aacg_plan_create_shaped_stages.argtypes = L.aacg_plan_create_shaped.argtypes
    L.aacg_plan_shape_table.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
    L.aacg_plan_shape_launch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    L.aacg_pipeline_set_wait_limit_ms.argtypes = [C.c_void_p, C.c_uint32]
    L.aacg_pipeline_stream_layout.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32)]
    L.aacg_pipeline_set_mix.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    L.aacg_pipeline_out_channels.argtypes = [C.c_void_p]
    L.aacg_mix_standard.argtypes = [C.c_uint32, C.c_uint32, C.c_float, C.c_int, C.c_void_p]
    L.aacg_pipeline_set_resample.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    L.aacg_pipeline_out_samples.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    L.aacg_resample_counts.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    L.aacg_resample_design.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.aacg_pipeline_set_features.argtypes = [C.c_void_p, C.POINTER(FeaturesConfig)]
    L.aacg_features_counts.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p]
    L.aacg_features_design.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.c_double, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    L.aacg_pipeline_set_loudness.argtypes = [C.c_void_p, C.POINTER(LoudnessConfig)]
    L.aacg_pipeline_loudness_out.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.aacg_pipeline_loudness_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    L.aacg_loudness_counts.argtypes = [C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p]
    L.aacg_loudness_design.argtypes = [C.c_uint32, C.c_void_p]
    L.aacg_loudness_integrate.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.aacg_pipeline_set_limiter.argtypes = [C.c_void_p, C.POINTER(LimiterConfig)]
    L.aacg_pipeline_set_gain.argtypes = [C.c_void_p, C.c_uint32, C.c_float]
    L.aacg_pipeline_gain.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_float)]
    L.aacg_pipeline_set_concealment.argtypes = [C.c_void_p, C.POINTER(ConcealConfig)]
    L.aacg_pipeline_concealed.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.aacg_conceal_state_bytes.argtypes = [C.c_uint32, C.c_uint32]
    L.aacg_conceal_state_bytes.restype = C.c_size_t
    L.aacg_plan_conceal_refused.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32,
                                            C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    L.aacg_limiter_design.argtypes = [C.c_uint32, C.c_double, C.c_double, C.POINTER(LimiterConfig)]
    L.aacg_pipeline_set_true_peak.argtypes = [C.c_void_p, C.POINTER(TruePeakConfig)]
    L.aacg_pipeline_true_peak_out.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.aacg_true_peak_design.argtypes = [C.c_uint32, C.c_uint32, C.c_double, C.c_double, C.c_void_p, C.c_size_t]
    L.aacg_pipeline_set_trim.argtypes = [C.c_void_p, C.POINTER(TrimConfig)]
    L.aacg_pipeline_set_stream_trim.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64]
    L.aacg_pipeline_stream_trim.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.aacg_trim_counts.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    L.aacg_trim_design.argtypes = [C.c_uint64, C.c_uint64, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32] + [C.POINTER(C.c_uint64)] * 4
    L.aacg_trim_design_delay.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32] + [C.POINTER(C.c_uint64)] * 4
    L.aacg_pipeline_set_limiter_true_peak.argtypes = [C.c_void_p, C.POINTER(TruePeakConfig)]
    L.aacg_pipeline_limiter_delay.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    _lib = L
    return L


# ---- device front end (aacg_parser_*, include/aacgpu.h) -------------------------------------------------
CODE_ENTRY_DTYPE = np.dtype([("code", "<u4"), ("len", "u1"), ("v", "i1", (4,)), ("reserved", "u1", (3,))])
PARSE_FRAME_DTYPE = np.dtype([("byte_offset", "<u4"), ("byte_length", "<u4")])
PARSE_RESULT_DTYPE = np.dtype([("status", "u1"), ("n_units", "u1"), ("n_channels", "u1"), ("flags", "u1"), ("bits_used", "<u4")])
WALK_RESULT_DTYPE = np.dtype([("n_frames", "<u4"), ("status", "<u4"), ("bytes_consumed", "<u4"), ("reserved", "<u4")])
META_DTYPE = np.dtype(("<u2", (120,)))
PARSE_APPLY_PULSES, PARSE_REFERENCE_QUIRKS, PARSE_SKIP_ZERO_FILL = 1, 2, 4


def debug_transform(x, is_short=False, identity_rotation=False, sample_index=3, device=0, vm=False):
    """aacg_debug_transform: the kernels' IMDCT stage on one spectrum (1024 floats), windows forced to 1; returns 2048 floats.
    vm: the int16 seam's variant of the stage (mirror-lane exchanges as DPP, long columns dealt out by long_col)."""
    L = load_library()
    x = np.ascontiguousarray(x, np.float32)
    assert x.size == 1024
    out = np.zeros(2048, np.float32)
    rc = L.aacg_debug_transform(device, sample_index, int(bool(is_short)) | (2 if vm else 0), int(identity_rotation), x.ctypes.data, out.ctypes.data)
    if rc:
        raise AacgError(rc, "aacg_debug_transform failed")
    return out



class TimerMark:
    """aacg_timer_*: a HIP event that only measures time (hipEventDisableSystemFence), recorded on a given stream.
    `a.elapsed_ms(b)` after the stream has been synchronised."""
    def __init__(self):
        self.h = C.c_void_p()
        rc = load_library().aacg_timer_create(C.byref(self.h))
        if rc:
            raise AacgError(rc, "aacg_timer_create failed")

    def record(self, stream):
        rc = load_library().aacg_timer_record(self.h, stream)
        if rc:
            raise AacgError(rc, "aacg_timer_record failed")

    def elapsed_ms(self, later):
        ms = C.c_float()
        rc = load_library().aacg_timer_elapsed_ms(self.h, later.h, C.byref(ms))
        if rc:
            raise AacgError(rc, "aacg_timer_elapsed_ms failed (stream not synchronised?)")
        return float(ms.value)

    def __del__(self):
        try:
            if self.h:
                load_library().aacg_timer_destroy(self.h)
                self.h = C.c_void_p()
        except Exception:
            pass

def debug_route(input_kind, output_kind, plan_flags, pipelined=False, debug_flags=0):
    """aacg_debug_route: the launches (kernel names, ' + ' between them) the engine's ONE route decision makes for a planned batch
    with these flags (ROUTE_PLAN_*) on an engine of these kinds.  No device needed."""
    buf = C.create_string_buffer(512)
    rc = load_library().aacg_debug_route(input_kind, output_kind, debug_flags, plan_flags, 1 if pipelined else 0, buf, 512)
    if rc:
        raise AacgError(rc, "aacg_debug_route: no registered kernel for this route")
    return buf.value.decode()


def run_kernels():
    """The registered run kernels as {symbol: switches} (aacg_debug_run_kernel)."""
    out, i = {}, 0
    buf = C.create_string_buffer(128)
    while True:
        key = load_library().aacg_debug_run_kernel(i, buf, 128)
        if key < 0:
            return out
        out[buf.value.decode()] = key
        i += 1


PIPE_STREAMS = 3        # AACG_PIPE_STREAMS: launches of a pipelined sequence that may be in flight side by side (aacg_device.h)


def pipeline_order(n, streams=PIPE_STREAMS):
    """How launch n of a pipelined sequence on `streams` streams is ordered (aacg_pipeline_order, aacg_routes.cpp): (stream, the round whose completion
    events the host waits for before enqueuing it or -1, whether its own completion gets an event, the launch up to which
    everything is known complete when it is enqueued or -1, number of rotating overlap buffers the rule has to cover)."""
    lib = load_library()
    lib.aacg_debug_pipeline_order.argtypes = [C.c_ulonglong, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_longlong), C.POINTER(C.c_int), C.POINTER(C.c_longlong)]
    st, w, m, u = C.c_int(), C.c_longlong(), C.c_int(), C.c_longlong()
    k = lib.aacg_debug_pipeline_order(n, streams, C.byref(st), C.byref(w), C.byref(m), C.byref(u))
    return st.value, w.value, bool(m.value), u.value, k


def calib_copy(d_dst, d_src, n_bytes, stream=0):
    """aacg_calib_copy: float4 device-to-device copy with the run kernels' launch shape, enqueued on `stream`."""
    rc = load_library().aacg_calib_copy(d_dst, d_src, n_bytes, stream)
    if rc:
        raise AacgError(rc, "aacg_calib_copy failed")


def standard_codebooks():
    """The 12 codebooks of ISO/IEC 14496-3 as (entries, counts), from the library (aacg_standard_codebooks)."""
    L = load_library()
    entries, counts = np.zeros(L.aacg_standard_codebooks(None, None), CODE_ENTRY_DTYPE), np.zeros(12, np.uint32)
    L.aacg_standard_codebooks(entries.ctypes.data, counts.ctypes.data)
    return entries, counts


def alloc_parse_outputs(n_frames, max_units, max_channels, want_tns):
    blocks = n_frames * max_channels
    return {"units": np.zeros(n_frames * max_units, UNIT_DTYPE), "q": np.zeros((blocks, 1024), np.int16),
            "meta": np.zeros((blocks, 120), np.uint16), "tns": np.zeros(blocks, TNS_DTYPE) if want_tns else None,
            "results": np.zeros(n_frames, PARSE_RESULT_DTYPE)}


class Parser:
    """aacg_parser: one GPU lane parses one frame.  entries / counts: the 12 codebooks as CODE_ENTRY_DTYPE records."""

    def __init__(self, entries=None, counts=None, sample_index=3, device=0):
        self.lib = load_library()
        if entries is None:
            entries, counts = standard_codebooks()
        entries = np.ascontiguousarray(entries)
        counts = np.ascontiguousarray(counts, np.uint32)
        assert entries.dtype == CODE_ENTRY_DTYPE and counts.size == 12
        h = C.c_void_p()
        rc = self.lib.aacg_parser_create(device, sample_index, entries.ctypes.data, counts.ctypes.data, C.byref(h))
        self.handle = h
        if rc != 0:
            msg = self.lib.aacg_parser_last_error(h).decode() if h else "aacg_parser_create failed"
            self.close()
            raise AacgError(rc, msg)

    def close(self):
        if getattr(self, "handle", None):
            self.lib.aacg_parser_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise AacgError(rc, self.lib.aacg_parser_last_error(self.handle).decode())

    def parse_batch(self, data, frames, max_units, max_channels, options=PARSE_REFERENCE_QUIRKS, want_tns=False):
        data = np.ascontiguousarray(data, np.uint8)
        frames = np.ascontiguousarray(frames)
        assert frames.dtype == PARSE_FRAME_DTYPE
        out = alloc_parse_outputs(len(frames), max_units, max_channels, want_tns)
        self._check(self.lib.aacg_parse_batch(self.handle, data.ctypes.data, data.size, frames.ctypes.data, len(frames), max_units, max_channels,
                                              options, out["units"].ctypes.data, out["q"].ctypes.data, out["meta"].ctypes.data,
                                              out["tns"].ctypes.data if want_tns else None, out["results"].ctypes.data))
        return out

    def parse_device(self, d_bytes, d_frames, n_frames, max_units, max_channels, options, d_units, d_q, d_meta, d_tns, d_results, stream=0):
        """Device pointers (ints); asynchronous on `stream`."""
        self._check(self.lib.aacg_parse_device(self.handle, d_bytes, d_frames, n_frames, max_units, max_channels, options,
                                               d_units, d_q, d_meta, d_tns, d_results, stream))

    def walk(self, data, spans, max_frames, options=PARSE_REFERENCE_QUIRKS):
        """aacg_parse_walk: where the raw_data_blocks of each span lie.  spans: PARSE_FRAME_DTYPE byte ranges in `data`, each
        starting at a block boundary.  Returns (frames [n_spans][max_frames] PARSE_FRAME_DTYPE, zero beyond a span's count;
        results [n_spans] WALK_RESULT_DTYPE)."""
        data = np.ascontiguousarray(data, np.uint8)
        spans = np.ascontiguousarray(spans)
        assert spans.dtype == PARSE_FRAME_DTYPE
        frames = np.zeros((len(spans), max_frames), PARSE_FRAME_DTYPE)
        results = np.zeros(len(spans), WALK_RESULT_DTYPE)
        self._check(self.lib.aacg_parse_walk(self.handle, data.ctypes.data, data.size, spans.ctypes.data, len(spans), max_frames,
                                             options, frames.ctypes.data, results.ctypes.data))
        return frames, results

    def walk_device(self, d_bytes, d_spans, n_spans, max_frames, options, d_frames, d_results, stream=0):
        """Device pointers (ints); asynchronous on `stream`."""
        self._check(self.lib.aacg_parse_walk_device(self.handle, d_bytes, d_spans, n_spans, max_frames, options, d_frames, d_results, stream))

    def status_string(self, status):
        return self.lib.aacg_parse_status_string(int(status)).decode()


REFRESH_MAP_DTYPE = np.dtype([("parsed_index", "<u4"), ("frame_units", "<u4")])
PARSE_LAYOUT = 16          # AACG_PARSE_LAYOUT: a frame whose elements are not its stream's
PARSE_CONCEALED = 0x8      # AACG_PARSE_CONCEALED in aacg_parse_result.flags: a refused frame that repeats its stream's last good frame, faded


class Pipeline:
    """aacg_pipeline: bytes in, PCM out — device front end and transform behind one call per batch, `lanes` batches in flight
    (include/aacgpu.h).  channels = the streams' chanConfig (1..8).  device_plans: ONE plan shaped on the device for every batch
    (aacg_pipeline_config.plan_mode 1) instead of a kept plan per batch shape: for feeds whose batches seldom repeat a shape.
    mix: an (O, C) float matrix, O = 1 or 2 (aacg_pipeline_set_mix; mix_standard makes the usual one): the PCM is mixed on the device and
    O channels leave — self.channels is then O wherever PCM is sized, self.in_channels stays C.
    resample: (L, M, table) with table an (L, taps) float matrix (aacg_pipeline_set_resample; resample_design makes the usual one), or
    out_rate: a sample rate, for which the default table is designed from the rate of sample_index.  The PCM then leaves at L / M times
    the streams' rate, a ragged count of samples per stream: decode and collect return (pcm, results, n_refused, lengths) with pcm flat,
    stream after stream, lengths[s] samples of self.channels each; decode_tensor's lengths are those counts.  self.rate is the PCM's.
    features: a dict for set_features (aacg_pipeline_set_features; features_design makes the usual tables) — frame_length, hop, basis
    (2 x bins, frame_length), fb (n_mels, bins) and optionally pad_left, log, floor.  The last stage of the way out: float32 feature
    frames leave in the place of one channel of PCM, ragged like a resampler's samples: decode and collect return (frames, results,
    n_refused, lengths) with frames flat, lengths[s] feature frames of n_mels floats each; decode_tensor returns (S, n_mels, T).
    loudness: a dict for set_loudness (aacg_pipeline_set_loudness; loudness_design makes BS.1770's) — hop and coeffs (2, 5).  A tap on the
    transform's PCM, beside whatever else leaves: decode, submit, collect and decode_tensor return what they return without it, and
    take_loudness gives a batch's records, a list of (n_out[s], in_channels, 2) float32 arrays of {energy, sample peak} per hop.
    limiter: a LimiterConfig or a (ceiling, release) pair for set_limiter (aacg_pipeline_set_limiter; limiter_design makes one from dB and
    milliseconds).  A stage behind the mix and in front of the resampler: every stream's PCM is scaled by its slot's gain (set_gain, 1
    until set) and held below the ceiling, all channels alike, delayed by 64 samples; shapes and counts are what they are without it.
    limiter_true_peak: True (true_peak_design()'s table), or a (phases, taps, table) triple, for set_limiter_true_peak
    (aacg_pipeline_set_limiter_true_peak), with limiter: the ceiling holds for the oversampled signal too, and the delay is limiter_delay().
    true_peak: a dict for set_true_peak (aacg_pipeline_set_true_peak; true_peak_design makes the usual table) — phases, taps and table
    (phases, taps) —, on a pipeline with loudness: the oversampled peak of every hop of the meter, beside its records;
    take_true_peak gives a batch's, a list of (n_out[s], in_channels) float32 arrays.  Every other call returns what it returns without it.
    conceal: True, or a dict(fade_steps=, hold_frames=), for set_concealment (aacg_pipeline_set_concealment), with device_plans: a frame
    the parser or the refresh refuses repeats its stream's last good frame, fading, instead of going silent; its result keeps its status
    and gains PARSE_CONCEALED in `flags`.  concealed() counts such frames of collected batches.
    trim: True, or a (skip, keep) pair (keep None: no end), for set_pipeline_trim (aacg_pipeline_set_trim): the last PCM stage, behind the
    resampler and in front of the feature stage.  Each slot has a window in samples of what the stage receives (set_trim, stream_trim;
    trim_design converts a window in the stream's own samples and compensates the limiter's and the resampler's delays), and only the
    kept samples leave, a ragged count per stream: decode, collect and decode_tensor return lengths as for a resampled pipeline."""

    def __init__(self, channels=2, max_streams=1, max_frames=16, sample_index=3, device=0, output_kind=OUTPUT_F32,
                 parse_options=PARSE_REFERENCE_QUIRKS, lanes=0, entries=None, counts=None, device_plans=False, tns_spec=False, pns_spec=False,
                 carry_window_shape=False, mix=None, resample=None, out_rate=None, resample_taps=32, features=None, loudness=None, limiter=None, true_peak=None,
                 conceal=None, trim=None, limiter_true_peak=None):
        self.lib = load_library()
        if entries is None:
            entries, counts = standard_codebooks()
        entries, counts = np.ascontiguousarray(entries), np.ascontiguousarray(counts, np.uint32)
        cfg = PipelineConfig(self.lib.aacg_abi_version(), device, sample_index, max_streams, channels, max_frames, output_kind, parse_options, lanes,
                             1 if device_plans else 0, (PIPELINE_STAGE_TNS if tns_spec else 0) | (PIPELINE_STAGE_PNS if pns_spec else 0) |
                             (PIPELINE_STAGE_WINDOW_SHAPE if carry_window_shape else 0))
        h = C.c_void_p()
        rc = self.lib.aacg_pipeline_create(C.byref(cfg), entries.ctypes.data, counts.ctypes.data, C.byref(h))
        if rc != 0:
            raise AacgError(rc, "aacg_pipeline_create failed (no GPU?%s)" % (" or no room for the device plan's buffers: see stderr" if device_plans else ""))
        self.device_plans = bool(device_plans)
        self.handle, self.channels, self.i16, self.device = h, channels, output_kind == OUTPUT_I16, device
        self.in_channels = channels
        self.resample, self.rate = None, SAMPLE_RATES[sample_index]
        self.features = None
        self.loudness, self._loud, self._loud_last = None, {}, None
        self.limiter = self.limiter_true_peak = None
        self.true_peak, self._tp, self._tp_last, self._tp_armed = None, {}, None, None
        self._keep = {}
        self.conceal = None
        self.trim = None
        if conceal is not None and conceal is not False:
            try:
                self.set_concealment(**({} if conceal is True else dict(conceal)))
            except (AacgError, ValueError, TypeError):
                self.close()
                raise
        if mix is not None:
            m = np.ascontiguousarray(mix, np.float32)
            if m.ndim != 2 or m.shape[1] != channels:
                self.close()
                raise ValueError("Pipeline: mix is not an (O, %d) matrix" % channels)
            try:
                self.set_mix(m)
            except AacgError:
                self.close()
                raise
        if limiter is not None:
            try:
                self.set_limiter(limiter)
            except (AacgError, ValueError, TypeError):
                self.close()
                raise
        if limiter_true_peak is not None and limiter_true_peak is not False:
            try:
                d = true_peak_design() if limiter_true_peak is True else None
                self.set_limiter_true_peak(*((d["phases"], d["taps"], d["table"]) if d else limiter_true_peak))
            except (AacgError, ValueError, TypeError):
                self.close()
                raise
        if out_rate is not None and resample is None:
            try:
                resample = resample_design(self.rate, int(out_rate), resample_taps)
            except AacgError:
                self.close()
                raise
        if resample is not None:
            try:
                self.set_resample(*resample)
            except (AacgError, ValueError):
                self.close()
                raise
        if trim is not None and trim is not False:
            try:
                self.set_pipeline_trim(*((0, None) if trim is True else trim))
            except (AacgError, ValueError, TypeError):
                self.close()
                raise
        if features is not None:
            try:
                self.set_features(**features)
            except (AacgError, ValueError, TypeError):
                self.close()
                raise
        if loudness is not None:
            try:
                self.set_loudness(**loudness)
            except (AacgError, ValueError, TypeError):
                self.close()
                raise
        if true_peak is not None:
            try:
                self.set_true_peak(**true_peak)
            except (AacgError, ValueError, TypeError):
                self.close()
                raise

    def close(self):
        if getattr(self, "handle", None):
            self.lib.aacg_pipeline_destroy(self.handle)
            self.handle = None
            for p in getattr(self, "_pinned", []):
                self.lib.aacg_host_free(p)
            self._pinned = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise AacgError(rc, self.lib.aacg_pipeline_last_error(self.handle).decode())

    def pinned(self, shape, dtype):
        """numpy array over page-locked host memory (aacg_host_alloc): the PCM comes straight down from the device into it."""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = self.lib.aacg_host_alloc(n)
        if not p:
            raise AacgError(-3, "aacg_host_alloc failed")
        self._pinned = getattr(self, "_pinned", [])
        self._pinned.append(p)
        return np.frombuffer((C.c_char * n).from_address(p), dtype=dtype).reshape(shape)

    def set_wait_limit_ms(self, ms):
        self._check(self.lib.aacg_pipeline_set_wait_limit_ms(self.handle, int(ms)))

    def reset_stream(self, slot):
        self._check(self.lib.aacg_pipeline_reset_stream(self.handle, slot))

    def set_mix(self, matrix):
        """aacg_pipeline_set_mix: an (O, C) float matrix, O = 1 or 2, before the first batch; from then on O channels leave."""
        m = np.ascontiguousarray(matrix, np.float32)
        assert m.ndim == 2 and m.shape[1] == self.in_channels
        self._check(self.lib.aacg_pipeline_set_mix(self.handle, m.shape[0], m.ctypes.data))
        self.channels = int(self.lib.aacg_pipeline_out_channels(self.handle))

    def set_resample(self, L, M, table):
        """aacg_pipeline_set_resample: the (L, taps) table of an L / M resampler, before the first batch and after the mix."""
        h = np.ascontiguousarray(table, np.float32)
        if h.ndim != 2 or h.shape[0] != int(L):
            raise ValueError("Pipeline: the resampler's table is not an (L, taps) matrix")
        self._check(self.lib.aacg_pipeline_set_resample(self.handle, int(L), int(M), h.shape[1], h.ctypes.data))
        self.resample = (int(L), int(M), h)
        self.rate = self.rate * int(L) / int(M)

    def set_features(self, frame_length, hop, basis, fb, pad_left=0, log=True, floor=1e-10):
        """aacg_pipeline_set_features: basis (2 x bins, frame_length) and fb (n_mels, bins) float matrices, before the first batch and
        after the mix and the resampler; from then on feature frames of n_mels float32 leave instead of PCM."""
        basis, fb = np.ascontiguousarray(basis, np.float32), np.ascontiguousarray(fb, np.float32)
        if basis.ndim != 2 or fb.ndim != 2 or basis.shape[1] != int(frame_length) or basis.shape[0] != 2 * fb.shape[1]:
            raise ValueError("Pipeline: the feature stage's tables are not (2 x bins, frame_length) and (n_mels, bins) matrices")
        cfg = FeaturesConfig(int(frame_length), int(hop), int(pad_left), basis.shape[0], fb.shape[0], 1 if log else 0, float(floor), basis.ctypes.data, fb.ctypes.data)
        self._check(self.lib.aacg_pipeline_set_features(self.handle, C.byref(cfg)))
        self.features = {"frame_length": int(frame_length), "hop": int(hop), "pad_left": int(pad_left), "n_mels": int(fb.shape[0]), "log": bool(log),
                         "floor": float(np.float32(floor)), "basis": basis, "fb": fb}

    def set_loudness(self, hop, coeffs):
        """aacg_pipeline_set_loudness: a meter of `hop` samples with the two biquad sections coeffs (2, 5), before the first batch"""
        k = np.ascontiguousarray(coeffs, np.float32)
        if k.shape != (2, 5):
            raise ValueError("Pipeline: the meter's coefficients are not a (2, 5) matrix")
        cfg = LoudnessConfig(int(hop))
        C.memmove(cfg.coeffs, k.ctypes.data, 40)
        self._check(self.lib.aacg_pipeline_set_loudness(self.handle, C.byref(cfg)))
        self.loudness = {"hop": int(hop), "coeffs": k}

    def set_limiter(self, config):
        """aacg_pipeline_set_limiter: a LimiterConfig or a (ceiling, release) pair, before the first batch and after the mix"""
        cfg = config if isinstance(config, LimiterConfig) else LimiterConfig(*[float(v) for v in config])
        self._check(self.lib.aacg_pipeline_set_limiter(self.handle, C.byref(cfg)))
        self.limiter = LimiterConfig(cfg.ceiling, cfg.release)

    def set_limiter_true_peak(self, phases, taps, table):
        """aacg_pipeline_set_limiter_true_peak: a true-peak detector with the polyphase table (phases, taps) in front of the limiter's
        recurrence, on a pipeline with a limiter, before the first batch and the trim"""
        h = np.ascontiguousarray(table, np.float32)
        if h.shape != (int(phases), int(taps)):
            raise ValueError("Pipeline: the limiter's true-peak table is not a (phases, taps) matrix")
        cfg = TruePeakConfig(int(phases), int(taps), h.ctypes.data)
        self._check(self.lib.aacg_pipeline_set_limiter_true_peak(self.handle, C.byref(cfg)))
        self.limiter_true_peak = {"phases": int(phases), "taps": int(taps), "table": h}

    def limiter_delay(self):
        """aacg_pipeline_limiter_delay: the limiter's delay in samples, 64, or 64 + taps / 2 with the true-peak detector"""
        n = C.c_uint32()
        rc = self.lib.aacg_pipeline_limiter_delay(self.handle, C.byref(n))
        if rc != 0:
            raise AacgError(rc, "aacg_pipeline_limiter_delay: the pipeline has no limiter")
        return int(n.value)

    def set_concealment(self, fade_steps=CONCEAL_FADE_STEPS, hold_frames=CONCEAL_HOLD_FRAMES):
        """aacg_pipeline_set_concealment: refused frames repeat the stream's last good frame, fade_steps scalefactor steps (1.5 dB) down
        per lost frame, for at most hold_frames frames in a row; before the first batch, on a pipeline with device_plans"""
        if int(fade_steps) < 0 or int(hold_frames) < 0:
            raise ValueError("Pipeline: fade_steps and hold_frames are not negative")
        cfg = ConcealConfig(int(fade_steps), int(hold_frames))
        self._check(self.lib.aacg_pipeline_set_concealment(self.handle, C.byref(cfg)))
        self.conceal = {"fade_steps": int(fade_steps), "hold_frames": int(hold_frames)}

    def concealed(self):
        """aacg_pipeline_concealed: the frames concealed so far in batches that have been collected"""
        n = C.c_uint64()
        rc = self.lib.aacg_pipeline_concealed(self.handle, C.byref(n))
        if rc != 0:
            raise AacgError(rc, "aacg_pipeline_concealed")
        return int(n.value)

    def set_pipeline_trim(self, skip=0, keep=None):
        """aacg_pipeline_set_trim: the stage, with the window (skip, keep) every slot starts with (keep None: no end); before the first
        batch and after the mix, the limiter and the resampler"""
        cfg = TrimConfig(int(skip), TRIM_ALL if keep is None else int(keep))
        self._check(self.lib.aacg_pipeline_set_trim(self.handle, C.byref(cfg)))
        self.trim = (int(skip), None if keep is None else int(keep))

    def set_trim(self, slot, skip, keep=None):
        """aacg_pipeline_set_stream_trim: the slot's window (keep None: no end) and position 0, from the next batch enqueued that holds
        the slot; a reset leaves the window and restarts the position"""
        self._check(self.lib.aacg_pipeline_set_stream_trim(self.handle, int(slot), int(skip), TRIM_ALL if keep is None else int(keep)))

    def stream_trim(self, slot):
        """aacg_pipeline_stream_trim: (skip, keep, position) of the slot as they stand, keep None: no end"""
        s, k, q = C.c_uint64(), C.c_uint64(), C.c_uint64()
        rc = self.lib.aacg_pipeline_stream_trim(self.handle, int(slot), C.byref(s), C.byref(k), C.byref(q))
        if rc != 0:
            raise AacgError(rc, "aacg_pipeline_stream_trim(slot %d): no trim, or no such slot" % int(slot))
        return int(s.value), None if k.value == TRIM_ALL else int(k.value), int(q.value)

    def set_gain(self, slot, gain):
        """aacg_pipeline_set_gain: the slot's gain (0..1024) from the next batch enqueued that holds the slot; a reset leaves it"""
        self._check(self.lib.aacg_pipeline_set_gain(self.handle, int(slot), float(gain)))

    def gain(self, slot):
        """aacg_pipeline_gain: the slot's gain as it stands"""
        g = C.c_float()
        rc = self.lib.aacg_pipeline_gain(self.handle, int(slot), C.byref(g))
        if rc != 0:
            raise AacgError(rc, "aacg_pipeline_gain(slot %d): no limiter, or no such slot" % int(slot))
        return float(g.value)

    def set_true_peak(self, phases, taps, table):
        """aacg_pipeline_set_true_peak: the oversampled peak per hop of the meter with the polyphase table (phases, taps), on a pipeline
        with a meter, before the first batch"""
        h = np.ascontiguousarray(table, np.float32)
        if h.shape != (int(phases), int(taps)):
            raise ValueError("Pipeline: the true-peak table is not a (phases, taps) matrix")
        cfg = TruePeakConfig(int(phases), int(taps), h.ctypes.data)
        self._check(self.lib.aacg_pipeline_set_true_peak(self.handle, C.byref(cfg)))
        self.true_peak = {"phases": int(phases), "taps": int(taps), "table": h}

    def loudness_counts(self, slots, frames_per_stream):
        """aacg_pipeline_loudness_counts: the records per channel that the NEXT batch of these slots with these counts emits, per stream"""
        slots = np.ascontiguousarray(slots, np.uint32)
        counts = np.ascontiguousarray(frames_per_stream, np.uint32) if np.ndim(frames_per_stream) else np.full(len(slots), int(frames_per_stream), np.uint32)
        assert len(counts) == len(slots)
        n = np.zeros(len(slots), np.uint32)
        self._check(self.lib.aacg_pipeline_loudness_counts(self.handle, slots.ctypes.data, counts.ctypes.data, len(slots), n.ctypes.data))
        return n

    def _arm_loudness(self, slots, frames_per_stream):
        """a metered pipeline: buffers of the wrapper's own for the next submission's records, named to the library; else None"""
        if not self.loudness:
            return None
        n = self.loudness_counts(slots, frames_per_stream)
        rec = np.zeros(int(n.sum()) * self.in_channels * 2, np.float32)
        self._check(self.lib.aacg_pipeline_loudness_out(self.handle, rec.ctypes.data, rec.size, n.ctypes.data))
        self._tp_armed = None
        if self.true_peak:                               # ... and for its true-peak floats, a float where the meter has two
            tp = np.zeros(int(n.sum()) * self.in_channels, np.float32)
            self._check(self.lib.aacg_pipeline_true_peak_out(self.handle, tp.ctypes.data, tp.size))
            self._tp_armed = (tp, n)
        return rec, n

    def take_loudness(self, ticket=None):
        """The meter's records of a batch: a list with one (n_out[s], in_channels, 2) float32 array per stream, [..., 0] the hop's
        energy and [..., 1] its sample peak.  ticket: a submitted batch's, which is finished first if it is still in flight (collect
        still returns its PCM); None: the batch of the last decode."""
        if ticket is None:
            held = self._loud_last
        else:
            self._check(self.lib.aacg_pipeline_collect(self.handle, ticket))
            held = self._loud.pop(ticket, None)
        if held is None:
            raise ValueError("Pipeline.take_loudness: no records are held for that batch (no meter, or taken already)")
        rec, n = held
        ends = np.cumsum(n.astype(np.int64))
        return [rec[(e - k) * self.in_channels * 2:e * self.in_channels * 2].reshape(int(k), self.in_channels, 2) for e, k in zip(ends, n.astype(np.int64))]

    def take_true_peak(self, ticket=None):
        """The true-peak records of a batch: a list with one (n_out[s], in_channels) float32 array per stream, a float per hop of the
        meter.  ticket: a submitted batch's, which is finished first if it is still in flight (collect still returns its PCM and
        take_loudness its records, in any order); None: the batch of the last decode."""
        if ticket is None:
            held = self._tp_last
        else:
            self._check(self.lib.aacg_pipeline_collect(self.handle, ticket))
            held = self._tp.pop(ticket, None)
        if held is None:
            raise ValueError("Pipeline.take_true_peak: no records are held for that batch (no true-peak stage, or taken already)")
        tp, n = held
        ends = np.cumsum(n.astype(np.int64))
        return [tp[(e - k) * self.in_channels:e * self.in_channels].reshape(int(k), self.in_channels) for e, k in zip(ends, n.astype(np.int64))]

    def out_samples(self, slots, frames_per_stream):
        """aacg_pipeline_out_samples: the samples per channel that the NEXT batch of these slots with these counts emits, per stream —
        with a feature stage the feature frames"""
        slots = np.ascontiguousarray(slots, np.uint32)
        counts = np.ascontiguousarray(frames_per_stream, np.uint32) if np.ndim(frames_per_stream) else np.full(len(slots), int(frames_per_stream), np.uint32)
        assert len(counts) == len(slots)
        n = np.zeros(len(slots), np.uint32)
        self._check(self.lib.aacg_pipeline_out_samples(self.handle, slots.ctypes.data, counts.ctypes.data, len(slots), n.ctypes.data))
        return n

    def stream_layout(self, slot):
        """(channels of every element of the slot's frames, how many of the elements are decoded); ([], 0) before it is learnt."""
        ch, kept = np.zeros(8, np.uint8), C.c_uint32()
        n = self.lib.aacg_pipeline_stream_layout(self.handle, slot, ch.ctypes.data, C.byref(kept))
        if n < 0:
            raise AacgError(n, "aacg_pipeline_stream_layout")
        return [int(c) for c in ch[:n]], int(kept.value)

    def stream_window_shape(self, slot):
        """The window shape (0 sine, 1 KBD) each of the slot's channels carries into its next frame (carry_window_shape pipelines;
        zeros otherwise).  Finishes the batches in flight first."""
        sh = np.zeros(8, np.uint8)
        self._check(self.lib.aacg_pipeline_stream_window_shape(self.handle, slot, sh.ctypes.data))
        return [int(v) for v in sh[:self.in_channels]]

    def plan_builds(self):
        """how many plans the pipeline has built (one per batch shape it had not kept)"""
        return int(self.lib.aacg_pipeline_plan_builds(self.handle))

    def launch_counts(self):
        """{"shaped": batches whose plan was shaped on the device, "chained": transform launches that continued their predecessor
        through the cross-launch cells, "launches": transform launches} (aacg_pipeline_launch_counts)"""
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self.lib.aacg_pipeline_launch_counts(self.handle, C.byref(a), C.byref(b), C.byref(c)))
        return {"shaped": int(a.value), "chained": int(b.value), "launches": int(c.value)}

    def _args(self, data, frames, slots, frames_per_stream, pcm):
        data = np.ascontiguousarray(data, np.uint8)
        frames = np.ascontiguousarray(frames)
        slots = np.ascontiguousarray(slots, np.uint32)
        if np.ndim(frames_per_stream):
            counts = np.ascontiguousarray(frames_per_stream, np.uint32)
            assert len(counts) == len(slots)
            total = int(counts.sum())
        else:
            counts, total = None, len(slots) * int(frames_per_stream)
        assert frames.dtype == PARSE_FRAME_DTYPE and len(frames) == total
        n = len(frames)
        # a resampled pipeline: what each stream will emit (the clocks stand still until the batch is enqueued)
        self._ragged = bool(self.resample or self.features or self.trim)
        self._lengths = self.out_samples(slots, frames_per_stream).astype(np.int64) if self._ragged else None
        samples = int(self._lengths.sum()) if self._ragged else n * 1024
        width, dtype = (self.features["n_mels"], np.float32) if self.features else (self.channels, np.int16 if self.i16 else np.float32)
        if pcm is None:
            pcm = np.zeros(samples * width, dtype)
        assert pcm.size >= samples * width and (not self.features or pcm.dtype == np.float32)
        return data, frames, slots, counts, pcm, np.zeros(n, PARSE_RESULT_DTYPE), C.c_uint32(0)

    def decode(self, data, frames, slots, frames_per_stream, pcm=None):
        """Synchronous: (pcm, results, n_refused).  frames[s * F + f] = frame f of stream s in `data`.  frames_per_stream may be a
        sequence of per-stream counts (aacg_pipeline_decode_ragged): frames, PCM and results are then packed stream after stream."""
        data, frames, slots, counts, pcm, res, refused = self._args(data, frames, slots, frames_per_stream, pcm)
        self._loud_last = self._arm_loudness(slots, frames_per_stream)
        self._tp_last = self._tp_armed
        if counts is None:
            self._check(self.lib.aacg_pipeline_decode(self.handle, data.ctypes.data, data.size, frames.ctypes.data, slots.ctypes.data, len(slots),
                                                      frames_per_stream, pcm.ctypes.data, res.ctypes.data, C.byref(refused)))
        else:
            self._check(self.lib.aacg_pipeline_decode_ragged(self.handle, data.ctypes.data, data.size, frames.ctypes.data, slots.ctypes.data, len(slots),
                                                             counts.ctypes.data, pcm.ctypes.data, res.ctypes.data, C.byref(refused)))
        return (pcm, res, int(refused.value)) + ((self._lengths,) if self._ragged else ())

    def submit(self, data, frames, slots, frames_per_stream, pcm=None):
        """Asynchronous: returns a ticket; collect(ticket) -> (pcm, results, n_refused).  frames_per_stream as for decode."""
        data, frames, slots, counts, pcm, res, refused = self._args(data, frames, slots, frames_per_stream, pcm)
        loud = self._arm_loudness(slots, frames_per_stream)
        t = C.c_uint64()
        if counts is None:
            self._check(self.lib.aacg_pipeline_submit(self.handle, data.ctypes.data, data.size, frames.ctypes.data, slots.ctypes.data, len(slots),
                                                      frames_per_stream, pcm.ctypes.data, res.ctypes.data, C.byref(refused), C.byref(t)))
        else:
            self._check(self.lib.aacg_pipeline_submit_ragged(self.handle, data.ctypes.data, data.size, frames.ctypes.data, slots.ctypes.data, len(slots),
                                                             counts.ctypes.data, pcm.ctypes.data, res.ctypes.data, C.byref(refused), C.byref(t)))
        self._keep[t.value] = (pcm, res, refused) + ((self._lengths,) if self._ragged else ())
        if loud is not None:
            self._loud[t.value] = loud
        if self._tp_armed is not None:
            self._tp[t.value] = self._tp_armed
        return t.value

    def collect(self, ticket):
        """(pcm, results, n_refused) of a submitted batch; for a submit_device ticket pcm is the `out` that was given"""
        self._check(self.lib.aacg_pipeline_collect(self.handle, ticket))
        pcm, res, refused, *lengths = self._keep.pop(ticket)
        return (pcm, res, int(refused.value)) + tuple(lengths)

    @staticmethod
    def _device_memory(out):
        """(address, bytes) of `out`: anything with data_ptr() and nbytes or numel() * element_size() (a torch tensor), or the pair"""
        if hasattr(out, "data_ptr"):
            addr = out.data_ptr()
            nbytes = out.nbytes if hasattr(out, "nbytes") else out.numel() * out.element_size()
        else:
            try:
                addr, nbytes = out
            except (TypeError, ValueError):
                raise TypeError("submit_device: out is neither a tensor (data_ptr(), nbytes) nor an (address, nbytes) pair")
        if not isinstance(addr, int) or isinstance(addr, bool) or addr <= 0 or int(nbytes) < 0:
            raise ValueError("submit_device: out has no device address")
        return addr, int(nbytes)

    def submit_device(self, data, frames, slots, frames_per_stream, out, planar=False, stride_frames=None, layout=None):
        """Asynchronous, the PCM left on the device (aacg_pipeline_submit_device): returns a ticket; collect(ticket) ->
        (out, results, n_refused).  out: device memory of the pipeline's device, 16-byte aligned — a torch tensor, or an
        (address, nbytes) pair.  Packed (the default): [frame][1024][channels] as submit's PCM.  planar: [stream][channel]
        [stride_frames * 1024], zeros behind a stream's samples; stride_frames defaults to the largest count.  frames_per_stream:
        a scalar or per-stream counts, as for submit.  The batch writes out on a stream of the pipeline's, ordered behind nothing of
        the caller's: work already queued that reads or writes out's memory (torch's allocator hands a block freed on a stream out
        again while that stream's kernels on it are still queued) must have completed when this is called — synchronise that stream
        first, as decode_tensor does.  From then on out must stay untouched until collect, or until the stream given to wait_device
        has passed the wait.  layout: an AACG_PCM_* code given as such, in the place of planar."""
        addr, nbytes = self._device_memory(out)             # (before the library is called: an `out` without an address never reaches it)
        data = np.ascontiguousarray(data, np.uint8)
        frames = np.ascontiguousarray(frames)
        slots = np.ascontiguousarray(slots, np.uint32)
        counts = np.ascontiguousarray(frames_per_stream, np.uint32) if np.ndim(frames_per_stream) else np.full(len(slots), int(frames_per_stream), np.uint32)
        assert len(counts) == len(slots) and frames.dtype == PARSE_FRAME_DTYPE and len(frames) == int(counts.sum())
        lengths = self.out_samples(slots, counts).astype(np.int64) if self.resample or self.features or self.trim else None
        if planar and stride_frames is None:
            if self.features:                                     # rows of feature frames: the longest stream's count (at least one)
                stride_frames = max(int(lengths.max()) if len(lengths) else 0, 1)
            else:
                stride_frames = (int(counts.max()) if len(counts) else 0) if lengths is None else max((int(lengths.max()) + 1023) // 1024, 1 if self.trim else 0)
        desc = PcmDeviceOut(addr, nbytes, (PCM_PLANAR if planar else PCM_PACKED) if layout is None else int(layout), int(stride_frames or 0))
        res, refused, t = np.zeros(len(frames), PARSE_RESULT_DTYPE), C.c_uint32(0), C.c_uint64()
        loud = self._arm_loudness(slots, counts)
        self._check(self.lib.aacg_pipeline_submit_device(self.handle, data.ctypes.data, data.size, frames.ctypes.data, slots.ctypes.data, len(slots),
                                                         counts.ctypes.data, C.byref(desc), res.ctypes.data, C.byref(refused), C.byref(t)))
        self._keep[t.value] = (out, res, refused) + ((lengths,) if lengths is not None else ())
        if loud is not None:
            self._loud[t.value] = self._loud_last = loud
        if self._tp_armed is not None:
            self._tp[t.value] = self._tp_last = self._tp_armed
        return t.value

    def wait_device(self, ticket, stream=None):
        """Puts a HIP stream behind the ticket's batch without the host waiting (aacg_pipeline_wait_device): what is queued on it
        afterwards sees the batch's PCM.  stream: a hipStream_t as an integer, or anything with .cuda_stream (a torch stream);
        None: torch's current stream on the pipeline's device when torch is imported, else the null stream."""
        if stream is None:
            import sys
            torch = sys.modules.get("torch")
            stream = torch.cuda.current_stream(self.device).cuda_stream if torch is not None and torch.cuda.is_available() else 0
        stream = getattr(stream, "cuda_stream", stream)
        self._check(self.lib.aacg_pipeline_wait_device(self.handle, ticket, C.c_void_p(int(stream) or None)))

    def decode_tensor(self, data, frames, slots, frames_per_stream, planar=True):
        """One batch into a new torch tensor on the pipeline's device -> (tensor, lengths, results, n_refused).  C below is
        self.channels: the channels that leave, O for a pipeline with a mix.  planar:
        (B, C, max count * 1024) with lengths[s] = count * 1024 samples of stream s and zeros behind them; packed: (n, 1024, C),
        the n frames stream after stream.  The tensor is torch's current stream's: that stream is synchronised before the batch is
        submitted, because the allocator may hand out a block whose previous user's kernels are still queued there and the lane's
        stream would write under them (or a late fill land in the PCM); afterwards the stream is put behind the batch, so work queued
        on it sees the PCM, and the host has waited for the results only."""
        import torch
        slots = np.ascontiguousarray(slots, np.uint32)
        counts = np.ascontiguousarray(frames_per_stream, np.uint32) if np.ndim(frames_per_stream) else np.full(len(slots), int(frames_per_stream), np.uint32)
        shape = (len(slots), self.channels, int(counts.max()) * 1024) if planar else (int(counts.sum()), 1024, self.channels)
        if self.resample or self.trim:                            # rows of whole kilosamples that hold the longest stream (a trim: at least one); packed: flat (samples, C)
            n_out = self.out_samples(slots, counts)
            shape = (len(slots), self.channels, max((int(n_out.max()) + 1023) // 1024, 1 if self.trim else 0) * 1024) if planar else (int(n_out.sum()), self.channels)
        if self.features:                                         # (S, n_mels, T) with T the longest stream's feature frames; packed: flat (frames, n_mels)
            n_out = self.out_samples(slots, counts)
            shape = (len(slots), self.features["n_mels"], max(int(n_out.max()), 1)) if planar else (int(n_out.sum()), self.features["n_mels"])
        out = torch.empty(shape, dtype=torch.int16 if self.i16 and not self.features else torch.float32, device="cuda:%d" % self.device)
        torch.cuda.current_stream(self.device).synchronize()      # nothing of the block's previous life is still queued when the lane writes it
        t = self.submit_device(data, frames, slots, counts, out, planar=bool(planar))
        self.wait_device(t)
        out, res, refused, *lengths = self.collect(t)
        return out, lengths[0] if lengths else counts.astype(np.int64) * 1024, res, refused


def trim_design(skip_in, keep_in=None, limiter=False, resample=None, delay=None):
    """aacg_trim_design: the window at the trim's input for a window (skip_in, keep_in) in samples of the stream's own rate and time —
    (skip, keep, residual) with keep None for no end and residual a fractions.Fraction in [0, 1) output samples.  limiter: the pipeline
    has one (64 samples of delay); resample: the pipeline's (L, M, table) or (L, M, taps) with a linear-phase table.  delay: the
    limiter's delay in samples in the place of `limiter` (Pipeline.limiter_delay(): aacg_trim_design_delay).  Host code, exact."""
    import fractions
    L, M, taps = (1, 1, 0) if resample is None else (int(resample[0]), int(resample[1]), int(resample[2]) if np.ndim(resample[2]) == 0 else int(np.shape(resample[2])[1]))
    s, k, num, den = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    if delay is not None:
        rc = load_library().aacg_trim_design_delay(int(skip_in), TRIM_ALL if keep_in is None else int(keep_in), int(delay), L, M, taps,
                                                   C.byref(s), C.byref(k), C.byref(num), C.byref(den))
    else:
        rc = load_library().aacg_trim_design(int(skip_in), TRIM_ALL if keep_in is None else int(keep_in), 1 if limiter else 0, L, M, taps,
                                             C.byref(s), C.byref(k), C.byref(num), C.byref(den))
    if rc != 0:
        raise AacgError(rc, "aacg_trim_design(%d, %r, %d / %d, %d taps)" % (skip_in, keep_in, L, M, taps))
    return int(s.value), None if k.value == TRIM_ALL else int(k.value), fractions.Fraction(int(num.value), int(den.value))


def trim_counts(position, skip, keep, n_in):
    """aacg_trim_counts: (first_of, kept_of), uint32 arrays — of consecutive pieces of n_in[i] samples, the first at `position`, piece
    i keeps kept_of[i] samples beginning at its first_of[i]-th under the window (skip, keep), keep None: no end.  Host code."""
    n_in = np.ascontiguousarray(n_in, np.uint32)
    first, kept = np.zeros(len(n_in), np.uint32), np.zeros(len(n_in), np.uint32)
    rc = load_library().aacg_trim_counts(int(position), int(skip), TRIM_ALL if keep is None else int(keep), n_in.ctypes.data, len(n_in), first.ctypes.data, kept.ctypes.data)
    if rc != 0:
        raise AacgError(rc, "aacg_trim_counts(%d, %d, %r)" % (position, skip, keep))
    return first, kept


def mix_standard(channels, out_channels, surround_gain=2 ** -0.5, normalise=True):
    """The project's standard downmix (aacg_mix_standard, include/aacgpu.h has the table) as an (out_channels, channels) float32 matrix
    for Pipeline(mix=...): host code, no device."""
    m = np.zeros((int(out_channels), int(channels)), np.float32)
    rc = load_library().aacg_mix_standard(int(channels), int(out_channels), float(surround_gain), 1 if normalise else 0, m.ctypes.data)
    if rc != 0:
        raise AacgError(rc, "aacg_mix_standard(%d channels to %d)" % (channels, out_channels))
    return m


def resample_design(in_rate, out_rate, taps=32, rolloff=0.0, beta=0.0):
    """The project's default resampling table (aacg_resample_design, include/aacgpu.h): (L, M, table) with table (L, taps) float32, for
    Pipeline(resample=...): host code, no device.  rolloff and beta 0: the defaults, 0.95 and 9."""
    lib, L, M = load_library(), C.c_uint32(), C.c_uint32()
    rc = lib.aacg_resample_design(int(in_rate), int(out_rate), int(taps), float(rolloff), float(beta), C.byref(L), C.byref(M), None, 0)
    if rc == 0:
        table = np.zeros((L.value, int(taps)), np.float32)
        rc = lib.aacg_resample_design(int(in_rate), int(out_rate), int(taps), float(rolloff), float(beta), C.byref(L), C.byref(M), table.ctypes.data, table.size)
    if rc != 0:
        raise AacgError(rc, "aacg_resample_design(%d -> %d Hz, %d taps)" % (in_rate, out_rate, taps))
    return int(L.value), int(M.value), table


def loudness_design(rate, hop=None):
    """BS.1770's K-weighting at `rate` (aacg_loudness_design, include/aacgpu.h): a dict for Pipeline(loudness=...) with the two biquad
    sections as a (2, 5) float32 matrix; host code, no device.  hop None: rate // 10, so that four hops are the standard's 400 ms block."""
    k = np.zeros((2, 5), np.float32)
    rc = load_library().aacg_loudness_design(int(rate), k.ctypes.data)
    if rc != 0:
        raise AacgError(rc, "aacg_loudness_design(%d Hz)" % rate)
    return {"hop": int(rate) // 10 if hop is None else int(hop), "coeffs": k}


def true_peak_design(phases=4, taps=24, rolloff=0.95, beta=5.0):
    """aacg_true_peak_design: a dict for Pipeline(true_peak=...) with the oversampling table (phases, taps) float32 — the resampler's
    default design for 1 -> phases; host code, no device.  The defaults read sines up to 20 kHz at 48 kHz within EBU Tech 3341's
    tolerance."""
    table = np.zeros((int(phases), int(taps)), np.float32)
    rc = load_library().aacg_true_peak_design(int(phases), int(taps), float(rolloff), float(beta), table.ctypes.data, table.size)
    if rc != 0:
        raise AacgError(rc, "aacg_true_peak_design(%d phases of %d taps)" % (phases, taps))
    return {"phases": int(phases), "taps": int(taps), "table": table}


def limiter_design(rate, ceiling_db=-1.0, release_ms=200.0):
    """aacg_limiter_design: a LimiterConfig for Pipeline(limiter=...) — ceiling = 10^(ceiling_db / 20) in full-scale units, release = the
    share of the way back to a slot's gain that a block of 64 samples covers at a time constant of release_ms at `rate`"""
    cfg = LimiterConfig()
    rc = load_library().aacg_limiter_design(int(rate), float(ceiling_db), float(release_ms), C.byref(cfg))
    if rc != 0:
        raise AacgError(rc, "aacg_limiter_design(%d Hz, %g dB, %g ms)" % (rate, ceiling_db, release_ms))
    return cfg


def loudness_counts(hop, n0, samples):
    """aacg_loudness_counts: the records per channel that `samples` further samples complete at the clock n0"""
    n = C.c_uint64()
    rc = load_library().aacg_loudness_counts(int(hop), int(n0), int(samples), C.byref(n))
    if rc != 0:
        raise AacgError(rc, "aacg_loudness_counts(hop %d)" % hop)
    return int(n.value)


def loudness_integrate(records, hop, weights=None, momentary=False):
    """aacg_loudness_integrate: the gated loudness in LUFS (-inf: nothing above the gates) of one stream's records (n_hops, channels, 2)
    as take_loudness gives them — concatenate a stream's batches first.  weights: per channel, None all 1.  momentary: also the
    400 ms-block loudness of every block, (integrated, array of n_hops - 3)."""
    r = np.ascontiguousarray(records, np.float32)
    if r.ndim != 3 or r.shape[2] != 2:
        raise ValueError("loudness_integrate: records are not (n_hops, channels, 2)")
    w = None if weights is None else np.ascontiguousarray(weights, np.float64)
    if w is not None and w.shape != (r.shape[1],):
        raise ValueError("loudness_integrate: one weight per channel")
    out, mom = C.c_double(), np.zeros(max(r.shape[0] - 3, 0), np.float64)
    rc = load_library().aacg_loudness_integrate(r.ctypes.data, r.shape[0], r.shape[1], int(hop), None if w is None else w.ctypes.data, C.byref(out),
                                                mom.ctypes.data if momentary else None)
    if rc != 0:
        raise AacgError(rc, "aacg_loudness_integrate(%d hops of %d channels)" % r.shape[:2])
    return (out.value, mom) if momentary else out.value


def features_design(rate=16000, frame_length=400, hop=160, n_bins=None, n_mels=80, f_min=0.0, f_max=0.0):
    """The usual tables of a feature stage (aacg_features_design, include/aacgpu.h): a dict for Pipeline(features=...) with the
    periodic-Hann Fourier basis (2 n_bins, frame_length) and the Slaney mel filterbank (n_mels, n_bins); host code, no device.
    n_bins None: frame_length // 2 + 1; f_max 0: rate / 2.  The defaults are Whisper's; add pad_left, log and floor as wanted."""
    n_bins = int(frame_length) // 2 + 1 if n_bins is None else int(n_bins)
    basis, fb = np.zeros((2 * n_bins, int(frame_length)), np.float32), np.zeros((int(n_mels), n_bins), np.float32)
    rc = load_library().aacg_features_design(int(rate), int(frame_length), int(hop), n_bins, int(n_mels), float(f_min), float(f_max),
                                             basis.ctypes.data, basis.size, fb.ctypes.data, fb.size)
    if rc != 0:
        raise AacgError(rc, "aacg_features_design(%d Hz, %d / %d, %d bins, %d mels)" % (rate, frame_length, hop, n_bins, n_mels))
    return {"frame_length": int(frame_length), "hop": int(hop), "basis": basis, "fb": fb}


def features_counts(frame_length, hop, pad_left, n0, samples):
    """aacg_features_counts: the feature frames that `samples` further samples complete at the clock n0"""
    n = C.c_uint64()
    rc = load_library().aacg_features_counts(int(frame_length), int(hop), int(pad_left), int(n0), int(samples), C.byref(n))
    if rc != 0:
        raise AacgError(rc, "aacg_features_counts(%d / %d, pad %d)" % (frame_length, hop, pad_left))
    return int(n.value)


def resample_counts(L, M, n0, frames):
    """aacg_resample_counts: (samples each of `frames` consecutive frames emits at L / M from the clock n0, the clock modulo M after them)"""
    per, after = np.zeros(int(frames), np.uint32), C.c_uint32()
    rc = load_library().aacg_resample_counts(int(L), int(M), int(n0), int(frames), per.ctypes.data, C.byref(after))
    if rc != 0:
        raise AacgError(rc, "aacg_resample_counts(%d / %d)" % (L, M))
    return per, int(after.value)


class Plan:
    def __init__(self, engine, handle, n_units):
        self.engine, self.handle, self.n_units = engine, handle, n_units

    def destroy(self):
        if self.handle:
            self.engine.lib.aacg_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class Engine:
    """One engine per device (mirrors one FilterBank per decoder, for many streams at once)."""

    def __init__(self, input_kind=INPUT_QUANT_I16, max_streams=1, max_channels=2, device=0, sample_index=3,
                 max_batch_units=0, tns_mode=TNS_REFERENCE, pns_mode=PNS_REFERENCE, output_kind=OUTPUT_F32, cce_mode=CCE_REFERENCE):
        self.lib = load_library()
        cfg = Config(self.lib.aacg_abi_version(), device, sample_index, max_streams, max_channels, max_batch_units,
                     input_kind, tns_mode, pns_mode, output_kind, cce_mode)
        self.pcm_dtype = np.int16 if output_kind == OUTPUT_I16 else np.float32
        h = C.c_void_p()
        rc = self.lib.aacg_create(C.byref(cfg), C.byref(h))
        if rc:
            raise AacgError(rc, "aacg_create failed (is a GPU visible?)")
        self.handle = h
        self.input_kind = input_kind
        self.max_streams, self.max_channels = max_streams, max_channels

    def close(self):
        if self.handle:
            self.lib.aacg_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc < 0:
            raise AacgError(rc, self.lib.aacg_last_error(self.handle).decode())
        return rc

    # -- host-buffer path -----------------------------------------------------------------
    def decode_batch(self, units, coeffs, meta, n_pcm_floats, tns=None, cce=None, out=None):
        """out: an array to decode into (a caller that reuses its output buffer, as a real host does; default: a fresh one
        filled with NaN so that tests see every sample that was not written)."""
        if cce is not None:
            return self._decode_batch_ex(units, coeffs, meta, n_pcm_floats, tns, cce)
        units = np.ascontiguousarray(units)
        assert units.dtype == UNIT_DTYPE
        coeffs = np.ascontiguousarray(coeffs)
        assert coeffs.dtype == (np.int16 if self.input_kind == INPUT_QUANT_I16 else np.float32)
        n_blocks = coeffs.size // 1024
        if meta is not None:
            meta = np.ascontiguousarray(meta, np.uint16)
        if out is not None:
            assert out.dtype == self.pcm_dtype and out.size >= n_pcm_floats and out.flags["C_CONTIGUOUS"]
            pcm = out
        else:
            pcm = np.full(n_pcm_floats, np.nan, np.float32) if self.pcm_dtype == np.float32 else np.full(n_pcm_floats, -32768, np.int16)
        if tns is not None:
            tns = np.ascontiguousarray(tns)
            assert tns.dtype == TNS_DTYPE
            self._check(self.lib.aacg_decode_batch_tns(self.handle, units.ctypes.data, len(units), coeffs.ctypes.data, n_blocks,
                                                       meta.ctypes.data if meta is not None else None,
                                                       meta.size // 120 if meta is not None else 0,
                                                       tns.ctypes.data, len(tns), pcm.ctypes.data, pcm.size))
            return pcm
        self._check(self.lib.aacg_decode_batch(self.handle, units.ctypes.data, len(units), coeffs.ctypes.data, n_blocks,
                                               meta.ctypes.data if meta is not None else None,
                                               meta.size // 120 if meta is not None else 0, pcm.ctypes.data, pcm.size))
        return pcm

    def _decode_batch_ex(self, units, coeffs, meta, n_pcm_floats, tns, cce):
        """aacg_decode_batch_ex: every array of the batch in one record (coupling side info included)."""
        units, coeffs, cce = np.ascontiguousarray(units), np.ascontiguousarray(coeffs), np.ascontiguousarray(cce)
        assert units.dtype == UNIT_DTYPE and cce.dtype == CCE_DTYPE
        meta = np.ascontiguousarray(meta, np.uint16) if meta is not None else None
        tns = np.ascontiguousarray(tns) if tns is not None else None
        pcm = np.full(n_pcm_floats, np.nan, np.float32)
        b = Batch(units.ctypes.data, len(units), coeffs.ctypes.data, coeffs.size // 1024,
                  meta.ctypes.data if meta is not None else None, meta.size // 120 if meta is not None else 0,
                  tns.ctypes.data if tns is not None else None, len(tns) if tns is not None else 0,
                  cce.ctypes.data, len(cce), pcm.ctypes.data, pcm.size)
        self._check(self.lib.aacg_decode_batch_ex(self.handle, C.byref(b)))
        return pcm

    def submit(self, units, coeffs, meta, pcm, tns=None):
        """Asynchronous decode_batch into the caller's `pcm` array (keep every array alive until wait)."""
        assert units.dtype == UNIT_DTYPE and units.flags.c_contiguous and coeffs.flags.c_contiguous and pcm.flags.c_contiguous
        t = C.c_uint64()
        if tns is not None:
            assert tns.dtype == TNS_DTYPE and tns.flags.c_contiguous
            self._check(self.lib.aacg_submit_tns(self.handle, units.ctypes.data, len(units), coeffs.ctypes.data, coeffs.size // 1024,
                                                 meta.ctypes.data if meta is not None else None,
                                                 meta.size // 120 if meta is not None else 0,
                                                 tns.ctypes.data, len(tns), pcm.ctypes.data, pcm.size, C.byref(t)))
            return t.value
        self._check(self.lib.aacg_submit(self.handle, units.ctypes.data, len(units), coeffs.ctypes.data, coeffs.size // 1024,
                                         meta.ctypes.data if meta is not None else None,
                                         meta.size // 120 if meta is not None else 0, pcm.ctypes.data, pcm.size, C.byref(t)))
        return t.value

    def wait(self, ticket):
        self._check(self.lib.aacg_wait(self.handle, ticket))

    def pinned(self, shape, dtype):
        """numpy array over page-locked host memory (aacg_host_alloc): transfers from/to it are asynchronous."""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = self.lib.aacg_host_alloc(n)
        if not p:
            raise AacgError(-3, "aacg_host_alloc failed")
        buf = (C.c_char * n).from_address(p)
        a = np.frombuffer(buf, dtype=dtype).reshape(shape)
        self._pinned = getattr(self, "_pinned", [])
        self._pinned.append(p)
        return a

    # -- device-resident path -----------------------------------------------------------------
    def plan(self, units, tns=None, cce=None):
        units = np.ascontiguousarray(units)
        assert units.dtype == UNIT_DTYPE
        h = C.c_void_p()
        if cce is not None:
            cce = np.ascontiguousarray(cce)
            assert cce.dtype == CCE_DTYPE
            tns = np.ascontiguousarray(tns) if tns is not None else None
            self._check(self.lib.aacg_plan_create_ex(self.handle, units.ctypes.data, len(units), tns.ctypes.data if tns is not None else None,
                                                     len(tns) if tns is not None else 0, cce.ctypes.data, len(cce), C.byref(h)))
            return Plan(self, h, len(units))
        if tns is not None:
            tns = np.ascontiguousarray(tns)
            assert tns.dtype == TNS_DTYPE
            self._check(self.lib.aacg_plan_create_tns(self.handle, units.ctypes.data, len(units), tns.ctypes.data, len(tns), C.byref(h)))
            return Plan(self, h, len(units))
        self._check(self.lib.aacg_plan_create(self.handle, units.ctypes.data, len(units), C.byref(h)))
        return Plan(self, h, len(units))

    def plan_shaped(self, max_streams, max_frames, max_elems=1, n_sets=1, stages=False):
        """aacg_plan_create_shaped: a plan with a capacity instead of a shape, shaped on the device batch by batch
        (stages: aacg_plan_create_shaped_stages, the one for decode_pipelined_stages on a SPEC engine)."""
        h = C.c_void_p()
        make = self.lib.aacg_plan_create_shaped_stages if stages else self.lib.aacg_plan_create_shaped
        self._check(make(self.handle, max_streams, max_frames, max_elems, n_sets, C.byref(h)))
        return Plan(self, h, 0)

    def plan_shape_table(self, plan, set_index, table, parse_channels):
        """aacg_plan_shape_table: checks and completes the batch's table (SHAPE_STREAM_DTYPE, in place); -> the shape's plan units."""
        assert table.dtype == SHAPE_STREAM_DTYPE and table.flags["C_CONTIGUOUS"]
        n = C.c_uint32()
        self._check(self.lib.aacg_plan_shape_table(self.handle, plan.handle, set_index, table.ctypes.data, len(table), parse_channels, C.byref(n)))
        return int(n.value)

    def plan_stages(self, units):
        """aacg_plan_create_stages: a kept plan whose launches bring the optional stages' records (decode_pipelined_stages)"""
        units = np.ascontiguousarray(units)
        assert units.dtype == UNIT_DTYPE
        h = C.c_void_p()
        self._check(self.lib.aacg_plan_create_stages(self.handle, units.ctypes.data, len(units), C.byref(h)))
        return Plan(self, h, len(units))

    def decode_pipelined_stages(self, plan, d_coeffs, d_meta, d_tns_records, n_tns_records, d_pcm):
        self._check(self.lib.aacg_decode_pipelined_stages(self.handle, plan.handle, d_coeffs, d_meta, d_tns_records, n_tns_records, d_pcm))

    def tns_records_bytes(self, n_records):
        return int(self.lib.aacg_tns_records_bytes(n_records))

    def tns_records_from_parse(self, d_parsed_units, d_results, d_tns_info, n_frames, max_units, parse_channels, d_records, stream=0):
        """aacg_tns_records_from_parse: the batch's TNS records (DEV_TNS_DTYPE) and their matrices from aacg_parse_device's outputs,
        on the device; d_* raw device addresses, d_records of tns_records_bytes(n_frames * parse_channels) bytes."""
        self._check(self.lib.aacg_tns_records_from_parse(self.handle, d_parsed_units, d_results, d_tns_info, n_frames, max_units, parse_channels,
                                                         d_records, stream))

    def decode_device(self, plan, d_coeffs, d_meta, d_pcm, stream=0):
        """d_* are raw device addresses (e.g. torch.Tensor.data_ptr()); stream a hipStream_t handle or 0."""
        self._check(self.lib.aacg_decode_device(self.handle, plan.handle, d_coeffs, d_meta, d_pcm, stream))

    def decode_pipelined(self, plan, d_coeffs, d_meta, d_pcm, mark=None):
        """aacg_decode_pipelined: the next launch of `plan` on the engine's internal streams taken in turn; it may overlap the
        launch before it (their chains meet in rendezvous cells).  Results: after pipeline_join / synchronize.
        mark: a TimerMark bound to the launch's completion (aacg_decode_pipelined_timed; measurement only)."""
        if mark is not None:
            self._check(self.lib.aacg_decode_pipelined_timed(self.handle, plan.handle, d_coeffs, d_meta, d_pcm, mark.h))
        else:
            self._check(self.lib.aacg_decode_pipelined(self.handle, plan.handle, d_coeffs, d_meta, d_pcm))

    def pipeline_fork(self, stream):
        """The pipeline's later launches start after everything enqueued on `stream` so far."""
        self._check(self.lib.aacg_pipeline_fork(self.handle, stream))

    def pipeline_join(self, stream=0):
        """Work enqueued on `stream` from now on starts after the pipeline's launches so far; 0: the host waits for them."""
        self._check(self.lib.aacg_pipeline_join(self.handle, stream or None))

    def pipeline_chained(self):
        """Launches of decode_pipelined that continued (and were allowed to overlap) the launch before them."""
        return int(self.lib.aacg_pipeline_chained(self.handle))

    def pipeline_streams_used(self):
        """How many of the engine's internal streams the current pipelined sequence takes in turn (0 before the first launch)."""
        return int(self.lib.aacg_pipeline_streams_used(self.handle))

    def pipeline_info(self):
        """(streams the current pipelined sequence takes in turn, whether they were seen to run side by side: 1 / 0 / -1 before set-up)."""
        a, b = C.c_int(), C.c_int()
        self._check(self.lib.aacg_pipeline_info(self.handle, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_wait_limit_ms(self, ms):
        self._check(self.lib.aacg_set_wait_limit_ms(self.handle, int(ms)))

    def debug_set_wait_mode(self, mode, spin_us=-1.0):
        self._check(self.lib.aacg_debug_set_wait_mode(self.handle, mode, float(spin_us)))

    def debug_stall(self, which, ms):
        """One of the engine's streams (0: its own, 1..3: the pipeline's) busy for `ms` milliseconds: tests of the bounded waits."""
        self.lib.aacg_debug_stall.argtypes = [C.c_void_p, C.c_int, C.c_uint32]
        self._check(self.lib.aacg_debug_stall(self.handle, which, ms))

    def in_flight(self):
        buf = C.create_string_buffer(4096)
        self.lib.aacg_debug_in_flight(self.handle, buf, 4096)
        return buf.value.decode()

    def pipeline_concurrent(self):
        """True if the engine's internal streams were seen to run side by side (else pipelined launches serialise: correct, not faster)."""
        return bool(self.lib.aacg_pipeline_concurrent(self.handle))

    def plan_refresh_from_parse(self, plan, d_parsed_units, d_results, max_units, d_refused, stream=0):
        """Device pointers: the plan's unit records take what aacg_parse_device wrote (run tables unchanged)."""
        self._check(self.lib.aacg_plan_refresh_from_parse(self.handle, plan.handle, d_parsed_units, d_results, max_units, d_refused, stream))

    def plan_refresh_units(self, plan, units, stream=0):
        """The kept plan takes the next batch's unit records (same structure); raises AacgError(LAYOUT_CHANGE) otherwise."""
        units = np.ascontiguousarray(units)
        assert units.dtype == UNIT_DTYPE
        self._check(self.lib.aacg_plan_refresh_units(self.handle, plan.handle, units.ctypes.data, len(units), stream))

    def spectral_device(self, plan, d_coeffs, d_meta, d_spec, stream=0):
        self._check(self.lib.aacg_spectral_device(self.handle, plan.handle, d_coeffs, d_meta, d_spec, stream))

    def synchronize(self, stream=0):
        self._check(self.lib.aacg_synchronize(self.handle, stream))

    # -- overlap state ------------------------------------------------------------------------
    def get_overlap(self, stream, channel):
        a = np.empty(1024, np.float32)
        self._check(self.lib.aacg_get_overlap(self.handle, stream, channel, a.ctypes.data))
        return a

    def set_overlap(self, stream, channel, values):
        a = np.ascontiguousarray(values, np.float32)
        assert a.size == 1024
        self._check(self.lib.aacg_set_overlap(self.handle, stream, channel, a.ctypes.data))

    def get_window_shape(self, stream, channel):
        """The window shape (0 sine, 1 KBD) of the channel's last frame, as carry_window_shape left it: the other half of the state."""
        v = C.c_uint8()
        self._check(self.lib.aacg_get_window_shape(self.handle, stream, channel, C.byref(v)))
        return int(v.value)

    def set_window_shape(self, stream, channel, shape):
        self._check(self.lib.aacg_set_window_shape(self.handle, stream, channel, int(shape)))

    def carry_window_shape(self, plan, d_map, set=0, stream=0):
        """aacg_plan_carry_window_shape: behind plan_refresh_from_parse_ex on the same stream, window_shape_prev of the set's records
        from the frame before, a stream's first frame from the engine's state.  d_map: the refresh's map (a device address)."""
        self._check(self.lib.aacg_plan_carry_window_shape(self.handle, plan.handle, d_map, set, stream))

    def reset_stream(self, stream):
        self._check(self.lib.aacg_reset_stream(self.handle, stream))

    def table(self, which):
        n = self._check(self.lib.aacg_get_table(self.handle, which, np.empty(1, np.float32).ctypes.data, 0))
        a = np.empty(n, np.float32)
        self._check(self.lib.aacg_get_table(self.handle, which, a.ctypes.data, n))
        return a

    def kernel_name(self):
        return self.lib.aacg_kernel_name().decode()

    def debug_set_route(self, flags):
        """Diagnostic route choices for parity tests (aacg_debug_set_route): 1 = independent coupling as the separate pass."""
        self._check(self.lib.aacg_debug_set_route(self.handle, flags))

    def plan_kernels(self, plan, pipelined=False):
        """The launches aacg_decode_device (pipelined: aacg_decode_pipelined) makes for this plan, by kernel name (what a rocprofv3 kernel trace shows)."""
        buf = C.create_string_buffer(512)
        self._check(self.lib.aacg_plan_kernels_ex(self.handle, plan.handle, 1 if pipelined else 0, buf, 512))
        return buf.value.decode()
