"""PCM left on the device (aacg_pipeline_submit_device / aacg_pipeline_wait_device, include/aacgpu.h), without a GPU: the binding's
aacg_pcm_device_out against the header's, the new symbols in the library, and what Pipeline.submit_device refuses by itself."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import aacgpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pcm_device_out_layout_matches_header(tmp_path):
    """sizeof / offsetof of aacg_pcm_device_out from a C probe compiled from the header, and the two layout constants"""
    src = r'''
    #include "include/aacgpu.h"
    #include <stddef.h>
    int sizes[] = { sizeof(aacg_pcm_device_out), offsetof(aacg_pcm_device_out, d_pcm), offsetof(aacg_pcm_device_out, d_pcm_bytes),
                    offsetof(aacg_pcm_device_out, layout), offsetof(aacg_pcm_device_out, stride_frames), AACG_PCM_PACKED, AACG_PCM_PLANAR };
    '''
    c, so = str(tmp_path / "s.c"), str(tmp_path / "s.so")
    open(c, "w").write(src)
    subprocess.run(["gcc", "-shared", "-fPIC", "-I", ROOT, "-o", so, c], check=True)
    got = list((ctypes.c_int * 7).in_dll(ctypes.CDLL(so), "sizes"))
    T = aacgpu.PcmDeviceOut
    assert got == [ctypes.sizeof(T), T.d_pcm.offset, T.d_pcm_bytes.offset, T.layout.offset, T.stride_frames.offset, aacgpu.AACG_PCM_PACKED, aacgpu.AACG_PCM_PLANAR]
    assert got == [24, 0, 8, 16, 20, 0, 1]
    assert [n for n, _ in T._fields_] == ["d_pcm", "d_pcm_bytes", "layout", "stride_frames"]


def test_library_exports_the_new_symbols(engine_lib):
    for name in ("aacg_pipeline_submit_device", "aacg_pipeline_wait_device"):
        assert name in aacgpu.ABI_SYMBOLS and hasattr(engine_lib, name), name
    lib = aacgpu.load_library()
    assert lib.aacg_pipeline_submit_device.argtypes[7]._type_ is aacgpu.PcmDeviceOut and len(lib.aacg_pipeline_submit_device.argtypes) == 11
    assert len(lib.aacg_pipeline_wait_device.argtypes) == 3
    # null handles: the calls answer without a device
    assert lib.aacg_pipeline_wait_device(None, 1, None) == -1
    assert lib.aacg_pipeline_submit_device(None, None, 0, None, None, 0, None, None, None, None, None) == -1


class NoLibrary:
    """stands where the library would: any call into it fails the test"""

    def __getattr__(self, name):
        raise AssertionError("the library was called (%s)" % name)


def test_submit_device_refuses_an_out_without_an_address():
    """an `out` that is no tensor and no (address, nbytes) pair, or whose address is nothing, is refused before the library is called"""
    p = aacgpu.Pipeline.__new__(aacgpu.Pipeline)             # no device here: the object without aacg_pipeline_create
    p.lib, p.handle, p.channels, p.i16, p.device, p._keep = NoLibrary(), None, 2, False, 0, {}
    frames = np.zeros(2, aacgpu.PARSE_FRAME_DTYPE)
    data = np.zeros(64, np.uint8)

    class NullTensor:
        nbytes = 2 * 2048 * 4

        def data_ptr(self):
            return 0

    for out, err in ((None, TypeError), (object(), TypeError), (np.zeros(4096, np.float32), TypeError), ((0, 16384), ValueError), ((None, 16384), ValueError),
                     (NullTensor(), ValueError), ((1.5, 16384), ValueError), ((4096,), TypeError)):
        with pytest.raises(err):
            p.submit_device(data, frames, [0], 2, out)
    assert p._keep == {}
    # what it takes an address from
    assert aacgpu.Pipeline._device_memory((4096, 100)) == (4096, 100)

    class Tensor:
        def data_ptr(self):
            return 8192

        def numel(self):
            return 10

        def element_size(self):
            return 2

    assert aacgpu.Pipeline._device_memory(Tensor()) == (8192, 20)
    p.handle = None                                          # (nothing to destroy)
