"""lentil_hip_camera_rays_spectral / lentil_hip_trace_points_spectral without a GPU: the symbols, the unchanged ABI, and
what the Python wrappers refuse before anything reaches the library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import common
from pota_amd import _abi, capi
from test_trace_points_host import _from_c

SYMBOLS = ("lentil_hip_camera_rays_spectral", "lentil_hip_trace_points_spectral")


def test_both_symbols_are_declared_and_exported():
    lib = capi.load_library()
    txt = open(os.path.join(common.ROOT, "include", "lentil_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"int\s+lentil_hip_camera_rays_spectral\s*\(\s*lentil_hip_ctx\s*\*ctx,\s*const\s+lentil_camera_ray_batch\s*\*batch,"
                     r"\s*const\s+double\s*\*lambdas\s*\)\s*;", txt)
    assert re.search(r"int\s+lentil_hip_trace_points_spectral\s*\(\s*lentil_hip_ctx\s*\*ctx,\s*const\s+lentil_point_batch\s*\*batch,"
                     r"\s*const\s+double\s*\*lambdas\s*\)\s*;", txt)
    for n in SYMBOLS:
        assert hasattr(lib, n), "liblentil_hip.so does not export %s" % n
        assert n in capi.EXPORTS
    # no context: an error, not a crash -- and no GPU is needed to say so
    assert lib.lentil_hip_camera_rays_spectral(None, None, None) == _abi.ERR_INVALID
    assert lib.lentil_hip_trace_points_spectral(None, None, None) == _abi.ERR_INVALID


def test_the_abi_is_the_one_it_was():
    """additions only: version 1, and the two batch structs keep the sizes they had before the spectral calls"""
    assert capi.load_library().lentil_hip_abi_version() == 1
    got = _from_c('  printf("%d %zu %zu\\n", (int)LENTIL_ABI_VERSION, sizeof(lentil_camera_ray_batch), sizeof(lentil_point_batch));')
    assert got == [1, 64, 80]
    assert (C.sizeof(_abi.CameraRayBatch), C.sizeof(_abi.PointBatch)) == (64, 80)


class _NoLibrary:
    """stands where the library does: a wrapper that gets as far as calling it has not refused"""

    def __getattr__(self, name):
        raise AssertionError("the wrapper called %s" % name)


def _ctx():
    ctx = object.__new__(capi.Context)          # no lentil_hip_create: no GPU
    ctx.lib, ctx.h, ctx.device = _NoLibrary(), C.c_void_p(), 0
    return ctx


def test_wrappers_refuse_a_wrong_lambdas_array():
    import torch
    ctx = _ctx()
    try:
        inp = np.zeros((5, 6), np.float32)
        cs, pixel = np.zeros((5, 3), np.float32), np.zeros(5, np.uint32)
        calls = (lambda lam: ctx.camera_rays(inp, lambdas=lam), lambda lam: ctx.trace_points(cs, pixel, 2, lambdas=lam))
        for call in calls:
            for bad in (np.zeros(4), np.zeros(6), np.zeros((5, 1)),            # the wrong length or shape
                        np.zeros(5, np.float32), np.zeros(5, np.int64),        # the wrong dtype
                        torch.zeros(5, dtype=torch.float64)):                  # a tensor beside numpy arrays
                with pytest.raises(ValueError, match="lambdas"):
                    call(bad)
            with pytest.raises(AssertionError, match="_spectral"):           # a right one goes through to the library
                call(np.zeros(5))
        # ... and the checks of the device form, as far as they go without a device: numpy beside tensors, a tensor that is
        # not on the context's GPU, the wrong dtype
        for bad in (np.zeros(5), torch.zeros(5, dtype=torch.float64), torch.zeros(5, dtype=torch.float32)):
            with pytest.raises(ValueError, match="lambdas"):
                capi._lambdas_arg("camera_rays", bad, 5, 0)
    finally:
        ctx.h = C.c_void_p()                        # (nothing for __del__ to destroy)
