"""lentil_hip_set_visit_lambdas / lentil_hip_spectral_pass_stats without a GPU: the symbols, the flag, the unchanged ABI, and
what the Python wrapper hands to the library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import common
from pota_amd import _abi, capi
from test_trace_points_host import _from_c

SYMBOLS = ("lentil_hip_set_visit_lambdas", "lentil_hip_spectral_pass_stats")


def test_the_symbols_are_declared_and_exported():
    lib = capi.load_library()
    txt = open(os.path.join(common.ROOT, "include", "lentil_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"int\s+lentil_hip_set_visit_lambdas\s*\(\s*lentil_hip_ctx\s*\*ctx,\s*const\s+double\s*\*lambdas,\s*uint64_t\s+n,"
                     r"\s*uint32_t\s+flags\s*\)\s*;", txt)
    assert re.search(r"int\s+lentil_hip_spectral_pass_stats\s*\(\s*lentil_hip_ctx\s*\*ctx,\s*uint64_t\s+stats\[4\]\s*\)\s*;", txt)
    for n in SYMBOLS:
        assert hasattr(lib, n), "liblentil_hip.so does not export %s" % n
        assert n in capi.EXPORTS
    # no context: an error, not a crash -- and no GPU is needed to say so
    assert lib.lentil_hip_set_visit_lambdas(None, None, 0, 0) == _abi.ERR_INVALID
    assert lib.lentil_hip_spectral_pass_stats(None, None) == _abi.ERR_INVALID


def test_the_flag_and_the_abi_version():
    """an addition only: version 1, the structs a pass's caller fills keep their sizes"""
    assert capi.load_library().lentil_hip_abi_version() == 1
    got = _from_c('  printf("%d %u %zu %zu %zu\\n", (int)LENTIL_ABI_VERSION, (unsigned)LENTIL_LAMBDAS_DEVICE_POINTER, sizeof(lentil_params), '
                  'sizeof(lentil_visits), sizeof(lentil_counters));')
    assert got == [1, _abi.LAMBDAS_DEVICE_POINTER, C.sizeof(_abi.Params), C.sizeof(_abi.Visits), C.sizeof(_abi.Counters)]
    assert _abi.LAMBDAS_DEVICE_POINTER == 1


class _Recorder:
    """stands where the library stands: keeps what every call was given"""

    def __init__(self):
        self.calls = []

    def lentil_hip_set_visit_lambdas(self, h, lambdas, n, flags):
        self.calls.append(("set", lambdas, int(n), int(flags)))
        return _abi.OK

    def lentil_hip_spectral_pass_stats(self, h, stats):
        self.calls.append(("stats",))
        stats[0], stats[1], stats[2], stats[3] = 3, 1234, 2, 0
        return _abi.OK


def _ctx(lib):
    ctx = object.__new__(capi.Context)          # no lentil_hip_create: no GPU
    ctx.lib, ctx.h, ctx.device = lib, C.c_void_p(), 0
    return ctx


def test_the_wrapper_hands_over_the_column_as_it_is():
    import torch
    ctx = _ctx(_Recorder())
    try:
        lam = np.array([0.45, 0.0, 0.65, 0.55, 0.5])
        ctx.set_visit_lambdas(lam)
        ctx.set_visit_lambdas([0.5, 0.0])                                   # a plain sequence: its own length
        ctx.set_visit_lambdas(None)
        ctx.set_visit_lambdas()
        calls = ctx.lib.calls
        assert calls[0] == ("set", lam.ctypes.data, 5, 0)                   # the caller's own float64 array, its own length
        assert calls[1][2:] == (2, 0) and calls[1][1]
        assert calls[2] == calls[3] == ("set", None, 0, 0)
        assert ctx.spectral_pass_stats() == (3, 1234, 2, 0) and calls[4] == ("stats",)
        n_calls = len(calls)
        for bad in (np.zeros(5, np.float32), np.zeros(5, np.int64), np.zeros((5, 1)),      # the wrong dtype or shape
                    torch.zeros(5, dtype=torch.float64)):                                   # a tensor as host memory
            with pytest.raises(ValueError, match="lambdas"):
                ctx.set_visit_lambdas(bad)
        # device=True: numpy as device memory, a tensor that is not on the context's GPU, the wrong dtype
        for bad in (np.zeros(5), torch.zeros(5, dtype=torch.float64), torch.zeros(5, dtype=torch.float32)):
            with pytest.raises(ValueError, match="lambdas"):
                ctx.set_visit_lambdas(bad, device=True)
        assert len(calls) == n_calls                                        # (nothing of these reached the library)
    finally:
        ctx.h = C.c_void_p()                        # (nothing for __del__ to destroy)
