"""lentil_hip_list_draws_spectral without a GPU: the symbol, the unchanged ABI, what the Python wrapper refuses before anything
reaches the library, and which of the two symbols it calls."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import common
from pota_amd import _abi, capi
from test_trace_points_host import _from_c

SYMBOL = "lentil_hip_list_draws_spectral"


def test_the_symbol_is_declared_and_exported():
    lib = capi.load_library()
    txt = open(os.path.join(common.ROOT, "include", "lentil_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"int\s+lentil_hip_list_draws_spectral\s*\(\s*lentil_hip_ctx\s*\*ctx,\s*const\s+lentil_draw_list\s*\*list,"
                     r"\s*const\s+double\s*\*lambdas\s*\)\s*;", txt)
    assert hasattr(lib, SYMBOL), "liblentil_hip.so does not export %s" % SYMBOL
    assert SYMBOL in capi.EXPORTS
    # no context: an error, not a crash -- and no GPU is needed to say so
    assert lib.lentil_hip_list_draws_spectral(None, None, None) == _abi.ERR_INVALID


def test_the_abi_is_the_one_it_was():
    """an addition only: version 1, and the list's two structs keep their sizes"""
    assert capi.load_library().lentil_hip_abi_version() == 1
    got = _from_c('  printf("%d %zu %zu\\n", (int)LENTIL_ABI_VERSION, sizeof(lentil_draw_list), sizeof(lentil_draw));')
    assert got == [1, 64, 32]
    assert (C.sizeof(_abi.DrawList), np.dtype(_abi.Draw).itemsize) == (64, 32)


class _NoLibrary:
    """stands where the library does: a wrapper that gets as far as calling it has not refused"""

    def __getattr__(self, name):
        raise AssertionError("the wrapper called %s" % name)


def _ctx(lib):
    ctx = object.__new__(capi.Context)          # no lentil_hip_create: no GPU
    ctx.lib, ctx.h, ctx.device = lib, C.c_void_p(), 0
    return ctx


def test_the_wrapper_refuses_a_wrong_lambdas_array():
    import torch
    ctx = _ctx(_NoLibrary())
    try:
        call = lambda lam, **kw: ctx.list_draws(3, 5, capacity=8, lambdas=lam, **kw)      # noqa: E731
        for bad in (np.zeros(4), np.zeros(6), np.zeros((5, 1)),            # the wrong length or shape
                    np.zeros(5, np.float32), np.zeros(5, np.int64),        # the wrong dtype
                    torch.zeros(5, dtype=torch.float64)):                  # a tensor beside numpy records
            with pytest.raises(ValueError, match="lambdas"):
                call(bad)
        with pytest.raises(ValueError, match=r"one per visit"):
            call(np.zeros(4))
        # device=True: numpy beside a tensor of records, a tensor that is not on the context's GPU, the wrong dtype
        for bad in (np.zeros(5), torch.zeros(5, dtype=torch.float64), torch.zeros(5, dtype=torch.float32)):
            with pytest.raises(ValueError, match="lambdas"):
                call(bad, device=True)
        with pytest.raises(AssertionError, match="lentil_hip_list_draws_spectral"):      # a right one goes through to the library
            call(np.zeros(5))
        with pytest.raises(AssertionError, match="lentil_hip_list_draws$"):              # none: the scalar symbol
            ctx.list_draws(3, 5, capacity=8)
        # the other spectral calls keep their wording
        with pytest.raises(ValueError, match="one per ray"):
            capi._lambdas_arg("camera_rays", np.zeros(4), 5, None)
        with pytest.raises(ValueError, match="one per point"):
            capi._lambdas_arg("trace_points", np.zeros(4), 5, None)
    finally:
        ctx.h = C.c_void_p()                        # (nothing for __del__ to destroy)


class _Recorder:
    """stands where the library stands: keeps what every call was given and answers `n_draws` records"""

    def __init__(self, n_draws):
        self.calls, self.n_draws = [], n_draws

    def _answer(self, symbol, ref, lambdas):
        b = ref._obj
        self.calls.append((symbol, int(b.first_visit), int(b.n_visits), int(b.flags), int(b.capacity), float(b.lam), lambdas))
        b.n_draws[0] = self.n_draws
        if b.attempts:
            b.attempts[0] = 7
        return _abi.OK

    def lentil_hip_list_draws(self, h, ref):
        return self._answer("scalar", ref, None)

    def lentil_hip_list_draws_spectral(self, h, ref, lambdas):
        return self._answer("spectral", ref, lambdas)


def test_lambdas_choose_the_symbol_and_nothing_else():
    lam = np.array([0.45, 0.0, 0.65, 0.55, 0.5])
    ctx = _ctx(_Recorder(3))
    try:
        ctx.plan_visits = lambda first, n: (None, (n, n, 5))             # totals[2] = 5
        rec, n_draws, attempts = ctx.list_draws(3, 5, capacity=8, lam=0.5, probed=True, lambdas=lam)
        assert rec.shape == (3,) and (n_draws, attempts) == (3, 7)
        ctx.list_draws(3, 5, capacity=8, lam=0.5, probed=True)
        ctx.list_draws(3, 5, lambdas=lam)                                # capacity None: totals[2]
        ctx.list_draws(3, 0, lambdas=lam[:0])                            # an empty range: no pointer is handed over
        calls = ctx.lib.calls
        assert calls[0] == ("spectral", 3, 5, _abi.DRAWS_PROBED, 8, 0.5, lam.ctypes.data)      # the caller's own float64 array
        assert calls[1] == ("scalar", 3, 5, _abi.DRAWS_PROBED, 8, 0.5, None)
        assert calls[2] == ("spectral", 3, 5, 0, 5, 0.0, lam.ctypes.data)
        assert calls[3] == ("spectral", 3, 0, 0, 0, 0.0, None)
        # the channel list's counting call takes the wavelengths too
        ctx.lib.calls.clear()
        ctx.list_draws(3, 5, channels=True, lambdas=lam)
        assert ctx.lib.calls == [("spectral", 3, 5, _abi.DRAWS_CHANNELS, 0, 0.0, lam.ctypes.data),
                                 ("spectral", 3, 5, _abi.DRAWS_CHANNELS, 3, 0.0, lam.ctypes.data)]
    finally:
        ctx.h = C.c_void_p()
