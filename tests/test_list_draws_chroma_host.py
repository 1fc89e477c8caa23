"""LENTIL_DRAWS_CHANNELS and lentil_hip_draw_channels without a GPU: the constant, the symbol, the channels of a parameter set
against the reference's fp32 arithmetic restated in numpy, and the Python wrapper's flag."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import common
from pota_amd import _abi, capi


def _from_c(body):
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "lentil_hip.h"\nint main(void) {\n%s\n  return 0;\n}\n' % body
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(common.ROOT, "include"), c, "-o", exe])
        return [int(v) for v in subprocess.check_output([exe]).split()]


def test_the_constant_matches_the_header():
    got = _from_c('  printf("%u %u %u\\n", (unsigned)LENTIL_DRAWS_DEVICE_POINTERS, (unsigned)LENTIL_DRAWS_PROBED, (unsigned)LENTIL_DRAWS_CHANNELS);')
    assert got == [_abi.DRAWS_DEVICE_POINTERS, _abi.DRAWS_PROBED, _abi.DRAWS_CHANNELS] == [1, 2, 4]


def test_the_symbol_is_exported_and_bound():
    lib = capi.load_library()
    assert hasattr(lib, "lentil_hip_draw_channels") and "lentil_hip_draw_channels" in capi.EXPORTS
    assert callable(capi.draw_channels)
    assert lib.lentil_hip_abi_version() == 1
    n, lam = C.c_uint32(), (C.c_double * 3)()
    assert lib.lentil_hip_draw_channels(None, C.byref(n), lam, None) == _abi.ERR_INVALID
    p = common.po_setup(48, 32)[0]
    assert lib.lentil_hip_draw_channels(C.byref(p), None, lam, None) == _abi.ERR_INVALID
    assert lib.lentil_hip_draw_channels(C.byref(p), C.byref(n), None, None) == _abi.ERR_INVALID
    assert lib.lentil_hip_draw_channels(C.byref(p), C.byref(n), lam, None) == _abi.OK and n.value == 1      # the weights are optional


def _want(c, lambda_bw):
    """src/lentil_filter.cpp:254-268 with linear_interpolate (src/global.h:3-5) in fp32: lerpf(1 - c, 0.35, 0.55), 0.55,
    lerpf(c, 0.55, 0.85), the argument 1.0 - c formed in double and rounded to float"""
    f = np.float32
    if c > 0:
        c = f(c)
        p0 = f(np.float64(1.0) - np.float64(c))
        lam = [f(0.35) + p0 * (f(0.55) - f(0.35)), f(0.55), f(0.55) + c * (f(0.85) - f(0.55))]
        assert all(x.dtype == np.float32 for x in lam)
        return np.array(lam, np.float64), 3.0 * np.eye(3, dtype=np.float32)
    return np.full(3, np.float64(f(lambda_bw))), np.ones((3, 3), np.float32)


@pytest.mark.parametrize("c", [0.0, 0.5, 1.0, -0.5])
def test_polynomial_optics_channels(c):
    p = common.po_setup(48, 32, abb_chromatic=c)[0]
    n, lam, w = capi.draw_channels(p)
    want_lam, want_w = _want(c, p.lambda_bw)
    assert n == (3 if c != 0 else 1)
    assert lam.dtype == np.float64 and np.array_equal(lam.view(np.uint64), want_lam.view(np.uint64))
    assert w.dtype == np.float32 and np.array_equal(w, want_w)
    if c > 0:
        assert lam[0] < lam[1] < lam[2] and np.float32(0.35) <= lam[0] and lam[2] <= np.float32(0.85)


@pytest.mark.parametrize("c", [0.0, 0.6, -0.5])
def test_the_thin_lens_has_one_white_channel(c):
    p = common.tl_setup(48, 32, abb_chromatic=c)
    n, lam, w = capi.draw_channels(p)
    assert n == 1 and np.array_equal(lam, np.full(3, np.float64(np.float32(p.lambda_bw)))) and np.array_equal(w, np.ones((3, 3), np.float32))


def test_another_lambda_bw_is_passed_through():
    p = common.po_setup(48, 32, abb_chromatic=-0.25)[0]
    p.lambda_bw = 0.45
    n, lam, w = capi.draw_channels(p)
    assert n == 3 and np.array_equal(lam, np.full(3, np.float64(np.float32(0.45)))) and (w == 1).all()


class _Recorder:
    """stands where the library stands: keeps the lentil_draw_list of every call and answers `n_draws` records"""

    def __init__(self, n_draws):
        self.calls, self.n_draws = [], n_draws

    def lentil_hip_list_draws(self, h, ref):
        b = ref._obj
        self.calls.append((int(b.flags), int(b.capacity), float(b.lam)))
        b.n_draws[0] = self.n_draws
        if b.attempts:
            b.attempts[0] = 7
        return _abi.OK


def _wrapper(n_draws):
    ctx = capi.Context.__new__(capi.Context)
    ctx.lib, ctx.h, ctx.device = _Recorder(n_draws), None, 0
    ctx.plan_visits = lambda first, n: (None, (n, n, 5))             # totals[2] = 5
    return ctx


def test_the_channels_argument_sets_the_flag():
    ctx = _wrapper(3)
    rec, n_draws, attempts = ctx.list_draws(0, 10, capacity=8)
    assert ctx.lib.calls == [(0, 8, 0.0)] and rec.shape == (3,) and (n_draws, attempts) == (3, 7)
    ctx = _wrapper(3)
    ctx.list_draws(0, 10, capacity=8, channels=True)
    assert ctx.lib.calls == [(_abi.DRAWS_CHANNELS, 8, 0.0)]
    ctx = _wrapper(3)
    ctx.list_draws(0, 10, capacity=8, channels=True, probed=True, lam=0.5)
    assert ctx.lib.calls == [(_abi.DRAWS_CHANNELS | _abi.DRAWS_PROBED, 8, 0.5)]


def test_without_a_capacity_the_channel_list_is_sized_by_a_counting_call():
    ctx = _wrapper(40)                                               # more than totals[2]
    rec, n_draws, attempts = ctx.list_draws(0, 10, channels=True)
    assert ctx.lib.calls == [(_abi.DRAWS_CHANNELS, 0, 0.0), (_abi.DRAWS_CHANNELS, 40, 0.0)]
    assert rec.shape == (40,) and n_draws == 40
    ctx = _wrapper(3)                                                # the plain list: totals[2], one call
    ctx.list_draws(0, 10)
    assert ctx.lib.calls == [(0, 5, 0.0)]
