"""lentil_hip_trace_points_probed without a GPU: the symbol, lentil_point_probe's layout against its ctypes mirror, the
unchanged ABI, and what the Python wrapper refuses before anything reaches the library."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import common
from pota_amd import _abi, capi
from test_spectral_host import _ctx
from test_trace_points_host import _from_c

FIELDS = ["origin", "time", "exempt", "lambdas"]


def test_the_symbol_is_declared_and_exported():
    lib = capi.load_library()
    txt = open(os.path.join(common.ROOT, "include", "lentil_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"int\s+lentil_hip_trace_points_probed\s*\(\s*lentil_hip_ctx\s*\*ctx,\s*const\s+lentil_point_batch\s*\*batch,"
                     r"\s*const\s+lentil_point_probe\s*\*probe\s*\)\s*;", txt)
    assert hasattr(lib, "lentil_hip_trace_points_probed") and "lentil_hip_trace_points_probed" in capi.EXPORTS
    # no context: an error, not a crash -- and no GPU is needed to say so
    assert lib.lentil_hip_trace_points_probed(None, None, None) == _abi.ERR_INVALID


def test_point_probe_layout_matches_the_header():
    body = '  printf("%zu\\n", sizeof(lentil_point_probe));\n' + "".join(
        '  printf("%%zu\\n", offsetof(lentil_point_probe, %s));\n' % f for f in FIELDS)
    got = _from_c(body)
    assert got == [C.sizeof(_abi.PointProbe)] + [getattr(_abi.PointProbe, f).offset for f in FIELDS] == [32, 0, 8, 16, 24]
    assert [n for n, _ in _abi.PointProbe._fields_] == FIELDS
    txt = open(os.path.join(common.ROOT, "include", "lentil_hip.h")).read()
    decl = re.search(r"typedef struct lentil_point_probe \{(.*?)\} lentil_point_probe;", txt, re.S).group(1)
    decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    assert re.findall(r"(\w+)\s*;", decl) == FIELDS


def test_the_abi_is_the_one_it_was():
    assert capi.load_library().lentil_hip_abi_version() == 1
    got = _from_c('  printf("%d %zu\\n", (int)LENTIL_ABI_VERSION, sizeof(lentil_point_batch));')
    assert got == [1, 80] and C.sizeof(_abi.PointBatch) == 80


def test_the_wrapper_has_the_signature_of_the_issue():
    names = list(inspect.signature(capi.Context.trace_points_probed).parameters)
    assert names == ["self", "cs", "pixel", "attempts", "origin", "first_attempt", "time", "exempt", "lam", "lambdas", "want_xy",
                     "want_sensor", "want_tries"]


def test_the_wrapper_refuses_mismatched_kinds_and_shapes():
    import torch
    ctx = _ctx()
    try:
        n = 5
        cs, pixel, origin = np.zeros((n, 3), np.float32), np.zeros(n, np.uint32), np.zeros((n, 3), np.float32)
        call = lambda **kw: ctx.trace_points_probed(**dict(dict(cs=cs, pixel=pixel, attempts=2, origin=origin), **kw))      # noqa: E731
        bad = [dict(origin=np.zeros((n, 2), np.float32)), dict(origin=np.zeros((n + 1, 3), np.float32)), dict(origin=None),
               dict(cs=np.zeros((n, 2), np.float32)), dict(pixel=np.zeros(n + 1, np.uint32)), dict(first_attempt=np.zeros(n - 1, np.uint32)),
               dict(time=np.zeros(n + 1, np.float32)), dict(time=np.zeros((n, 1), np.float32)), dict(exempt=np.zeros(n - 1, np.uint8)),
               dict(lambdas=np.zeros(n + 1)), dict(lambdas=np.zeros(n, np.float32)),
               # tensors beside numpy arrays
               dict(origin=torch.zeros((n, 3))), dict(time=torch.zeros(n)), dict(exempt=torch.zeros(n, dtype=torch.uint8)),
               dict(pixel=torch.zeros(n, dtype=torch.int32)), dict(lambdas=torch.zeros(n, dtype=torch.float64)),
               # numpy arrays beside a tensor, and a tensor that is not on the context's GPU
               dict(cs=torch.zeros((n, 3))), dict(cs=torch.zeros((n, 3)), origin=torch.zeros((n, 3)), pixel=torch.zeros(n, dtype=torch.int32))]
        for kw in bad:
            with pytest.raises(ValueError, match="trace_points"):
                call(**kw)
        with pytest.raises(AssertionError, match="lentil_hip_trace_points_probed"):      # a right one goes through to the library
            call(time=np.zeros(n, np.float32), exempt=np.zeros(n, np.uint8), lambdas=np.zeros(n))
    finally:
        ctx.h = C.c_void_p()                        # (nothing for __del__ to destroy)
