"""lentil_hip_trace_points without a GPU: the symbols, the layout of lentil_point_batch, the two codes."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import common
from pota_amd import _abi, capi

FIELDS = ["n_points", "attempts", "flags", "cs", "pixel", "first_attempt", "lambda", "out_pixel", "out_xy", "out_sensor", "out_tries"]


def test_both_symbols_are_exported():
    lib = capi.load_library()
    for n in ("lentil_hip_trace_points", "lentil_hip_trace_points_path"):
        assert hasattr(lib, n), "liblentil_hip.so does not export %s" % n
        assert n in capi.EXPORTS
    assert lib.lentil_hip_abi_version() == 1
    # no context: an error, not a crash -- and no GPU is needed to say so
    assert lib.lentil_hip_trace_points(None, None) == _abi.ERR_INVALID
    assert lib.lentil_hip_trace_points_path(None, None) == _abi.ERR_INVALID


def _from_c(body):
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "lentil_hip.h"\nint main(void) {\n%s\n  return 0;\n}\n' % body
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(common.ROOT, "include"), c, "-o", exe])
        return [int(v) for v in subprocess.check_output([exe]).split()]


def test_point_batch_layout_matches_the_header():
    """sizeof and every offsetof of the ctypes mirror vs the C struct (compiled here with gcc)"""
    body = '  printf("%zu\\n", sizeof(lentil_point_batch));\n' + "".join(
        '  printf("%%zu\\n", offsetof(lentil_point_batch, %s));\n' % f for f in FIELDS)
    got = _from_c(body)
    mine = [C.sizeof(_abi.PointBatch)] + [getattr(_abi.PointBatch, "lam" if f == "lambda" else f).offset for f in FIELDS]
    assert got == mine
    assert [n for n, _ in _abi.PointBatch._fields_] == ["lam" if f == "lambda" else f for f in FIELDS]
    # the header declares exactly these members, in this order
    txt = open(os.path.join(common.ROOT, "include", "lentil_hip.h")).read()
    decl = re.search(r"typedef struct lentil_point_batch \{(.*?)\} lentil_point_batch;", txt, re.S).group(1)
    decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    assert re.findall(r"(\w+)\s*;", decl) == FIELDS


def test_the_constants_match_the_header():
    got = _from_c('  printf("%u %u %u\\n", (unsigned)LENTIL_POINTS_DEVICE_POINTERS, (unsigned)LENTIL_POINT_VIGNETTED, (unsigned)LENTIL_POINT_OUTSIDE);')
    assert got == [_abi.POINTS_DEVICE_POINTERS, _abi.POINT_VIGNETTED, _abi.POINT_OUTSIDE] == [1, 0xFFFFFFFF, 0xFFFFFFFE]
    assert (_abi.POINTS_PATH_THIN_LENS, _abi.POINTS_PATH_INTERPRETER, _abi.POINTS_PATH_COMPILED_IN) == (0, 1, 2)
