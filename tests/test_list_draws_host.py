"""lentil_hip_plan_visits / lentil_hip_list_draws without a GPU: the symbols, the layout of the two records and of
lentil_draw_list, the constants."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np

import common
from pota_amd import _abi, capi

PLAN_FIELDS = ["cs", "add_energy", "weight", "samples", "pixel", "flags"]
DRAW_FIELDS = ["visit", "attempt", "pixel", "tries", "xy"]
LIST_FIELDS = ["first_visit", "n_visits", "flags", "capacity", "out", "lambda", "n_draws", "attempts"]


def test_the_symbols_are_exported_and_bound():
    lib = capi.load_library()
    for n in ("lentil_hip_plan_visits", "lentil_hip_list_draws", "lentil_hip_list_draws_path"):
        assert hasattr(lib, n), "liblentil_hip.so does not export %s" % n
        assert n in capi.EXPORTS
    assert hasattr(lib, "lentil_hip_trace_points")                     # (what the position parity is taken against)
    for m in ("plan_visits", "list_draws", "list_draws_path"):
        assert callable(getattr(capi.Context, m))
    assert lib.lentil_hip_abi_version() == 1
    # no context: an error, not a crash -- and no GPU is needed to say so
    assert lib.lentil_hip_plan_visits(None, 0, 0, None, 0, None) == _abi.ERR_INVALID
    assert lib.lentil_hip_list_draws(None, None) == _abi.ERR_INVALID
    assert lib.lentil_hip_list_draws_path(None, None) == _abi.ERR_INVALID


def _from_c(body):
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "lentil_hip.h"\nint main(void) {\n%s\n  return 0;\n}\n' % body
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(common.ROOT, "include"), c, "-o", exe])
        return [int(v) for v in subprocess.check_output([exe]).split()]


def _layout(struct, fields):
    return _from_c('  printf("%%zu\\n", sizeof(%s));\n' % struct + "".join(
        '  printf("%%zu\\n", offsetof(%s, %s));\n' % (struct, f) for f in fields))


def _declared(struct):
    txt = open(os.path.join(common.ROOT, "include", "lentil_hip.h")).read()
    decl = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), txt, re.S).group(1)
    decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    return [re.sub(r"\[\d+\]", "", m) for m in re.findall(r"(\w+(?:\[\d+\])?)\s*[;,]", decl)]


def test_both_records_are_32_bytes_with_the_documented_offsets():
    assert _layout("lentil_visit_plan", PLAN_FIELDS) == [32, 0, 12, 16, 20, 24, 28]
    assert _layout("lentil_draw", DRAW_FIELDS) == [32, 0, 4, 8, 12, 16]
    for dt, fields, offs in ((_abi.VisitPlan, PLAN_FIELDS, [0, 12, 16, 20, 24, 28]), (_abi.Draw, DRAW_FIELDS, [0, 4, 8, 12, 16])):
        assert dt.itemsize == 32 and list(dt.names) == fields
        assert [dt.fields[f][1] for f in fields] == offs
    assert _abi.VisitPlan["cs"].shape == (3,) and _abi.VisitPlan["cs"].base == np.float32
    assert _abi.VisitPlan["samples"] == np.uint32 and _abi.VisitPlan["weight"] == np.float32
    assert _abi.Draw["xy"].shape == (2,) and _abi.Draw["xy"].base == np.float64 and _abi.Draw["tries"] == np.int32
    assert _declared("lentil_visit_plan") == PLAN_FIELDS and _declared("lentil_draw") == DRAW_FIELDS


def test_draw_list_layout_matches_the_header():
    got = _layout("lentil_draw_list", LIST_FIELDS)
    names = ["lam" if f == "lambda" else f for f in LIST_FIELDS]
    assert got == [C.sizeof(_abi.DrawList)] + [getattr(_abi.DrawList, f).offset for f in names]
    assert [n for n, _ in _abi.DrawList._fields_] == names
    assert _declared("lentil_draw_list") == LIST_FIELDS


def test_the_constants_match_the_header():
    got = _from_c('  printf("%u %u %u\\n", (unsigned)LENTIL_PLAN_DEVICE_POINTERS, (unsigned)LENTIL_PLAN_REDISTRIBUTE, (unsigned)LENTIL_DRAWS_DEVICE_POINTERS);')
    assert got == [_abi.PLAN_DEVICE_POINTERS, _abi.PLAN_REDISTRIBUTE, _abi.DRAWS_DEVICE_POINTERS] == [1, 1, 1]
    assert (_abi.DRAWS_PATH_THIN_LENS, _abi.DRAWS_PATH_INTERPRETER, _abi.DRAWS_PATH_COMPILED_IN) == (0, 1, 2)
