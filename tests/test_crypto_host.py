"""lentil_hip_debug_last_crypto without a GPU: the symbol is exported and bound, the kernel names are the header's, a null
context is refused and nothing is written for it, and the header compiles for a C99 caller.  (That a context reads four zeros
before its first pass with cryptomatte AOVs needs a context: tests/test_gpu_crypto_shapes.py.)"""
import ctypes as C
import os
import re
import subprocess

import common
from pota_amd import _abi, capi


def test_symbol_is_exported_and_bound():
    lib = capi.load_library()
    assert "lentil_hip_debug_last_crypto" in capi.EXPORTS
    fn = lib.lentil_hip_debug_last_crypto
    assert fn.argtypes is not None and fn.restype is not None
    assert hasattr(capi.Context, "debug_last_crypto")


def test_a_null_context_is_refused_and_the_zeros_stay():
    lib = capi.load_library()
    out = (C.c_uint32 * 4)()
    assert lib.lentil_hip_debug_last_crypto(None, out) == _abi.ERR_INVALID
    assert tuple(out) == (0, 0, 0, 0)


def test_kernel_names_are_the_headers():
    with open(os.path.join(common.ROOT, "include", "lentil_hip.h")) as f:
        text = f.read()
    names = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"LENTIL_CRYPTO_DIRECT_(\w+) = (\d+)", text))
    assert names == {"ATOMIC": capi.CRYPTO_DIRECT_ATOMIC, "OWNER": capi.CRYPTO_DIRECT_OWNER, "TILE": capi.CRYPTO_DIRECT_TILE}
    assert (capi.CRYPTO_DIRECT_ATOMIC, capi.CRYPTO_DIRECT_OWNER, capi.CRYPTO_DIRECT_TILE) == (1, 2, 3)


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "last_crypto.c"
    src.write_text('#include "lentil_hip.h"\n'
                   "int tiled(lentil_hip_ctx *ctx) {\n"
                   "  uint32_t out[4];\n"
                   "  int rc = lentil_hip_debug_last_crypto(ctx, out);\n"
                   "  return rc ? rc : (out[0] == LENTIL_CRYPTO_DIRECT_TILE && out[1] != LENTIL_CRYPTO_DIRECT_OWNER - 2u && out[0] != LENTIL_CRYPTO_DIRECT_ATOMIC);\n"
                   "}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(common.ROOT, "include"),
                           "-c", str(src), "-o", str(tmp_path / "last_crypto.o")])
