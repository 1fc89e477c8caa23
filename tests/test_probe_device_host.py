"""The device occlusion callback's interface without a GPU: the three symbols are exported and bound, the ABI version has not
moved, and the header's types fit together for a C99 caller."""
import os
import subprocess

import common
from pota_amd import capi

NAMES = ["lentil_hip_set_occlusion_probe_device", "lentil_hip_probe_device_stats", "lentil_hip_test_sphere_occluder_device"]


def test_symbols_are_exported_and_bound():
    lib = capi.load_library()
    for name in NAMES:
        assert name in capi.EXPORTS
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is not None
    assert capi.sphere_occluder_device()
    assert hasattr(capi.Context, "set_occlusion_probe_device") and hasattr(capi.Context, "probe_device_stats")


def test_abi_version_stays_1():
    assert capi.load_library().lentil_hip_abi_version() == 1


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "probe_device.c"
    src.write_text('#include "lentil_hip.h"\n'
                   "lentil_probe_device_fn the_sphere = lentil_hip_test_sphere_occluder_device;\n"
                   "int set(lentil_hip_ctx *ctx, void *user) {\n"
                   "  uint64_t stats[4];\n"
                   "  int rc = lentil_hip_set_occlusion_probe_device(ctx, the_sphere, user, (const float *)0);\n"
                   "  return rc ? rc : lentil_hip_probe_device_stats(ctx, stats);\n"
                   "}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(common.ROOT, "include"),
                           "-c", str(src), "-o", str(tmp_path / "probe_device.o")])
