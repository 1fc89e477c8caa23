"""Forward camera rays in batches (lentil_hip_camera_rays), the parts that need no GPU: the declaration, the layout of the
ctypes mirror of lentil_camera_ray_batch against the header (compiled here), and the per-ray xor128 seeding rule as
pota_amd.capi documents it against tea<8> of the oracle."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np

import common
from pota_amd import _abi, capi


def test_header_declares_camera_rays():
    txt = open(os.path.join(common.ROOT, "include", "lentil_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+lentil_hip_camera_rays\s*\(\s*lentil_hip_ctx\s*\*\s*\w+\s*,\s*const\s+lentil_camera_ray_batch\s*\*\s*\w+\s*\)\s*;", txt)
    assert "lentil_hip_camera_rays" in capi.EXPORTS
    assert hasattr(capi.load_library(), "lentil_hip_camera_rays")
    assert capi.load_library().lentil_hip_abi_version() == 1          # the call is an addition: the ABI version stays


def test_batch_struct_matches_the_header():
    fields = ["n", "first_ray", "in", "out", "tries", "lambda", "exposure", "rng_seed", "flags"]
    mine = ["n", "first_ray", "inp", "out", "tries", "lam", "exposure", "rng_seed", "flags"]
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"lentil_hip.h\"\nint main(void) {\n"
    src += '  printf("%zu", sizeof(lentil_camera_ray_batch));\n'
    for f in fields:
        src += '  printf(" %%zu", offsetof(lentil_camera_ray_batch, %s));\n' % f
    src += '  printf(" %u %u\\n", LENTIL_RAYS_DEVICE_POINTERS, LENTIL_RAYS_NO_DIFFERENTIALS);\n  return 0;\n}\n'
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(common.ROOT, "include"), c, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    want = [C.sizeof(_abi.CameraRayBatch)] + [getattr(_abi.CameraRayBatch, f).offset for f in mine]
    assert got[:-2] == want
    assert got[-2:] == [_abi.RAYS_DEVICE_POINTERS, _abi.RAYS_NO_DIFFERENTIALS]
    assert (_abi.RAY_IN_FLOATS, _abi.RAY_OUT_FLOATS) == (6, 21)


def test_ray_seeding_rule(orc):
    """w0 = tea8(id, seed), w_k = tea8(id, w_{k-1}); all zero -> xor128's initial constants"""
    rng = np.random.default_rng(11)
    ids = np.concatenate([np.array([0, 1, 63, 64, 0xFFFFFFFF], np.uint64), rng.integers(0, 1 << 32, 200, dtype=np.uint64)]).astype(np.uint32)
    for seed in (0, 1, 0xDEADBEEF):
        got = capi.ray_rng_state(ids, seed)
        assert got.shape == (ids.size, 4) and got.dtype == np.uint32
        for k, rid in enumerate(ids):
            w, want = seed, []
            for _ in range(4):
                w = orc.orc_tea8(int(rid), w)
                want.append(w)
            if not any(want):
                st = (C.c_uint32 * 4)()
                orc.orc_xor128_init(st)
                want = list(st)
            assert [int(x) for x in got[k]] == want
    assert [int(x) for x in capi.ray_rng_state(7, 3)] == [int(x) for x in capi.ray_rng_state(np.array([7]), 3)[0]]
