"""The lens's forward members -- eval_fw_newton (one Newton step of lens_pt_sample_aperture) and eval_out (lens_evaluate's
four outer-pupil polynomials) -- as the two emitters write them, without a GPU: the C++ emitter of csrc/lentil_lens_jit.h
writes, for the two shipped tables, what tools/gen_lens_code.py writes (and the headers under csrc/generated/ are what the
generator writes today), and the run-time unit -- four solve kernels and the camera-rays kernel -- compiles for a table that
is not built in."""
import importlib.util
import os
import re

import pytest

import common
from pota_amd import capi, lens_io

GEN = os.path.join(common.ROOT, "pota_amd", "csrc", "generated")
SHIPPED = ["double_gauss_50mm", "petzval_58mm"]


def _member(src, name):
    """the text of one static member, from its declaration to the line that closes its body"""
    a = src.index("static __device__ __forceinline__ void %s(" % name)
    b = src.index("\n  }\n", a)
    return src[a:b]


def _coefficients(src):
    a = src.index("__device__ __constant__ double kCoef")
    b = src.index("};", a)
    return [float.fromhex(x) for x in re.findall(r"-?0x[0-9a-f.]+p[+-]\d+", src[a:b])]


@pytest.fixture(scope="module")
def generated(tmp_path_factory):
    """tools/gen_lens_code.py run into a scratch directory: {lens: header text}"""
    spec = importlib.util.spec_from_file_location("gen_lens_code", os.path.join(common.ROOT, "tools", "gen_lens_code.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    gen.OUT_DIR = str(tmp_path_factory.mktemp("generated"))
    out = {}
    for lens in SHIPPED:
        gen.gen_lens(lens, lens_io.load_lens_json(lens))
        with open(os.path.join(gen.OUT_DIR, "lens_%s.h" % lens)) as f:
            out[lens] = f.read()
    return out


@pytest.mark.parametrize("lens", SHIPPED)
def test_emitter_writes_the_generators_forward_members(generated, lens):
    table, keep = lens_io.make_lens_table(lens_io.load_lens_json(lens))
    rc, src, log, seconds, code_bytes = capi.lens_jit_compile(table, compile=False)
    assert rc == 0
    ref = generated[lens]
    assert _coefficients(src) == _coefficients(ref)          # backward and forward coefficients, one array, one order
    for name in ("eval_fw_newton", "eval_out"):
        mine, theirs = _member(src, name), _member(ref, name)
        assert "LENTIL_SLOAD8" in theirs and mine.replace("kCoef_rt", "K") == theirs.replace("kCoef_" + lens, "K"), name
    # every polynomial the forward step needs is written: 2 + 2 + 4 + 4 targets, and 4
    fw = _member(ref, "eval_fw_newton")
    for target in ["pred_ap[%d]" % i for i in range(2)] + ["pred_dir[%d]" % i for i in range(2)] + ["Jap[%d]" % i for i in range(4)] + [
            "Jappos[%d]" % i for i in range(4)]:
        assert "\n  %s = " % target in fw, target
    for i in range(4):
        assert "\n  out[%d] = " % i in _member(ref, "eval_out")


@pytest.mark.parametrize("lens", SHIPPED)
def test_committed_headers_are_what_the_generator_writes(generated, lens):
    with open(os.path.join(GEN, "lens_%s.h" % lens)) as f:
        assert f.read() == generated[lens]


def test_run_time_unit_with_the_camera_rays_kernel_compiles():
    """anamorphic_petzval_58mm: no kernel of it is built in.  hiprtc cross-compiles for gfx950 without a GPU."""
    table, keep = lens_io.make_lens_table(lens_io.load_lens_json("anamorphic_petzval_58mm"))
    rc, src, log, seconds, code_bytes = capi.lens_jit_compile(table, compile=True)
    assert rc == 0, log[:2000]
    print("run-time unit: %.1f s, %d bytes" % (seconds, code_bytes))
    assert "eval_fw_newton" in src and "eval_out" in src and code_bytes > 100000 and seconds < 180
