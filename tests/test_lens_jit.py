"""Run-time lens specialisation (pota_amd/csrc/lentil_lens_jit.h): the emitter and the compilation, without a GPU.

The reference compiles every lens into the plugin (include/auto_generated_lens_includes/load_lt_sample_aperture.h:4-47,
src/lentil.h:1308); the library emits and compiles a lens's straight-line code at run time for any table that has no kernel
built in.  Here: the C++ emitter writes, for the two shipped lenses, exactly what tools/gen_lens_code.py wrote into
csrc/generated/ (whose kernels the GPU suite checks bit for bit against the interpreter and the oracle), and hiprtc compiles
the four solve kernels for a table that is NOT built in.  tests/test_gpu_lens_jit.py runs them.

The same two checks over the generated tables of tests/lens_tables.py (exponents up to 15, wavelength powers up to 15, polynomials
of one to four terms and of none, 1536 packed terms), which reach the emitter branches no shipped table does;
tests/test_gpu_lens_tables.py runs those kernels.
"""
import concurrent.futures
import importlib.util
import os
import re
import time

import pytest

import common
import lens_tables
from pota_amd import capi, lens_io

GEN = os.path.join(common.ROOT, "pota_amd", "csrc", "generated")


def _coefficients(src):
    a = src.index("__device__ __constant__ double kCoef")
    b = src.index("};", a)
    return [float.fromhex(x) for x in re.findall(r"-?0x[0-9a-f.]+p[+-]\d+", src[a:b])]


def _functions(src, name):
    a = src.index("static __device__ __forceinline__ void eval_bw")
    b = src.index("static __device__ __forceinline__ double transmittance")
    c = src.index("};", b)
    return src[a:b].replace(name, "K"), src[b:c].replace(name, "K")


@pytest.mark.parametrize("lens", ["double_gauss_50mm", "petzval_58mm"])
def test_emitter_writes_what_the_generator_wrote(lens):
    table, keep = lens_io.make_lens_table(lens_io.load_lens_json(lens))
    rc, src, log, seconds, code_bytes = capi.lens_jit_compile(table, compile=False)
    assert rc == 0
    with open(os.path.join(GEN, "lens_%s.h" % lens)) as f:
        ref = f.read()
    assert _coefficients(src) == _coefficients(ref)           # the same doubles in the same order (base terms and c * e derivatives)
    assert _functions(src, "kCoef_rt") == _functions(ref, "kCoef_" + lens)       # ... and the same operations on them, text for text


def test_a_table_that_is_not_built_in_compiles():
    """anamorphic_petzval_58mm (cylindrical outer pupil; BASELINE config 4's "anamorphic"): no kernel of it is built into the
    library.  hiprtc cross-compiles for gfx950 without a GPU; a machine without libhiprtc skips."""
    table, keep = lens_io.make_lens_table(lens_io.load_lens_json("anamorphic_petzval_58mm"))
    rc, src, log, seconds, code_bytes = capi.lens_jit_compile(table, compile=True)
    if rc != 0 and "hiprtc is not available" in log:
        pytest.skip("no libhiprtc on this machine")
    assert rc == 0, log[:2000]
    assert code_bytes > 100000 and "struct Lens_rt" in src and seconds < 120


# ---- the generated tables (tests/lens_tables.py) ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def generator(tmp_path_factory):
    """tools/gen_lens_code.py loaded in-process, writing into a scratch directory: spec -> header text"""
    spec = importlib.util.spec_from_file_location("gen_lens_code", os.path.join(common.ROOT, "tools", "gen_lens_code.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    gen.OUT_DIR = str(tmp_path_factory.mktemp("generated"))

    def run(ident, lens_spec):
        gen.gen_lens(ident, lens_spec)
        with open(os.path.join(gen.OUT_DIR, "lens_%s.h" % ident)) as f:
            return f.read()

    return run


@pytest.mark.parametrize("case", lens_tables.EMITTER_CASES)
def test_emitter_writes_what_the_generator_writes_for_a_generated_table(generator, case):
    """eval_bw, transmittance and the forward members text for text, the coefficients double for double -- on tables with
    powers the shipped ones never name (x_10 ... x_15, lp3 ... lp15), "0.0" targets, an empty transmittance and blocks of eight
    coefficients that touch up to eight polynomials"""
    table, keep = lens_tables.table(case)
    rc, src, log, seconds, code_bytes = capi.lens_jit_compile(table, compile=False)
    assert rc == 0
    ident = "case_" + case.replace("-", "_")
    ref = generator(ident, lens_tables.spec(case))
    assert _coefficients(src) == _coefficients(ref)
    assert [c.hex() for c in _coefficients(src)] == [c.hex() for c in _coefficients(ref)]      # (-0.0 is not 0.0)
    assert _functions(src, "kCoef_rt") == _functions(ref, "kCoef_" + ident)
    bw, rest = _functions(src, "kCoef_rt")
    if case in ("high-exponents", "all-fifteen", "full"):
        assert all("const double %s_15 = %s * %s_7 * %s_7;" % (v, v, v, v) in bw for v in ("x", "y", "dx", "dy"))
        assert "const double x_14 = x_7 * x_7;" in bw or case == "all-fifteen"
    if case in ("lambda-powers", "full"):
        assert all("const double lp%d = lp[%d];" % (e, e) in bw for e in range(3, 16)) and "lp[15]" in rest


@pytest.fixture(scope="module")
def compiled():
    """every case of EMITTER_CASES through hiprtc, started side by side (ctypes lets go of the interpreter lock): {case: (rc,
    source, log, seconds, code bytes)}.  hiprtc takes the compilations of a process one after the other all the same -- the
    seconds of a case include its wait for the ones before it"""
    tables = {case: lens_tables.table(case) for case in lens_tables.EMITTER_CASES}
    t0 = time.time()
    with concurrent.futures.ThreadPoolExecutor(max(1, min(len(tables), (os.cpu_count() or 2) - 1, 12))) as pool:
        jobs = {case: pool.submit(capi.lens_jit_compile, tables[case][0], True) for case in tables}
        out = {case: job.result() for case, job in jobs.items()}
    wall = time.time() - t0
    print("hiprtc, %d tables side by side: %.1f s; each: %s" % (len(out), wall, ", ".join("%s %.1f s / %d KB" % (c, r[3], r[4] >> 10)
                                                                                           for c, r in out.items())))
    return out


@pytest.mark.parametrize("case", lens_tables.EMITTER_CASES)
def test_a_generated_table_compiles(compiled, case):
    """The four solve kernels and the camera-rays kernel of every case.  Measured on an 8-CPU machine without a GPU: 8-12 s of
    one CPU per table (short-a, first through, 7.8 s; the 1536-term table about 12 s, 719 KB of code, the others 493-613 KB);
    the ten, started together, were through after 101 s -- one after the other, inside hiprtc.  A machine without libhiprtc
    skips, as above."""
    rc, src, log, seconds, code_bytes = compiled[case]
    if rc != 0 and "hiprtc is not available" in log:
        pytest.skip("no libhiprtc on this machine")
    assert rc == 0, log[:2000]
    assert code_bytes > 100000 and "struct Lens_rt" in src and seconds < 180
