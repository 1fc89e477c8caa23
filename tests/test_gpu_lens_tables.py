"""The lens paths on the generated tables of tests/lens_tables.py, against the oracle: exponents up to 15, wavelength powers
up to 15, polynomials of one to four terms and of none, permuted sums, 1536 packed terms -- and the two refusals.

Every lens test before this one ran on a shipped table (at most 48 terms a polynomial and 707 packed, no exponent above 9, no
wavelength exponent above 2).  Here, per table: the table interpreter (contexts created under LENTIL_LENS_JIT=0, so that no
compilation is started that the test would not wait for) through lt_sample_aperture, the backward trace, the focus search, the
camera rays, the traced points and the pass in its chunked and streamed forms; the cooperative straggler kernel; and the
kernels hiprtc compiles from the emitter's straight-line code, which one module-wide fixture compiles for all tables first.
The oracle's results are computed once per table (lens_tables keeps them) and never written to.
tests/test_lens_table_cases.py holds the tables to the oracle alone: none of the comparisons here is empty.

(lentil_hip_test_lt_sample_aperture has no output for the iteration count: the oracle's counts are what the straggler bar is
taken from, tests/test_lens_table_cases.py::test_stragglers_would_be_parked.)
"""
import ctypes as C
import time

import numpy as np
import pytest

import common
import lens_tables as lt
import oracle_lib
import trace_point_cases as tc
from pota_amd import _abi, capi
from test_gpu_camera_rays import LAM, _inputs, oracle_rays
from test_gpu_parity import check_frame, check_logs, gpu_run
from test_gpu_trace_points import _check_po

pytestmark = pytest.mark.gpu

N_TRACE, N_SHIFTS, N_RAYS, N_QUERIES, K_ATTEMPTS = 1024, 300, 515, 256, 4      # (515 rays: two blocks and a partial wave)
SEED = 0x1234


def _counts(c):
    return int(c.redistributed_visits), int(c.attempted_draws), int(c.accepted_draws)


@pytest.fixture
def interp(monkeypatch, gpu_ctx_factory):
    """name -> a context on the table's camera, created with the run-time compilation off (the switch is read at creation):
    a process that ends while a compiling thread is still at work can crash at exit"""
    monkeypatch.setenv("LENTIL_LENS_JIT", "0")

    def make(name, chroma=0.0):
        p, model, table, keep = lt.setup(name, chroma)
        ctx = gpu_ctx_factory()
        ctx.set_params(p)
        ctx.set_lens(table)
        assert not ctx.lens_is_compiled() and ctx.lens_jit_status()[0] == 0       # no kernel built in, none being compiled
        return ctx

    return make


# ---- the interpreter, per table ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", lt.RUN)
def test_lt_sample_aperture(orc, interp, name):
    """sensor, out and transmittance of every one of the 3 x 2000 solves, bit for bit (NaN-aware)"""
    want = lt.oracle_aperture(orc, name)
    scene, ap = lt.sample_points(name)
    ctx = interp(name)
    for k, lam in enumerate(lt.LAMBDAS):
        sensor, out, T = ctx.test_lt_sample_aperture(scene, ap, lam)
        assert np.array_equal(T, want["T"][k], equal_nan=True), (name, lam)
        assert np.array_equal(sensor, want["sensor"][k], equal_nan=True), (name, lam)
        assert np.array_equal(out, want["out"][k], equal_nan=True), (name, lam)


_traced = {}


def _oracle_trace_bw(orc, name):
    if name not in _traced:
        p, model, table, keep = lt.setup(name)
        rng = np.random.default_rng(3)
        n = N_TRACE
        target = np.stack([rng.uniform(-600, 600, n), rng.uniform(-400, 400, n), rng.uniform(500, 5000, n)], 1)
        px, py = rng.integers(0, lt.W, n).astype(np.int32), rng.integers(0, lt.H, n).astype(np.int32)
        att = rng.integers(0, 3000, n).astype(np.int32)
        lens = orc.orc_lens_create(C.byref(table))
        exy, eok = np.zeros((n, 2)), np.zeros(n, np.int32)
        sp = (C.c_double * 2)()
        for i in range(n):
            eok[i] = orc.orc_trace_ray_bw_po(C.byref(p), lens, None, oracle_lib.darr(*target[i]), sp, int(px[i]), int(py[i]), int(att[i]),
                                             p.lambda_bw, None)
            if eok[i]:
                exy[i] = sp[0], sp[1]
        orc.orc_lens_destroy(lens)
        _traced[name] = (target, px, py, att, exy, eok)
    return _traced[name]


@pytest.mark.parametrize("name", lt.RUN)
def test_trace_bw_po(orc, interp, name):
    target, px, py, att, exy, eok = _oracle_trace_bw(orc, name)
    if lt.BY_NAME[name]["min_draws"] >= lt.MIN_DRAWS:
        assert eok.mean() > 0.3
    xy, ok = interp(name).test_trace_bw_po(target, px, py, att)
    assert np.array_equal(ok, eok)
    assert np.array_equal(xy[ok == 1], exy[ok == 1])


def _oracle_chain(orc, lens, table, shift, lam):
    """camera_get_y0_intersection_distance step by step in the oracle (tests/test_gpu_focus.py)"""
    sensor = (C.c_double * 5)(0, 0, 0, 0, lam)
    ap = (C.c_double * 5)(0, float(table.lens_aperture_housing_radius) * 0.25, 0, 0, 0)
    out = (C.c_double * 5)()
    orc.orc_pt_sample_aperture(lens, sensor, ap, shift)
    sensor[0] += sensor[2] * shift
    sensor[1] += sensor[3] * shift
    T = orc.orc_lens_evaluate(lens, sensor, out)
    return list(sensor), [out[0], out[1], out[2], out[3], T]


@pytest.mark.parametrize("name", lt.RUN)
def test_y0_intersection_and_focus_search(orc, interp, name):
    """the forward Newton step and lens_evaluate over a few hundred sensor shifts, bit for bit; the focus search's winner is
    the sequential loop's, and the shift the host library's setup put into the parameters"""
    p, model, table, keep = lt.setup(name)
    ctx = interp(name)
    rng = np.random.default_rng(13)
    shifts = np.concatenate([rng.uniform(-45.0, 45.0, N_SHIFTS - 53), rng.uniform(-2.0, 2.0, 50), [0.0, -45.0, 45.0]])
    lens = orc.orc_lens_create(C.byref(table))
    try:
        for lam in lt.LAMBDAS:
            dist, sensor, out = ctx.test_y0_intersection(shifts, lam)
            es, eo, ed = np.empty_like(sensor), np.empty_like(out), np.empty_like(dist)
            for i, sh in enumerate(shifts):
                es[i], eo[i] = _oracle_chain(orc, lens, table, float(sh), lam)
                ed[i] = orc.orc_camera_get_y0_intersection_distance(lens, float(sh), lam)
            assert np.array_equal(sensor, es, equal_nan=True)
            assert np.array_equal(out, eo, equal_nan=True)
            assert np.array_equal(dist, ed, equal_nan=True)
            if name != "one-term":
                assert np.isfinite(ed).mean() > 0.9
        for focal_mm, lam in ((1500.0, 0.55), (999999999.0, 0.62)):
            assert ctx.focus_search(focal_mm, lam) == orc.orc_logarithmic_focus_search(lens, focal_mm, lam), (name, focal_mm, lam)
    finally:
        orc.orc_lens_destroy(lens)
    assert ctx.focus_search(float(p.focus_distance), 550.0 * 0.001) == float(p.sensor_shift)


_rays = {}


def _oracle_rays(orc, name):
    if name not in _rays:
        p, model, table, keep = lt.setup(name)
        inp = _inputs(N_RAYS, 9, 1.1, 0.7)
        lens = orc.orc_lens_create(C.byref(table))
        want, tries = oracle_rays(orc, p, lens, None, inp, seed=SEED)
        orc.orc_lens_destroy(lens)
        if lt.BY_NAME[name]["min_draws"] >= lt.MIN_DRAWS:
            assert int((want[:, 6] != 0).sum()) > N_RAYS // 4 and int((tries > 0).sum()) > 0
        for a in (inp, want, tries):
            a.setflags(write=False)
        _rays[name] = (inp, want, tries)
    return _rays[name]


def _check_rays(ctx, orc, name, path):
    inp, want, want_tries = _oracle_rays(orc, name)
    got, got_tries = ctx.camera_rays(inp, lam=LAM, seed=SEED, want_tries=True)
    assert ctx.camera_rays_path() == path
    assert np.array_equal(got_tries, want_tries)
    bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(1))[0]
    assert bad.size == 0, (name, bad[:8], got[bad[:2]], want[bad[:2]])


@pytest.mark.parametrize("name", lt.RUN)
def test_camera_rays(orc, interp, name):
    """every word of every ray, and every try count ("empty-ap-dx" and the short tables change these and nothing else)"""
    _check_rays(interp(name), orc, name, _abi.RAYS_PATH_INTERPRETER)


_points = {}


def _oracle_points(orc, name):
    """N_QUERIES scene points x K_ATTEMPTS attempts from a random first one, as tests/trace_point_cases.py draws and answers
    them"""
    if name not in _points:
        p, model, table, keep = lt.setup(name)
        rng = np.random.default_rng(0x7A1)
        n, k = N_QUERIES, K_ATTEMPTS
        target = np.stack([rng.uniform(-600, 600, n), rng.uniform(-400, 400, n), rng.uniform(500, 5000, n)], 1)
        px, py = rng.integers(0, lt.W, n).astype(np.int32), rng.integers(0, lt.H, n).astype(np.int32)
        first = rng.integers(0, 3000, n).astype(np.uint32)
        cs = np.ascontiguousarray((-target / 10.0).astype(np.float32))
        lens = orc.orc_lens_create(C.byref(table))
        ok, tries, sensor = np.zeros((n, k), bool), np.zeros((n, k), np.int32), np.full((n, k, 2), np.nan)
        sp, tr = (C.c_double * 2)(), C.c_int()
        for i in range(n):
            t = oracle_lib.darr(-float(cs[i, 0]) * 10.0, -float(cs[i, 1]) * 10.0, -float(cs[i, 2]) * 10.0)
            for m in range(k):
                ok[i, m] = orc.orc_trace_ray_bw_po(C.byref(p), lens, None, t, sp, int(px[i]), int(py[i]), int(first[i]) + m, p.lambda_bw, C.byref(tr))
                tries[i, m] = tr.value
                if ok[i, m]:
                    sensor[i, m] = sp[0], sp[1]
        orc.orc_lens_destroy(lens)
        xy, pixel = tc.pixel_mapping(p, sensor)
        want = dict(ok=ok, tries=tries, sensor=sensor, xy=xy, pixel=np.where(ok, pixel, tc.VIGNETTED).astype(np.uint32))
        _points[name] = (cs, tc.pack_pixel(px, py), first, want)
    return _points[name]


@pytest.mark.parametrize("name", lt.RUN)
def test_trace_points(orc, interp, name):
    """pixels, continuous positions, sensor positions and try counts of every query, bit for bit"""
    cs, pixel, first, want = _oracle_points(orc, name)
    if lt.BY_NAME[name]["min_draws"] >= lt.MIN_DRAWS:
        assert int((want["pixel"] < tc.OUTSIDE).sum()) > N_QUERIES
    ctx = interp(name)
    got = ctx.trace_points(cs, pixel, K_ATTEMPTS, first_attempt=first, want_sensor=True, want_tries=True)
    assert ctx.trace_points_path() == _abi.POINTS_PATH_INTERPRETER
    _check_po(got, want, lt.setup(name)[0])


def _check_pass(ctx, orc, name, chroma, lens_mode, frame=True):
    """one pass of the context against the oracle's: counters, draw list, frame (the project's 1e-5 bar)"""
    p, model, table, keep = lt.setup(name, chroma)
    ref = lt.oracle_pass(orc, name, chroma)
    c = gpu_run(ctx, p, table, lt.stream(name)[0], lens_mode=lens_mode, compiled=False)
    assert _counts(c) == _counts(ref.counters()), name
    check_logs(ctx, ref)
    if lt.BY_NAME[name]["negative"]:
        assert ctx.draw_log().shape[0] == 0 and c.attempted_draws > 0
    if chroma:
        assert set(np.unique(ctx.draw_log()[:, 1] >> 30)) == {0, 1, 2}
    if frame:
        check_frame(ctx, ref)
    return c


PASSES = [(n, 0.0) for n in lt.RUN] + [(c["name"], lt.CHROMA) for c in lt.CASES if c["chroma"]]
PASS_IDS = [n + ("-chroma" if ch else "") for n, ch in PASSES]


@pytest.mark.parametrize("stream", ["0", "1"], ids=["chunked", "streamed"])
@pytest.mark.parametrize("name,chroma", PASSES, ids=PASS_IDS)
def test_pass(orc, interp, monkeypatch, name, chroma, stream):
    """64 x 48 x 9 visits, samples_override 48, the interpreter: a context's first pass waits for its scan, its second runs
    blind -- per chunk under LENTIL_STREAM=0, streamed under LENTIL_STREAM=1"""
    monkeypatch.setenv("LENTIL_STREAM", stream)
    ctx = interp(name, chroma)
    first = _check_pass(ctx, orc, name, chroma, 1)
    assert first.streamed == 0 and first.blind_chunks == 0
    second = _check_pass(ctx, orc, name, chroma, 1)
    assert second.blind_chunks >= 1 and second.streamed == (1 if stream == "1" else 0)


# ---- stragglers ----------------------------------------------------------------------------------------------------------------
STRAGGLERS = [(n, lt.CHROMA if lt.BY_NAME[n]["chroma"] else 0.0) for n in lt.STRAGGLER_CASES]


@pytest.fixture
def straggler_env(monkeypatch):
    monkeypatch.setenv("LENTIL_SLOW_AT", str(lt.SLOW_AT))
    monkeypatch.setenv("LENTIL_SLOW_FROM_ROUND", "0")
    monkeypatch.setenv("LENTIL_SLOW_MAX_LANES", "64")       # by default a dry wave parks only its last four lanes


@pytest.mark.parametrize("name,chroma", STRAGGLERS, ids=[n + ("-chroma" if ch else "") for n, ch in STRAGGLERS])
def test_stragglers(orc, interp, straggler_env, name, chroma):
    """Solves still running after two iterations are parked and finished by solve_slow_kernel (CoopLens: ipow_lane, the
    per-channel lambda_pow tables, `if (c)`, 40 KB of dynamic LDS a wave on the 1536-term table), and the counters and the draw
    list stay the oracle's.  What that holds the cooperative kernel to is pixels: on "high-exponents" and "lambda-powers" the
    terms with exponents 10-15 and wavelength powers 3-15 decide 40 % and 95 % of the draws' pixels
    (tests/test_lens_table_cases.py, MIN_MOVED), so a wrong exponent or a wrong lambda_pow entry there moves hundreds of draws
    -- tried once with ipow_lane taking 13 for 12 and with lambda_pow[e - 1] for e >= 10: both fail here; a power that is
    wrong in its last bit moves no draw and is not seen.
    The bar on slow_solves: only waves that have run dry park, and a full queue (at least 3072 usable records, sized from the
    pass's draws) leaves a solve in its lane, so the oracle's iteration counts bound the parked solves from above, not from
    below.  What they do say: on every one of these tables nine solves in ten run longer than two iterations
    (tests/test_lens_table_cases.py::test_stragglers_would_be_parked), the regime in which
    test_stragglers_finish_in_the_cooperative_kernel asks for more than 1000 parked solves of this very frame's ~29 000 attempts
    -- a third of the smallest queue.  The same bar is kept."""
    ctx = interp(name, chroma)
    c = _check_pass(ctx, orc, name, chroma, 1, frame=not chroma)
    print(name, "parked", int(c.slow_solves), "of", int(c.attempted_draws), "attempts")
    assert c.slow_solves > 1000                        # (the bar of test_stragglers, and why it is that one)


# ---- the run-time kernels ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def jit(tmp_path_factory):
    """Every table of JIT_CASES set on contexts of its own first -- set_lens hands each to a compiling thread -- then one wait
    for all of them.  Per table: a context for the passes and the rays (created under LENTIL_RAYS_COMPILED=1) and one created
    under the straggler switches; both share the table's one compilation.  The contexts are closed only after every
    compilation has ended."""
    mp = pytest.MonkeyPatch()
    mp.setenv("LENTIL_JIT_CACHE", str(tmp_path_factory.mktemp("jit_cache")))
    mp.delenv("LENTIL_LENS_JIT", raising=False)
    made, ctxs = [], {}
    try:
        t0 = time.time()
        for name in lt.JIT_CASES:
            p, model, table, keep = lt.setup(name)
            pair = []
            for env in ({"LENTIL_RAYS_COMPILED": "1"},
                        {"LENTIL_SLOW_AT": str(lt.SLOW_AT), "LENTIL_SLOW_FROM_ROUND": "0", "LENTIL_SLOW_MAX_LANES": "64"}):
                with pytest.MonkeyPatch.context() as m:
                    for k, v in env.items():
                        m.setenv(k, v)
                    ctx = capi.Context(0)
                made.append(ctx)
                ctx.set_params(p)
                ctx.set_lens(table)
                assert ctx.lens_jit_status()[0] in (1, 2)
                pair.append(ctx)
            ctxs[name] = tuple(pair)
        failed = []
        for name, (ctx, slow) in ctxs.items():
            try:
                ctx.lens_jit_wait(900.0)
            except capi.LentilError as e:
                failed.append((name, str(e)))
        wall = time.time() - t0
        print("run-time kernels of %d tables: %.1f s of wall time; compile seconds each: %s" % (
            len(ctxs), wall, ", ".join("%s %.1f" % (n, c[0].lens_jit_status()[1]) for n, c in ctxs.items())))
        assert not failed, failed
        yield ctxs
    finally:
        for ctx in made:                      # (whatever happened above: no compilation is left running behind a closed context)
            try:
                ctx.lens_jit_wait(900.0)
            except capi.LentilError:
                pass
        for ctx in made:
            ctx.close()
        mp.undo()


_jit_passes = {}          # passes a context of the fixture has done: its first one waits for its scan, later ones run blind


def _jit_pass(ctx, orc, name, chroma):
    c = _check_pass(ctx, orc, name, chroma, 0)
    done = _jit_passes.get(id(ctx), 0)
    _jit_passes[id(ctx)] = done + 1
    if done == 0:
        assert c.streamed == 0 and c.blind_chunks == 0
    return c, done


@pytest.mark.parametrize("name", lt.JIT_CASES)
def test_run_time_kernel_passes(orc, jit, name):
    """lens mode 0 on a table with a compiled kernel: chunked, then streamed; draw lists the oracle's (and so the
    interpreter's, test_pass), frames inside the bar"""
    ctx, slow = jit[name]
    assert ctx.lens_jit_status()[0] == 2 and not ctx.lens_is_compiled()
    _jit_pass(ctx, orc, name, 0.0)
    second, done = _jit_pass(ctx, orc, name, 0.0)          # (the same stream as the pass before it: blind, streamed)
    assert second.streamed == 1 and second.blind_chunks >= 1
    assert ctx.lens_jit_status()[0] == 2              # (a code object that does not load is reported here as failed)


@pytest.mark.parametrize("name", lt.JIT_CASES)
def test_run_time_kernel_with_stragglers(orc, jit, name):
    """the run-time kernel parks, the cooperative kernel finishes: the hand-over between the two evaluations of one table"""
    ctx, slow = jit[name]
    c, done = _jit_pass(slow, orc, name, 0.0)
    assert slow.lens_jit_status()[0] == 2
    print(name, "parked", int(c.slow_solves), "of", int(c.attempted_draws), "attempts")
    assert c.slow_solves > 1000                        # (the bar of test_stragglers, and why it is that one)


def test_run_time_kernel_chroma(orc, jit):
    ctx, slow = jit["lambda-powers"]
    for k in range(2):                                 # (the three-channel instances of the run-time kernel, both forms of the pass)
        c, done = _jit_pass(ctx, orc, "lambda-powers", lt.CHROMA)
    assert c.blind_chunks >= 1 and ctx.lens_jit_status()[0] == 2


@pytest.mark.parametrize("name", lt.JIT_CASES)
def test_run_time_kernel_camera_rays(orc, jit, name):
    ctx, slow = jit[name]
    ctx.set_params(lt.setup(name)[0])
    ctx.set_lens_mode(0)
    _check_rays(ctx, orc, name, _abi.RAYS_PATH_RUN_TIME)


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refused_tables_leave_the_context_as_it_was(orc, interp):
    """set_lens with 1537 packed terms or an exponent of 16 returns LENTIL_ERR_UNSUPPORTED and changes nothing: the next pass
    with the good table set again is the earlier one draw for draw"""
    good = "high-exponents"
    ctx = interp(good)
    _check_pass(ctx, orc, good, 0.0, 1)
    before = common.sort_log(ctx.draw_log())
    refused = [c["name"] for c in lt.CASES if c["refused"]]
    assert len(refused) == 6
    for name in refused:
        table, keep = lt.table(name)
        with pytest.raises(capi.LentilError) as e:
            ctx.set_lens(table)
        assert e.value.code == _abi.ERR_UNSUPPORTED, (name, e.value)
    _check_pass(ctx, orc, good, 0.0, 1)
    assert np.array_equal(common.sort_log(ctx.draw_log()), before) and before.shape[0] >= lt.MIN_DRAWS
