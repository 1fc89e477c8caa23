"""The cryptomatte replay across table widths, tile tails, stream shapes and forms of the pass (tests/crypto_cases.py), against
the oracle.

Each case: the own-pixel kernel and variant the pass launched (lentil_hip_debug_last_crypto) are what the case's shape
selects; the counters equal the oracle's; the id set of every pixel is the oracle's exactly; weights and totals are within
1e-5 of the pixel's total (compare_tables of tests/test_crypto.py), and bit for bit on every pixel no draw lands on wherever an
owner or tile kernel ran -- one lane adds such a pixel's visits in stream order; the ranked images are compared with
compare_ranks, and bit for bit on every pixel where the stream redistributes nothing (ties, rotate, many); the beauty's weight
is within 1e-5.  tests/test_crypto_cases.py holds the cases to what they claim."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import common
import crypto_cases as cc
from pota_amd import capi
from test_crypto import TOL, compare_ranks, compare_tables

pytestmark = pytest.mark.gpu

# what the library reads once per process (test_child sets them for its children)
FLAGS_FROM_WORK = 0 if os.environ.get("LENTIL_CRYPTO_FLAGS", "1")[:1] == "0" else capi.CRYPTO_FLAGS_FROM_WORK
ONE_BLOCK_PER_CU = os.environ.get("LENTIL_CRYPTO_TILE_BLOCKS") == "1"


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _env(monkeypatch, case):
    for name, value in (("LENTIL_CRYPTO_TILE", case["tile"]), ("LENTIL_CRYPTO_LAZY_CLEAR", "1" if case["lazy"] else None)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)
    for name in ("LENTIL_STREAM", "LENTIL_CHUNKS"):
        monkeypatch.delenv(name, raising=False)
    for name, value in case["ctx_env"].items():
        monkeypatch.setenv(name, value)


def _context(make, case, b):
    ctx = make()
    ctx.set_params(b["p"])
    if b["table"] is not None:
        ctx.set_lens(b["table"])
    ctx.set_bokeh(None)
    ctx.alloc_frame(1)
    assert ctx.debug_last_crypto() == (0, 0, 0, 0)
    ctx.alloc_crypto(cc.N_CRYPTO, case["S"])
    if case["probe"]:
        ctx.set_occlusion_probe_device(capi.sphere_occluder_device(), b["sphere"].ctypes.data, None)
    _bind(ctx, b)
    assert ctx.debug_last_crypto() == (0, 0, 0, 0)          # nothing before the first pass
    return ctx


def _bind(ctx, b):
    ctx.upload_visits(b["visits"])
    cv, keep = capi.make_crypto_visits(b["hashes"], b["weights"])
    ctx.upload_crypto(cv)
    if b["lam"] is not None:
        ctx.set_visit_lambdas(b["lam"])


def _pass(ctx, clear=True):
    if clear:
        ctx.clear_frame()
    ctx.redistribute()
    ctx.resolve()
    ctx.sync()
    c = ctx.counters()
    assert c.worklist_overflow == 0
    return c


def _ran(ctx, case, variant=None, flushed=None):
    """the hook reads what the table says"""
    kernel, first = cc.expect_kernel(case)
    variant = first if variant is None else (variant if kernel == cc.TILE else 0)
    flushed = cc.expect_flushed(case) if flushed is None else flushed
    got = ctx.debug_last_crypto()
    if kernel == cc.TILE and not FLAGS_FROM_WORK:
        print("flags decided from the columns:", case["name"])
    bits = (FLAGS_FROM_WORK if kernel == cc.TILE else 0) | (capi.CRYPTO_WIPE_FLUSHED if flushed else 0)
    assert got[:2] == (kernel, variant) and got[3] == bits and got[2] >= 1, (case["name"], got, (kernel, variant, bits))
    if kernel == cc.TILE:
        tiles, tail = cc.tiles_and_tail(case)
        assert got[2] <= tiles + (1 if tail else 0)
    return got


def _same_counters(c, ref, passes=1):
    rc = ref.counters()
    assert (c.visits * passes, c.redistributed_visits * passes, c.accepted_draws * passes) == (rc.visits, rc.redistributed_visits, rc.accepted_draws)


def _untouched(ctx, *logs):
    m = np.ones(ctx.n_pixels, bool)
    for log in logs:
        m[log[:, 2]] = False
    return m


def _ranks_bit_for_bit(ctx, ref, ranks):
    for a in range(cc.N_CRYPTO):
        for rank in ranks:
            out, has = ctx.download_crypto(a, rank)
            rout, rhas = ref.crypto_rank(a, rank)
            assert np.array_equal(has, rhas), (a, rank)
            bad = np.flatnonzero((_bits(out) != _bits(rout)).any(axis=1) & rhas)
            # (an id of -0.0 comes back as the table's key, +0.0: equal as floats, as the maps' keys are)
            bad = [p for p in bad if not (np.array_equal(out[p], rout[p]) and np.array_equal(_bits(out[p, 1::2]), _bits(rout[p, 1::2])))]
            assert not bad, "crypto %d rank %d: %d pixels differ, first %d: %s against %s" % (a, rank, len(bad), bad[0], out[bad[0]], rout[bad[0]])
            assert not out[~rhas].any()


def _placed_where_the_probing_ends(ctx, case, b):
    """a stream that redistributes nothing, through an owner or tile kernel: a pixel's ids were entered in stream order, so
    each sits in the slot its probe sequence (crypto_first_slot, then slot after slot) reaches first"""
    own = {}
    for v in range(b["n"]):
        own.setdefault(int(b["pix"][v]), []).append(v)
    for a in range(cc.N_CRYPTO):
        ids, wts, tot = ctx.download_crypto_table(a)
        for pix, vs in own.items():
            keys = cc.own_visits_model(case, b, a, vs)[0]
            assert np.array_equal(ids[pix], cc.placement(keys, case["S"])), (case["name"], a, pix, ids[pix], keys)


def _compare(ctx, case, ref, untouched, exact=True, b=None):
    compare_tables(ctx, ref, cc.N_CRYPTO, ctx.n_pixels, exact_pixels=untouched if exact else None)
    ranked = sum(int(ref.crypto_rank(a, r)[1].sum()) for a in range(cc.N_CRYPTO) for r in case["ranks"])
    # (tests/test_crypto_cases.py: the near-tie rule leaves out at most 5 % of a case's ranked pixels)
    compare_ranks(ctx, ref, cc.N_CRYPTO, ranks=case["ranks"], min_checked=ranked - int(np.ceil(0.05 * ranked)) if not case["direct_only"] else 0)
    if case["direct_only"]:
        assert untouched.all()
        _ranks_bit_for_bit(ctx, ref, case["ranks"])
        if exact:
            _placed_where_the_probing_ends(ctx, case, b)
    buf, w = ctx.download_accum(0)
    rw = ref.weight()
    assert np.array_equal(w != 0, rw != 0) and common.rel_err(w[rw != 0], rw[rw != 0]) < TOL


def run_single(orc, make, monkeypatch, case):
    _env(monkeypatch, case)
    b = cc.build(case)
    ref = cc.oracle_frame(orc, case, b)
    try:
        ctx = _context(make, case, b)
        kernel = cc.expect_kernel(case)[0]
        streamed = []
        for frame in range(case["frames"]):
            c = _pass(ctx)
            got = _ran(ctx, case)
            _same_counters(c, ref)
            streamed.append(int(c.streamed))
            log = ctx.draw_log()
            assert np.array_equal(common.sort_log(log), common.sort_log(ref.log()))
            print(case["name"], "frame", frame, "hook", got, "streamed", c.streamed, "draws", log.shape[0])
            _compare(ctx, case, ref, _untouched(ctx, log), exact=kernel != cc.ATOMIC, b=b)
        if case["name"] == "streamed":
            assert streamed[0] == 0 and 1 in streamed[1:], streamed
        if case["name"] == "grid_stride" and ONE_BLOCK_PER_CU:
            tiles, tail = cc.tiles_and_tail(case)
            assert 1 <= got[2] < tiles, (got, tiles)         # blocks go round the tiles more than once
            print("grid stride: %d blocks walk %d tiles" % (got[2], tiles + 1))
        if case["name"] == "chunked":
            assert not any(streamed) and ctx.last_launches()[0] == 3, (streamed, ctx.last_launches())      # a scan per chunk
        if case["probe"]:
            assert ctx.probe_stats()[1] > 0
        if case["spectral"] and b["table"] is not None:
            assert ctx.spectral_pass_stats()[0] == case["frames"]
    finally:
        ref.close()


@pytest.mark.parametrize("case", cc.SINGLE, ids=[c["name"] for c in cc.SINGLE])
def test_crypto_shape(orc, gpu_ctx_factory, monkeypatch, case):
    run_single(orc, gpu_ctx_factory, monkeypatch, case)


def run_buckets(orc, make, monkeypatch):
    """The four buckets of a 64 x 48 frame, one after the other into one frame without a clear between them: variants 1, 0, 0, 0;
    the tables are the oracle's after the four streams."""
    cases = [cc.BY_NAME[n] for n in cc.BUCKETS]
    _env(monkeypatch, cases[0])
    bs = [cc.build(c) for c in cases]
    ref = cc.oracle_frame(orc, cases[0], bs[0])
    singles = [cc.oracle_frame(orc, c, b) for c, b in zip(cases[1:], bs[1:])]
    try:
        for c, b in zip(cases[1:], bs[1:]):
            ref.rebind_crypto(b["hashes"], b["weights"])
            cc.oracle_into(orc, ref, c, b)
        ctx = _context(make, cases[0], bs[0])
        logs = []
        for k, (case, b) in enumerate(zip(cases, bs)):
            if k:
                _bind(ctx, b)
            c = _pass(ctx, clear=(k == 0))
            _ran(ctx, case, variant=1 if k == 0 else 0)
            if k:
                _same_counters(c, singles[k - 1])
            logs.append(ctx.draw_log())
        rc = ref.counters()
        assert sum(l.shape[0] for l in logs) == rc.accepted_draws
        _compare(ctx, dict(cases[0], ranks=(0, 2, 4)), ref, _untouched(ctx, *logs))
    finally:
        ref.close()
        for r in singles:
            r.close()


def test_buckets_into_one_frame(orc, gpu_ctx_factory, monkeypatch):
    run_buckets(orc, gpu_ctx_factory, monkeypatch)


def test_accumulate_two_passes_behind_one_clear(orc, gpu_ctx_factory, monkeypatch):
    """clear, pass, pass: variant 1, then 0 -- the second pass reads the lines, adds to them and writes them back"""
    case = cc.BY_NAME["accumulate"]
    _env(monkeypatch, case)
    b = cc.build(case)
    ref = cc.oracle_frame(orc, case, b, passes=2)
    try:
        ctx = _context(make=gpu_ctx_factory, case=case, b=b)
        c = _pass(ctx)
        _ran(ctx, case, variant=1)
        log = ctx.draw_log()
        c = _pass(ctx, clear=False)
        _ran(ctx, case, variant=0)
        _same_counters(c, ref, passes=2)
        assert np.array_equal(common.sort_log(ctx.draw_log()), common.sort_log(log))
        _compare(ctx, case, ref, _untouched(ctx, log))
    finally:
        ref.close()


def test_lazy_clear_then_download_before_any_pass(orc, gpu_ctx_factory, monkeypatch):
    """the wipe is put off; a download before any pass flushes it and reads empty tables; the pass that follows finds them wiped"""
    case = cc.BY_NAME["lazy_download_first"]
    _env(monkeypatch, case)
    b = cc.build(case)
    ref = cc.oracle_frame(orc, case, b)
    try:
        ctx = _context(gpu_ctx_factory, case, b)
        monkeypatch.delenv("LENTIL_CRYPTO_LAZY_CLEAR")
        _pass(ctx)                                          # the tables hold a frame
        monkeypatch.setenv("LENTIL_CRYPTO_LAZY_CLEAR", "1")
        ctx.clear_frame()
        for a in range(cc.N_CRYPTO):
            ids, wts, tot = ctx.download_crypto_table(a)
            assert (ids == 0xFFFFFFFF).all() and not _bits(wts).any() and not _bits(tot).any()
            out, has = ctx.download_crypto(a, 0)
            assert not has.any() and not _bits(out).any()
        c = ctx.redistribute()
        ctx.resolve(); ctx.sync()
        _ran(ctx, case, variant=1, flushed=False)            # (the download has flushed it)
        _same_counters(ctx.counters(), ref)
        _compare(ctx, case, ref, _untouched(ctx, ctx.draw_log()))
    finally:
        ref.close()


def _placed(ctx, a):
    ids, wts, tot = ctx.download_crypto_table(a)
    return ids, wts, tot


def test_overflow_is_counted_and_the_rest_is_right(orc, gpu_ctx_factory, monkeypatch):
    """Pixels that meet S + 2 ids: the pass fails with the number of adds that found the table full -- the number a walk of
    the pixel's visits in order gives --, pixels that did not overflow hold the oracle's sums bit for bit, the others the
    model's placed ids and sums, and the tile and owner kernels agree.  crypto_direct_kernel places ids in any order: the
    error alone."""
    tables = {}
    for name in ("overflow_tile", "overflow_owner", "overflow_atomic"):
        case = cc.BY_NAME[name]
        _env(monkeypatch, case)
        b = cc.build(case)
        ref = cc.oracle_frame(orc, case, b)
        try:
            ctx = _context(gpu_ctx_factory, case, b)
            ctx.clear_frame()
            with pytest.raises(capi.LentilError, match="table full") as e:
                ctx.redistribute()
            _ran(ctx, case)
            if cc.expect_kernel(case)[0] == cc.ATOMIC:
                continue
            own = {}
            for v in range(b["n"]):
                own.setdefault(int(b["pix"][v]), []).append(v)
            want_full = 0
            got = [_placed(ctx, a) for a in range(cc.N_CRYPTO)]
            over = 0
            for pix, vs in own.items():
                for a in range(cc.N_CRYPTO):
                    keys, sums, total, full = cc.own_visits_model(case, b, a, vs, slots=case["S"])
                    want_full += full
                    ids, wts, tot = got[a]
                    used = ids[pix] != 0xFFFFFFFF
                    have = dict(zip(ids[pix][used].tolist(), _bits(wts[pix][used]).tolist()))
                    assert have == dict(zip(keys, _bits(np.array(sums, np.float32)).tolist())), (name, pix, a)
                    assert np.array_equal(ids[pix], cc.placement(keys, case["S"])), (name, pix, a)      # each id where its probing ends
                    assert _bits(tot[pix]) == _bits(total)
                    if not full:
                        rk, rw, rtot = ref.crypto_pixel(a, pix)
                        order = np.argsort(np.array(keys, np.uint32).view(np.float32), kind="stable")
                        assert np.array_equal(np.array(keys, np.uint32).view(np.float32)[order], rk)
                        assert np.array_equal(_bits(np.array(sums, np.float32)[order]), _bits(rw)) and _bits(total) == _bits(np.float32(rtot))
                    over += bool(full)
            assert over > 100 and want_full > 0
            assert re.search(r"(^|\D)%d cryptomatte adds found" % want_full, str(e.value)), (str(e.value), want_full)
            tables[name] = got
        finally:
            ref.close()
    for a in range(cc.N_CRYPTO):
        for x, y in zip(tables["overflow_tile"][a], tables["overflow_owner"][a]):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


# ---- children: what the library reads once per process ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cc.CHILDREN))
def test_child(name):
    """LENTIL_CRYPTO_TILE_BLOCKS=1: 302 tiles and a 5-pixel tail under num_cu blocks -- the grid-stride loop, the barrier at its
    head and the reuse of LDS between tiles (the case's own test asserts blocks < tiles there); LENTIL_CRYPTO_FLAGS=0: the
    redistributed visits decided again from the columns, for a tail, the buckets and the thin lens (their tests expect the
    hook's bit 0 clear there).  Each in one child pytest process, started once behind the parent's own GPU work, with a time
    limit."""
    child = cc.CHILDREN[name]
    env = dict(os.environ, **child["env"])
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-s", "-m", "gpu", "-k", child["select"]], env=env,
                       cwd=common.ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "%d passed" % child["tests"] in r.stdout and "skipped" not in r.stdout, r.stdout[-3000:]
    for line in child["says"]:
        assert line in r.stdout, (line, r.stdout[-3000:])
