"""The table of lens-table cases (tests/lens_tables.py) against the oracle alone -- no GPU: what keeps
tests/test_gpu_lens_tables.py from passing emptily.

Per case: the structural facts the case claims, computed from its spec (which exponents occur where, the packed count by
pack_lens_table's own rule, which polynomials are empty); the vacuity bars -- on the GPU test's pass the oracle alone still
redistributes MIN_VISITS visits and accepts MIN_DRAWS draws with the table (the negative case: none, and says so); for a case
that adds or reorders terms, that the oracle's lt_sample_aperture over the GPU test's own points differs from the table it
descends from at half of the converged points at least and that the draw list differs -- for the two cases whose terms are
meant to be seen through a pass, that a twentieth of the draws lie elsewhere (MIN_MOVED) --, so that the case would notice what
it is there for; and the two refusals, from the library's own packing (no GPU: lentil_hip_debug_lens_jit_compile).
"""
import collections
import re

import numpy as np
import pytest

import lens_tables as lt
from pota_amd import _abi, capi, lens_io


def _exps(terms, field):
    return set(int(e[field]) for c, e in terms)


# ---- the list ------------------------------------------------------------------------------------------------------------------
def test_every_entry_is_covered_and_every_case_needed():
    named = collections.Counter(t for c in lt.CASES for t in c["covers"])
    assert set(named) == set(lt.REQUIRED), (sorted(set(lt.REQUIRED) - set(named)), sorted(set(named) - set(lt.REQUIRED)))
    assert len(set(lt.REQUIRED)) == len(lt.REQUIRED)
    for c in lt.CASES:
        assert any(named[t] == 1 for t in c["covers"]), "%s is the only cover of nothing" % c["name"]      # deleting it would show
        assert c["note"] and c["name"] in lt._BUILDERS
    assert sum(1 for c in lt.CASES if c["negative"]) == 1
    for names in (lt.STRAGGLER_CASES, lt.JIT_CASES, lt.EMITTER_CASES):
        assert set(names) <= set(lt.RUN) and len(set(names)) == len(names)
    assert len(lt.JIT_CASES) <= 12                   # compiled side by side, a thread each, on 16 CPUs


def test_the_limits_are_the_librarys():
    with open(lt.common.ROOT + "/pota_amd/csrc/lentil_device.h") as f:
        src = f.read()
    assert "constexpr int kMaxTerms = %d;" % lt.MAX_TERMS in src and "constexpr int kMaxExp = %d;" % lt.MAX_EXP in src


def test_the_shipped_tables_reach_none_of_this():
    """what the cases add is not in a shipped table: no exponent above 9, no wavelength exponent above 2, no empty polynomial,
    no polynomial shorter than 16 terms, 471 ... 707 packed terms"""
    counts = {}
    for name in lens_io.available_lenses():
        spec = lens_io.load_lens_json(name)
        pk = lt.packed_polys(spec)
        assert max(max(_exps(t, f)) for t in pk.values() for f in range(4)) <= 9
        assert max(max(_exps(t, 4)) for t in pk.values()) <= 2
        assert min(len(spec["polys"][n]) for n in lt.POLYS) >= 16 and min(len(t) for t in pk.values()) >= 1
        counts[name] = lt.packed_count(spec)
    assert counts == {"double_gauss_50mm": 533, "petzval_58mm": 707, "anamorphic_petzval_58mm": 471}


# ---- structure -----------------------------------------------------------------------------------------------------------------
def test_high_exponents_structure():
    spec = lt.spec("high-exponents")
    pk = lt.packed_polys(spec)
    for v in range(4):
        for poly in lt.ITERATION + ("out_t",):
            assert set(range(10, 16)) <= _exps(spec["polys"][poly], v), (poly, v)
    # ... and one less in the derivatives the iteration evaluates: ap_x, ap_y by dx, dy; out_dx, out_dy by x, y
    for i in range(2):
        for j in range(2):
            assert set(range(9, 15)) <= _exps(pk["P_DAP_%d%d" % (i, j)], 2 + j)
            assert set(range(9, 15)) <= _exps(pk["P_DOUT_%d%d" % (i, j)], j)
            assert set(range(9, 15)) <= _exps(pk["P_DAPPOS_%d%d" % (i, j)], j)
    assert max(max(e) for t in pk.values() for c, e in t) == lt.MAX_EXP


def test_all_fifteen_structure():
    spec = lt.spec("all-fifteen")
    for poly in lt.ITERATION + ("out_t",):
        es = [tuple(e) for c, e in spec["polys"][poly]]
        assert (15,) * 5 in es
        for f in range(5):
            assert tuple(15 if v == f else 0 for v in range(5)) in es, (poly, f)
    # the derivatives keep 15 beside 14: the neighbours of a decremented field stay full
    pk = lt.packed_polys(spec)
    assert (14, 15, 15, 15, 15) in [tuple(e) for c, e in pk["P_DOUT_00"]] and (15, 15, 15, 14, 15) in [tuple(e) for c, e in pk["P_DAP_01"]]
    assert all(np.isfinite(c) and c != 0.0 for t in pk.values() for c, e in t)


def test_lambda_powers_structure():
    spec = lt.spec("lambda-powers")
    pk = lt.packed_polys(spec)
    for poly in lt.ITERATION + ("out_t",):
        assert set(range(3, 16)) <= _exps(spec["polys"][poly], 4), poly
    for name, terms in pk.items():
        if name.startswith("P_DAP_") or name.startswith("P_DOUT_"):
            assert len(_exps(terms, 4) & set(range(3, 16))) >= 3, name          # the derivatives read the high entries too
    assert lt.BY_NAME["lambda-powers"]["chroma"] and [c["name"] for c in lt.CASES if c["chroma"]] == ["lambda-powers"]


def test_paraxial_and_degree_3_structure():
    spec = lt.spec("paraxial")
    assert all(2 <= len(spec["polys"][n]) <= 4 for n in lt.POLYS)
    assert all(sum(e[:4]) <= 1 for n in lt.POLYS for c, e in spec["polys"][n])
    assert lt.packed_count(spec) == 39
    # (a paraxial ap_x has no dy in it: its cross derivatives are empty, as in "empty-derivatives"; the others have 1-2 terms)
    assert max(len(t) for n, t in lt.packed_polys(spec).items() if n.startswith("P_")) <= 2
    spec3 = lt.spec("degree-3")
    assert all(sum(e[:4]) <= 3 for n in lt.POLYS for c, e in spec3["polys"][n]) and lt.packed_count(spec3) == 170


def _waits_used(table):
    """the n of every LENTIL_SWAIT_AFTERn the emitted members use (the source's #define lines name all eight, always)"""
    rc, src, log, seconds, code_bytes = capi.lens_jit_compile(table, compile=False)
    assert rc == 0
    assert all("#define LENTIL_SWAIT_AFTER%d(" % n in src for n in range(1, 9))
    return set(int(n) for n in re.findall(r"\n  LENTIL_SWAIT_AFTER(\d)\(", src[src.index("struct Lens_rt"):]))


def test_the_short_tables_make_the_emitter_use_every_wait_macro():
    """AFTER4 ... AFTER8 between them, each inside a member the run-time kernels call; AFTER1 ... AFTER3 are what the shipped
    tables use, and all they use"""
    used = {name: _waits_used(lt.table(name)[0]) for name in lt.WAITS_USED}
    assert used == lt.WAITS_USED
    assert set().union(*used.values()) >= set(range(2, 9)) and 1 in _waits_used(lt.table("full")[0])
    for n, name in ((4, "paraxial"), (5, "short-a"), (6, "short-a"), (7, "short-b"), (8, "one-term")):
        assert "emitter:swait-after-%d" % n in lt.BY_NAME[name]["covers"] and n in used[name]
    for lens in ("double_gauss_50mm", "petzval_58mm", "anamorphic_petzval_58mm"):
        assert _waits_used(lens_io.make_lens_table(lens_io.load_lens_json(lens))[0]) <= {1, 2, 3}
    assert set(lt.WAITS_USED) <= set(lt.JIT_CASES) and set(lt.WAITS_USED) <= set(lt.EMITTER_CASES)


def test_short_tables_structure():
    para = lt.spec("paraxial")
    for name in ("short-a", "short-b", "one-term"):
        spec = lt.spec(name)
        assert all(sum(e[:4]) <= 1 for n in lt.POLYS for c, e in spec["polys"][n])
        assert len(spec["polys"]["ap_dx"]) == len(spec["polys"]["ap_dy"]) == 1
        assert spec["polys"]["out_t"] == para["polys"]["out_t"]
    pk = lt.packed_polys(lt.spec("short-b"))
    assert [len(pk["P_DAP_%d%d" % (i, j)]) for i in range(2) for j in range(2)] == [2, 1, 1, 1]
    one = lt.spec("one-term")
    assert [len(one["polys"][n]) for n in ("out_x", "out_y", "out_dx", "out_dy")] == [1, 1, 1, 1]
    pk = lt.packed_polys(one)
    assert [len(pk["P_DAP_%d%d" % (i, j)]) for i in range(2) for j in range(2)] == [1, 1, 1, 1]
    assert len(pk["P_DOUT_00"]) == len(pk["P_DOUT_11"]) == 1             # the solve's second 2x2 system is still regular


def test_empty_polynomials():
    pk = lt.packed_polys(lt.spec("empty-derivatives"))
    assert [n for n, t in pk.items() if not t] == ["P_DAP_01", "P_DAP_10"]
    assert lt.packed_count(lt.spec("empty-derivatives")) == 428
    assert [n for n, t in lt.packed_polys(lt.spec("empty-polynomial")).items() if not t] == ["out_t"]
    assert [n for n, t in lt.packed_polys(lt.spec("empty-ap-dx")).items() if not t] == ["ap_dx"]
    # the emitter's "0.0" targets and PlainEmitter's empty branch are written
    src = capi.lens_jit_compile(lt.table("empty-derivatives")[0], compile=False)[1]
    assert "  Jap[1] = 0.0;" in src and "  Jap[2] = 0.0;" in src and "  Jap[0] = acc" in src
    src = capi.lens_jit_compile(lt.table("empty-polynomial")[0], compile=False)[1]
    assert "  const double t = 0.0;" in src
    src = capi.lens_jit_compile(lt.table("empty-ap-dx")[0], compile=False)[1]
    assert "  pred_dir[0] = 0.0;" in src and "  pred_dir[1] = acc" in src


def test_shuffled_structure():
    a, b, shipped = lt.spec("_unshuffled"), lt.spec("shuffled"), lt.spec(lt.DG)
    key = lambda t: (tuple(t[1]), t[0].hex())           # noqa: E731  (hex: -0.0 and 0.0 are two terms)
    moved = 0
    for n in lt.POLYS:
        assert a["polys"][n][:len(shipped["polys"][n])] == shipped["polys"][n]
        assert sorted(map(key, a["polys"][n])) == sorted(map(key, b["polys"][n])) and a["polys"][n] != b["polys"][n]      # a permutation
        moved += sum(1 for x, y in zip(a["polys"][n], b["polys"][n]) if key(x) != key(y))
        monomials = collections.Counter(tuple(e) for c, e in b["polys"][n])
        assert sum(1 for m, k in monomials.items() if k > 1) >= lt.N_DUPLICATES
        zeros = [c for c, e in b["polys"][n] if c == 0.0]
        assert sorted(np.signbit(zeros).tolist()) == [False, True]
    assert moved > 0.9 * sum(len(b["polys"][n]) for n in lt.POLYS)
    first = b["polys"]["out_x"][0][0], b["polys"]["ap_x"][0][0]
    assert first == (0.0, 0.0) and np.signbit(first[0]) and not np.signbit(first[1])
    # a zero term is packed, derivative and all: the library drops terms by exponent only
    assert lt.packed_count(b) == lt.packed_count(a) == 594


def test_full_structure():
    spec = lt.spec("full")
    assert lt.packed_count(spec) == lt.MAX_TERMS
    pk = lt.packed_polys(spec)
    base = lt.spec(lt.PZ)
    for n in lt.POLYS:
        assert spec["polys"][n][:len(base["polys"][n])] == base["polys"][n] and len(spec["polys"][n]) > 2 * len(base["polys"][n])
    assert set(range(1, 16)) <= set().union(*[_exps(t, 4) for t in pk.values()])
    for v in range(4):
        assert set(range(1, 16)) <= set().union(*[_exps(t, v) for t in pk.values()]), v
    assert max(max(e) for t in pk.values() for c, e in t) == lt.MAX_EXP
    assert lt.packed_count(lt.spec("one-over")) == lt.MAX_TERMS + 1
    # the one term more is a term of out_t behind the same table
    over = lt.spec("one-over")
    assert all(over["polys"][n] == spec["polys"][n] for n in lt.POLYS if n != "out_t") and over["polys"]["out_t"][:-1] == spec["polys"]["out_t"]


def test_packed_count_is_the_librarys():
    """lens_tables.packed_count restates pack_lens_table: the emitted coefficient array holds every packed term the backward
    members read, and the table one above the limit is refused where the table at it is taken (test_refusals)"""
    for name in ("paraxial", "empty-derivatives", "full"):
        pk = lt.packed_polys(lt.spec(name))
        src = capi.lens_jit_compile(lt.table(name)[0], compile=False)[1]
        # eval_bw's loads: the 14 polynomials of the iteration, eight to a block
        bw = src[src.index("void eval_bw("):src.index("double transmittance(")]
        n_bw = sum(len(pk[n]) for n in ("ap_x", "ap_y", "out_x", "out_y", "out_dx", "out_dy") + tuple(
            "P_%s_%d%d" % (k, i, j) for k in ("DAP", "DOUT") for i in range(2) for j in range(2)))
        assert bw.count("LENTIL_SLOAD8(") == (n_bw + 7) // 8


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals():
    refused = [c["name"] for c in lt.CASES if c["refused"]]
    assert refused == ["one-over"] + ["exponent-16-%s" % f for f in lt.FIELDS]
    for f, name in enumerate(refused[1:]):
        spec = lt.spec(name)
        assert lt.packed_count(spec) <= lt.MAX_TERMS
        big = [(n, e) for n in lt.POLYS for c, e in spec["polys"][n] if max(e) > lt.MAX_EXP]
        assert len(big) == 1 and big[0][1][f] == 16 and max(e for i, e in enumerate(big[0][1]) if i != f) <= 1
    for name in refused:
        table, keep = lt.table(name)
        assert capi.lens_jit_compile(table, compile=False)[0] == _abi.ERR_UNSUPPORTED, name
    for name in ("full", "all-fifteen"):
        table, keep = lt.table(name)
        assert capi.lens_jit_compile(table, compile=False)[0] == 0, name


# ---- the oracle on the GPU test's pass ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", lt.RUN)
def test_the_table_is_still_a_lens(orc, name):
    """the vacuity bars (conditions, not measurements): MIN_VISITS redistributed visits, MIN_DRAWS accepted draws -- and for
    the negative case every attempt made (all 16 tries of every draw) and none accepted"""
    case = lt.BY_NAME[name]
    c = lt.oracle_pass(orc, name).counters()
    print(name, "redistributed", c.redistributed_visits, "attempted", c.attempted_draws, "accepted", c.accepted_draws)
    assert c.redistributed_visits >= lt.MIN_VISITS
    if case["negative"]:
        p = lt.setup(name)[0]
        assert c.accepted_draws == 0 and lt.oracle_pass(orc, name).log().shape[0] == 0
        assert c.attempted_draws == c.redistributed_visits * case["samples"] * p.bidir_sample_mult >= lt.MIN_DRAWS
        assert not (lt.oracle_aperture(orc, name)["T"] > 0).any()
    elif name == "one-term":          # (not a lens, lens_tables says why: its own bar, and every attempt made)
        assert lt.MIN_DRAWS > c.accepted_draws >= case["min_draws"] == 100
        assert c.attempted_draws == c.redistributed_visits * case["samples"] * lt.setup(name)[0].bidir_sample_mult
    else:
        assert c.accepted_draws >= case["min_draws"] == lt.MIN_DRAWS
        assert (lt.oracle_aperture(orc, name)["T"] > 0).mean() > 0.3


def test_the_chromatic_pass_is_not_empty(orc):
    """the same frame and the same bars; the three channels are all accepted into"""
    ref = lt.oracle_pass(orc, "lambda-powers", lt.CHROMA)
    c = ref.counters()
    print("chroma: redistributed", c.redistributed_visits, "attempted", c.attempted_draws, "accepted", c.accepted_draws)
    assert c.redistributed_visits >= lt.MIN_VISITS and c.accepted_draws >= 2 * lt.MIN_DRAWS
    assert set(np.unique(ref.log()[:, 1] >> 30)) == {0, 1, 2}
    # the channels' wavelengths differ, so their power tables do: the white pass's draws are not the chromatic pass's
    assert c.attempted_draws != lt.oracle_pass(orc, "lambda-powers").counters().attempted_draws


def _differing_share(orc, name, other):
    """the share of the points both tables converge on (T > 0) where any output word of lt_sample_aperture differs"""
    a, b = lt.oracle_aperture(orc, name), lt.oracle_aperture(orc, other, points_of=name)
    both = (a["T"] > 0) & (b["T"] > 0)
    assert both.sum() >= 0.3 * both.size
    differ = (a["sensor"] != b["sensor"]).any(-1) | (a["out"] != b["out"]).any(-1) | (a["T"] != b["T"])
    return float(differ[both].mean()), int(both.sum())


@pytest.mark.parametrize("name", [c["name"] for c in lt.CASES if c["derived"]])
def test_a_derived_table_differs_from_its_base(orc, name):
    """sensitivity: what the case adds reaches the solve (half of the converged points at least give other bits) and the
    draws (another draw list)"""
    base = lt.BY_NAME[name]["base"]
    share, n = _differing_share(orc, name, base)
    print(name, "differs from", base, "at %.3f of %d converged points" % (share, n))
    assert share >= 0.5
    mine = lt.common.sort_log(lt.oracle_pass(orc, name).log())
    theirs = lt.common.sort_log(lt.oracle_pass(orc, base).log())
    assert mine.shape != theirs.shape or not np.array_equal(mine, theirs)
    if name in lt.MOVED_CASES:
        # ... and many of them: the pass-level comparisons of the GPU test (counters, draw list) would notice one wrong term.
        # The camera is the base's (the focus search ends on the same sensor shift), so what moved the draws is the terms.
        assert lt.setup(name)[0].sensor_shift == lt.setup(base)[0].sensor_shift
        moved = len(set(map(tuple, mine.tolist())) - set(map(tuple, theirs.tolist())))
        print(name, "draws on other (visit, attempt, pixel) than the base's: %d of %d" % (moved, mine.shape[0]))
        assert moved >= lt.MIN_MOVED * mine.shape[0]


def test_the_permutation_alone_changes_bits(orc):
    """"shuffled" against "_unshuffled", the same terms in the fitter's order: only the order of the sums differs, and the
    oracle's own outputs differ in bits at half of the converged points at least -- a path that added a polynomial's terms in
    another order than the table's would be seen on this table"""
    share, n = _differing_share(orc, "shuffled", "_unshuffled")
    print("the permutation changes %.3f of %d converged points" % (share, n))
    assert share >= 0.5


def test_stragglers_would_be_parked(orc):
    """tests/test_gpu_lens_tables.py parks solves still running after SLOW_AT = 2 iterations: on every straggler case nearly
    every solve of the oracle runs longer than that, the regime of test_stragglers_finish_in_the_cooperative_kernel (whose
    bar of 1000 parked solves the GPU test keeps)"""
    for name in lt.STRAGGLER_CASES:
        it = lt.oracle_aperture(orc, name)["iters"]
        assert (it > lt.SLOW_AT).mean() >= 0.9, name
