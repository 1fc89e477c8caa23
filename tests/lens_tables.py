"""The polynomial lens tables the lens paths are tested with beyond the three shipped ones (tests/test_lens_table_cases.py: the
tables against the oracle alone, no GPU; tests/test_lens_jit.py: the emitter and the compilation; tests/test_gpu_lens_tables.py:
the kernels against the oracle).  A plain module: no fixtures, fixed seeds; every table is generated here from a shipped lens's
JSON, tests/golden/ gains nothing.

The shipped tables have 16-48 terms a polynomial, 471-707 packed terms, no exponent above 9 and no wavelength exponent above 2.
The library promises kMaxExp = 15, kMaxTerms = 1536 packed terms (the nine base polynomials and their twelve c * e derivatives,
pack_lens_table in csrc/lentil_hip.hip), exponents packed four bits a field into DevTerm::e, and polynomials of any length,
none included.  What can go wrong there, and the case that is there for it:

  high-exponents      the power recursion for exponents 10-15 -- written five times (ipow_u, ipow_lane, PowerTable::power,
                      tools/gen_lens_code.py, the host library / oracle), all of which must round alike: every exponent 10 ... 15
                      of every one of x, y, dx, dy, in every polynomial the Newton iteration evaluates (so 9 ... 14 in their
                      derivatives) and in out_t
  all-fifteen         the four-bit packing: a term with 15 in all five fields at once, and for every field a term with 15 in it
                      and 0 in its neighbours (a field that leaks into the next one, the wavelength field at bit 16)
  lambda-powers       lambda_pow[3 ... 15]: no shipped term reads beyond entry 2.  Also run with abb_chromatic = 0.5, where every
                      channel has a power table of its own
  paraxial            2-4 terms a polynomial: a block of eight coefficients touches up to eight polynomials, the emitter writes
                      LENTIL_SWAIT_AFTER4 ... AFTER8, which no shipped table makes it write
  short-a, short-b    "paraxial" reaches AFTER3 and AFTER4 only.  Two tables made from it -- ap_dx, ap_dy cut to one term; short-a: two
                      more wavelength terms in ap_y; short-b: a small dy term in ap_x and dx term in ap_y, so that all four
                      d ap / d (dx, dy) have one term -- make the emitter write AFTER5 and AFTER6 (short-a) and AFTER7 (short-b)
  one-term            AFTER8 needs eight one-term polynomials in a row, which only out_x ... out_dy cut to one term each give: a
                      table whose outgoing direction no longer depends on the sensor direction, so it cannot be focused (the host's
                      focus search ends at its bound, -45 mm) and nearly every draw vignettes.  NOT a lens: it is compiled, its
                      pass is compared (attempts equal, the few hundred accepted draws equal), and it is held to no vacuity bar
                      but its own
  degree-3            a mid-size table (170 packed terms) between the two
  empty-derivatives   ap_x free of dy, ap_y free of dx: P_DAP_01 and P_DAP_10 have count 0 (the emitter's "0.0" targets, CoopLens's
                      `if (c)`)
  empty-polynomial    out_t without a term (PlainEmitter's `!n`, the interpreter's empty loop).  The transmittance is then 0
                      everywhere and the oracle accepts nothing: this is the one NEGATIVE case -- every attempt is still made and
                      solved, the attempted counts must be equal, both draw lists empty
  empty-ap-dx         ap_dx without a term: a base polynomial only the forward paths (camera rays, focus search) read; the pass
                      does not notice, the rays do
  shuffled            summation order: the shipped table with every polynomial's terms in a seeded permutation, a few duplicated
                      monomials, and terms with coefficient 0.0 and -0.0 (one of each leads its polynomial).  Held against
                      the shipped table like every case, and against "_unshuffled", the same terms in the fitter's order:
                      those two differ in rounding only, which is what a path that reorders a sum would change
  full                exactly 1536 packed terms: 24 KB of s_terms, ~40 KB of dynamic LDS per straggler wave, uint16 first / count /
                      idx near their largest values.  Built from petzval_58mm -- every other case descends from
                      double_gauss_50mm
  one-over            1537 packed terms: refused
  exponent-16-<f>     an exponent of 16 in field f = x, y, dx, dy, lambda in turn: refused

The recipe of an added term: exponents as the case says, coefficient +-s / prod R_v^e_v with R = (18, 12, 0.45, 0.45, 0.65) for
x [mm], y [mm], dx, dy, lambda [um] -- about the largest values the variables take on a 36 mm sensor behind these lenses, so that a
term is at most about s wherever it is evaluated.  s = 1e-3 (1e-4 for the padding of "full", 1e-2 for what the short tables add,
1 for the all-fields term, whose monomial is below 1e-9 nearly everywhere); signs from the case's seeded generator.
"high-exponents" and "lambda-powers" use s = 0.1 (mm; a pixel of the test's frame is 0.56 mm): the cooperative straggler kernel and
the run-time kernels are reached through a pass only, and a pass delivers pixels, not bits -- with s = 1e-3 an added term moved
next to no draw, and a wrong exponent or a wrong lambda_pow entry in those kernels would have moved none.  At 0.1 the added terms
move 40 % and 95 % of the oracle's draws to other pixels (MIN_MOVED below is the bar), so an error in one of them moves
hundreds.  (An error in a power's LAST BIT moves a sensor position by 1e-16 of itself and no draw at any scale: that the
recursions round alike is shown bit for bit where a path has fp64 outputs -- the interpreter's primitives -- and for ipow_lane
only as far as pixels show it.)  tests/test_lens_table_cases.py holds every
table to what the oracle makes of it: still a lens (the vacuity bars below), and different from the table it descends from.
"""
import copy
import ctypes as C

import numpy as np

import common
import oracle_lib
from pota_amd import lens_io

R = (18.0, 12.0, 0.45, 0.45, 0.65)
FIELDS = ("x", "y", "dx", "dy", "lambda")
ITERATION = ("ap_x", "ap_y", "out_x", "out_y", "out_dx", "out_dy")        # what one Newton iteration evaluates (and their derivatives)
POLYS = tuple(lens_io.OUT_NAMES + lens_io.AP_NAMES)
MAX_TERMS, MAX_EXP = 1536, 15                                             # kMaxTerms, kMaxExp (pota_amd/csrc/lentil_device.h)
S_TERM, S_PAD, S_ALL, S_SHORT = 1e-3, 1e-4, 1.0, 1e-2
S_HIGH = 0.1              # the terms of "high-exponents" and "lambda-powers": large enough to move draws by whole pixels

# the pass every case is run with, on the GPU and by the oracle
W, H, M, SAMPLES, F_HI = 64, 48, 9, 48, 0.02
# the vacuity bars: what the oracle alone must find on that pass for a table to count as a lens (conditions, not measurements)
MIN_VISITS, MIN_DRAWS = 500, 20000
CHROMA = 0.5
# the share of the oracle's accepted draws that must lie on other (visit, attempt, pixel) triples than the base table's, for the
# two cases whose added terms are meant to be seen through a pass: a twentieth -- a thousand draws -- is far above what the
# one-draw differences of rounding give and leaves a single wrong term of the case's 168 / 91 its hundreds
MIN_MOVED = 0.05
MOVED_CASES = ("high-exponents", "lambda-powers")
# the negative case makes five attempts a sample (bidir_sample_mult) where a lens needs 1.1, each with all of its 16 tries: a sixth of
# the samples keep its pass as long as the others'
NEGATIVE_SAMPLES = 8
# lt_sample_aperture alone
N_POINTS = 2000
LAMBDAS = (float(np.float32(0.55)), 0.45, 0.62)

REQUIRED = (
    ["exponents:10-15:iteration", "exponents:9-14:derivatives", "exponents:10-15:out_t"] +
    ["packing:all-fields-15", "packing:single-field-15"] +
    ["lambda:3-15:iteration", "lambda:3-15:out_t", "lambda:3-15:chroma"] +
    ["short:2-4-terms", "emitter:swait-after-4"] + ["emitter:swait-after-%d" % n for n in (5, 6, 7, 8)] +
    ["size:170"] +
    ["empty:P_DAP_01", "empty:P_DAP_10"] +
    ["empty:out_t", "empty:ap_dx"] +
    ["order:permuted", "order:duplicates", "order:signed-zeros"] +
    ["size:1536", "lens:petzval_58mm"] +
    ["refusal:1537"] + ["refusal:exponent-16:%s" % f for f in FIELDS]
)

CASES = []


def _case(name, base, note, covers, negative=False, refused=False, chroma=False, derived=False, samples=SAMPLES, min_draws=MIN_DRAWS):
    """base: the shipped lens the case is made from.  derived: the case adds or reorders terms, so
    tests/test_lens_table_cases.py holds it to a sensitivity check against `base`.  chroma: also run with abb_chromatic = CHROMA.
    samples: samples_override of the case's pass.  min_draws: the accepted draws the oracle must find at least."""
    CASES.append(dict(name=name, base=base, note=note, covers=tuple(covers), negative=negative, refused=refused, chroma=chroma,
                      derived=derived, samples=samples, min_draws=0 if negative else min_draws))


DG, PZ = "double_gauss_50mm", "petzval_58mm"
_case("high-exponents", DG, "exponents 10-15 of x, y, dx, dy in every polynomial of the iteration and in out_t",
      ["exponents:10-15:iteration", "exponents:9-14:derivatives", "exponents:10-15:out_t"], derived=True)
_case("all-fifteen", DG, "15 in all five fields of one term; 15 in one field and 0 in the others, for every field",
      ["packing:all-fields-15", "packing:single-field-15"], derived=True)
_case("lambda-powers", DG, "wavelength exponents 3-15 in every polynomial of the iteration and in out_t",
      ["lambda:3-15:iteration", "lambda:3-15:out_t", "lambda:3-15:chroma"], chroma=True, derived=True)
_case("paraxial", DG, "only terms of total degree <= 1 in x, y, dx, dy: 2-4 terms a polynomial", ["short:2-4-terms", "emitter:swait-after-4"])
_case("short-a", "paraxial", "paraxial, ap_dx / ap_dy of one term, two more terms in ap_y: blocks that touch 5 and 6 polynomials",
      ["emitter:swait-after-5", "emitter:swait-after-6"], derived=True)
_case("short-b", "paraxial", "paraxial, ap_dx / ap_dy of one term, cross terms in ap_x / ap_y: a block that touches 7 polynomials",
      ["emitter:swait-after-7"], derived=True)
# (not a lens: a hundred accepted draws that agree pixel for pixel, among 3072 pixels, are no accident; the attempts are all made)
_case("one-term", "paraxial", "one term in each of out_x ... out_dy: a block that touches 8 polynomials; cannot be focused",
      ["emitter:swait-after-8"], min_draws=100)
_case("degree-3", DG, "only terms of total degree <= 3: 170 packed terms", ["size:170"])
_case("empty-derivatives", DG, "ap_x free of dy, ap_y free of dx: two derivative polynomials without a term", ["empty:P_DAP_01", "empty:P_DAP_10"])
_case("empty-polynomial", DG, "out_t without a term: transmittance 0, nothing accepted -- the negative case", ["empty:out_t"], negative=True,
      samples=NEGATIVE_SAMPLES)
_case("empty-ap-dx", DG, "ap_dx without a term: read by the forward paths only", ["empty:ap_dx"])
_case("shuffled", DG, "every polynomial's terms permuted; duplicated monomials; coefficients 0.0 and -0.0",
      ["order:permuted", "order:duplicates", "order:signed-zeros"], derived=True)
_case("full", PZ, "padded to exactly 1536 packed terms, from the second shipped lens", ["size:1536", "lens:petzval_58mm"], derived=True)
_case("one-over", PZ, "1537 packed terms", ["refusal:1537"], refused=True)
for _f in FIELDS:
    _case("exponent-16-%s" % _f, DG, "one term with exponent 16 in %s" % _f, ["refusal:exponent-16:%s" % _f], refused=True)

BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
RUN = [c["name"] for c in CASES if not c["refused"]]                    # the tables that run
POSITIVE = [c["name"] for c in CASES if not c["refused"] and not c["negative"]]
# the subsets the paths with a cost of their own are run on.  ("paraxial" is among the straggler cases: the oracle's solves on it
# take 18 iterations on average, as many as on any table, so it parks as much -- and its 35 needed terms are fewer than the
# cooperative kernel has lanes.)
STRAGGLER_CASES = ["high-exponents", "all-fifteen", "lambda-powers", "paraxial", "empty-derivatives", "shuffled", "full"]
SLOW_AT = 2               # LENTIL_SLOW_AT of the straggler passes: solves still running after two iterations are parked
JIT_CASES = ["high-exponents", "lambda-powers", "paraxial", "short-a", "short-b", "one-term", "empty-derivatives", "empty-polynomial", "full"]
EMITTER_CASES = ["high-exponents", "all-fifteen", "lambda-powers", "paraxial", "short-a", "short-b", "one-term", "empty-derivatives",
                 "empty-polynomial", "full"]
# LENTIL_SWAIT_AFTERn as the emitted members of a case use them (the #define lines name all eight in every source)
WAITS_USED = {"paraxial": {3, 4}, "short-a": {2, 3, 5, 6}, "short-b": {2, 3, 4, 6, 7}, "one-term": {2, 7, 8}}


# ---- the tables ---------------------------------------------------------------------------------------------------------------
def derive(terms, var):
    """the c * e derivative of a polynomial by variable var, as pack_terms forms it: terms without var are dropped"""
    return [[float(c) * float(e[var]), [ee - (1 if i == var else 0) for i, ee in enumerate(e)]] for c, e in terms if e[var] > 0]


def packed_polys(spec):
    """{name: terms} of the 21 polynomials the library packs (pack_lens_table): the nine base ones, d ap_{x,y} / d {dx,dy}
    (P_DAP_ij), d out_{dx,dy} / d {x,y} (P_DOUT_ij) and d ap_{x,y} / d {x,y} (P_DAPPOS_ij)"""
    polys = spec["polys"]
    out = {n: polys[n] for n in POLYS}
    for i, a in enumerate(("x", "y")):
        for j in range(2):
            out["P_DAP_%d%d" % (i, j)] = derive(polys["ap_" + a], 2 + j)
            out["P_DOUT_%d%d" % (i, j)] = derive(polys["out_d" + a], j)
            out["P_DAPPOS_%d%d" % (i, j)] = derive(polys["ap_" + a], j)
    return out


def packed_count(spec):
    return sum(len(t) for t in packed_polys(spec).values())


def _cost(poly, e):
    """packed terms one more base term of `poly` with exponents e costs"""
    if poly in ("ap_x", "ap_y"):
        return 1 + sum(1 for v in range(4) if e[v] > 0)
    if poly in ("out_dx", "out_dy"):
        return 1 + sum(1 for v in range(2) if e[v] > 0)
    return 1


def _term(sign, s, e):
    scale = 1.0
    for v in range(5):
        scale *= R[v] ** e[v]
    return [(1.0 if sign else -1.0) * s / scale, [int(x) for x in e]]


def _shipped(name):
    return copy.deepcopy(lens_io.load_lens_json(name))


def _high_exponents():
    spec, rng = _shipped(DG), np.random.default_rng(0x41E)
    for poly in ITERATION + ("out_t",):
        for v in range(4):
            for big in range(10, 16):
                e = [0] * 5
                other = int(rng.integers(0, 4))
                if other != v:
                    e[other] = int(rng.integers(0, 3))
                e[4] = int(rng.integers(0, 3))
                e[v] = big
                spec["polys"][poly].append(_term(rng.integers(0, 2), S_HIGH, e))
    return spec


def _all_fifteen():
    spec, rng = _shipped(DG), np.random.default_rng(0xF15)
    for poly in ITERATION + ("out_t",):
        spec["polys"][poly].append(_term(rng.integers(0, 2), S_ALL, [15] * 5))
        for f in range(5):
            spec["polys"][poly].append(_term(rng.integers(0, 2), S_TERM, [15 if v == f else 0 for v in range(5)]))
    return spec


def _lambda_powers():
    spec, rng = _shipped(DG), np.random.default_rng(0x1A3)
    for poly in ITERATION + ("out_t",):
        for k, le in enumerate(range(3, 16)):
            e = [0] * 5
            e[k % 4] = 1
            if k % 2:
                e[(k + 1) % 4] = 1
            e[4] = le
            spec["polys"][poly].append(_term(rng.integers(0, 2), S_HIGH, e))
    return spec


def _degree_at_most(n):
    spec = _shipped(DG)
    for poly in POLYS:
        spec["polys"][poly] = [t for t in spec["polys"][poly] if sum(t[1][:4]) <= n]
    return spec



def _short(cross, extra_y, one_term_out=False):
    """"paraxial" with ap_dx and ap_dy cut to their leading term and: cross -- a small dy term in ap_x and dx term in ap_y, so
    that all four d ap / d (dx, dy) have one term; extra_y -- that many more terms y * lambda^(3 + k) in ap_y (they move the
    blocks of eight along); one_term_out -- ap_x and ap_y without their dx * lambda^2 / the extra terms and every outer-pupil
    polynomial cut to the one term the solve cannot do without (out_x, out_y: the direction's; out_dx, out_dy: the position's)"""
    spec = _degree_at_most(1)
    P = spec["polys"]
    if one_term_out:
        P["ap_x"] = [t for t in P["ap_x"] if t[1] != [0, 0, 1, 0, 2]]
    if cross:
        P["ap_x"].insert(1, _term(1, S_SHORT, [0, 0, 0, 1, 0]))
        P["ap_y"].insert(1, _term(1, S_SHORT, [0, 0, 1, 0, 0]))
    for k in range(extra_y):
        P["ap_y"].append(_term(1, S_SHORT, [0, 1, 0, 0, 3 + k]))
    P["ap_dx"], P["ap_dy"] = P["ap_dx"][:1], P["ap_dy"][:1]
    if one_term_out:
        for n, f in (("out_x", 2), ("out_y", 3), ("out_dx", 0), ("out_dy", 1)):
            P[n] = [t for t in P[n] if t[1][f] == 1 and t[1][4] == 0]
    return spec


def _empty_derivatives():
    spec = _shipped(DG)
    spec["polys"]["ap_x"] = [t for t in spec["polys"]["ap_x"] if t[1][3] == 0]
    spec["polys"]["ap_y"] = [t for t in spec["polys"]["ap_y"] if t[1][2] == 0]
    return spec


def _without(poly):
    spec = _shipped(DG)
    spec["polys"][poly] = []
    return spec


N_DUPLICATES = 2          # per polynomial


def _unshuffled():
    """the shipped table with, behind every polynomial's own terms, N_DUPLICATES of its monomials once more (a thousandth of
    their coefficients) and a term with coefficient 0.0 and one with -0.0 on two more of them -- in this, the fitter's, order"""
    spec, rng = _shipped(DG), np.random.default_rng(0x5AF)
    for poly in POLYS:
        terms = spec["polys"][poly]
        pick = rng.choice(len(terms), N_DUPLICATES + 2, replace=False)
        extra = [[terms[i][0] / 1024.0, list(terms[i][1])] for i in pick[:N_DUPLICATES]]
        extra.append([0.0, list(terms[pick[-2]][1])])
        extra.append([-0.0, list(terms[pick[-1]][1])])
        terms.extend(extra)
    return spec


def _shuffled():
    spec, rng = _unshuffled(), np.random.default_rng(0x5AF + 1)
    for poly in POLYS:
        terms = spec["polys"][poly]
        terms[:] = [terms[i] for i in rng.permutation(len(terms))]
    # a polynomial led by -0.0 and one led by 0.0: what a sum starts from
    for poly, zero in (("out_x", -0.0), ("ap_x", 0.0)):
        terms = spec["polys"][poly]
        i = next(i for i, t in enumerate(terms) if t[0] == 0.0 and np.signbit(t[0]) == np.signbit(zero))
        terms.insert(0, terms.pop(i))
    return spec


def _full(target=MAX_TERMS):
    """petzval_58mm padded with terms over all nine polynomials -- every exponent 1 ... 15 of every variable and of the wavelength
    among them -- to exactly `target` packed terms; the last few are terms of out_t, which cost one packed term each"""
    spec, rng = _shipped(PZ), np.random.default_rng(0xF011)
    n, k = packed_count(spec), 0
    while n < target:
        poly = POLYS[k % len(POLYS)]
        e = [0] * 5
        e[k % 4] = 1 + (k // 4) % 15
        e[(k + 1 + k // 36) % 4] += int(rng.integers(0, 3))
        e[4] = (k // 9) % 16
        e = [min(x, MAX_EXP) for x in e]
        if _cost(poly, e) > target - n:
            poly = "out_t"
        spec["polys"][poly].append(_term(rng.integers(0, 2), S_PAD, e))
        n += _cost(poly, e)
        k += 1
    return spec


def _one_over():
    return _full(MAX_TERMS + 1)


def _exponent_16(field):
    spec = _shipped(DG)
    e = [1, 0, 1, 0, 0]
    e[field] = 16
    spec["polys"]["ap_x"].append(_term(1, S_TERM, e))
    return spec


_BUILDERS = {
    "high-exponents": _high_exponents, "all-fifteen": _all_fifteen, "lambda-powers": _lambda_powers,
    "paraxial": lambda: _degree_at_most(1), "degree-3": lambda: _degree_at_most(3), "empty-derivatives": _empty_derivatives,
    "short-a": lambda: _short(False, 2), "short-b": lambda: _short(True, 0), "one-term": lambda: _short(True, 0, True),
    "empty-polynomial": lambda: _without("out_t"), "empty-ap-dx": lambda: _without("ap_dx"), "_unshuffled": _unshuffled,
    "shuffled": _shuffled, "full": _full, "one-over": _one_over, DG: lambda: _shipped(DG), PZ: lambda: _shipped(PZ),
}
for _i, _f in enumerate(FIELDS):
    _BUILDERS["exponent-16-%s" % _f] = (lambda i: lambda: _exponent_16(i))(_i)

_specs, _setups, _streams, _aperture, _passes = {}, {}, {}, {}, {}


def spec(name):
    """the spec dict ({"constants", "polys"}) of a case, of "_unshuffled" or of a shipped lens; built once, never written to"""
    if name not in _specs:
        _specs[name] = _BUILDERS[name]()
    return _specs[name]


def table(name):
    """(lentil_lens_table, keepalive) -- no camera setup: what the refusals and the emitter need"""
    return lens_io.make_lens_table(spec(name))


def setup(name, chroma=0.0):
    """(params, model, table, keep): the camera set up on the table by the host library (its focus search runs on the table),
    for the W x H pass.  Cached; chroma != 0 copies the parameters and sets abb_chromatic."""
    if name not in _setups:
        _setups[name] = common.po_setup(W, H, lens=spec(name), samples_override=BY_NAME[name]["samples"] if name in BY_NAME else SAMPLES)
    p, model, tab, keep = _setups[name]
    if chroma:
        p = type(p).from_buffer_copy(p)
        p.abb_chromatic = chroma
    return p, model, tab, keep


def stream(name):
    """(visits, column arrays -- which must outlive the visits) of the W x H x M pass"""
    if name not in _streams:
        _streams[name] = common.make_stream(setup(name)[0], W, H, M, f_hi=F_HI)
    return _streams[name]


def oracle_pass(orc, name, chroma=0.0):
    """the oracle's pass over stream(name): an oracle_lib.Frame with its draw log, computed once and left open (nothing writes
    to it)"""
    key = (name, chroma)
    if key not in _passes:
        p, model, tab, keep = setup(name, chroma)
        _passes[key] = common.run_oracle(orc, p, tab, stream(name)[0])
    return _passes[key]


def sample_points(name):
    """(scene fp64 [N_POINTS, 3], aperture fp64 [N_POINTS, 2]): the points lt_sample_aperture is run on, drawn as
    tests/test_gpu_parity.py::test_lt_sample_aperture_bit_exact draws them"""
    p = setup(name)[0]
    rng = np.random.default_rng(2)
    n = N_POINTS
    scene = np.stack([rng.uniform(-4000, 4000, n), rng.uniform(-3000, 3000, n), rng.uniform(400, 20000, n)], 1)
    ap = rng.uniform(-1, 1, (n, 2)) * p.aperture_radius
    return scene, ap


def oracle_aperture(orc, name, points_of=None):
    """orc_lt_sample_aperture of table `name` over sample_points(points_of or name) at LAMBDAS -> dict: sensor, out fp64
    [3, N_POINTS, 5], T fp64 [3, N_POINTS] (0: no ray), iters int32 [3, N_POINTS] (Newton iterations).  Computed once."""
    key = (name, points_of or name)
    if key not in _aperture:
        scene, ap = sample_points(points_of or name)
        tab, keep = table(name)
        lens = orc.orc_lens_create(C.byref(tab))
        n = scene.shape[0]
        o = dict(sensor=np.empty((3, n, 5)), out=np.empty((3, n, 5)), T=np.empty((3, n)), iters=np.empty((3, n), np.int32))
        s5, o5, it = (C.c_double * 5)(), (C.c_double * 5)(), C.c_int()
        try:
            for k, lam in enumerate(LAMBDAS):
                for i in range(n):
                    for j in range(5):
                        o5[j] = 0.0
                    o5[4] = lam
                    o["T"][k, i] = orc.orc_lt_sample_aperture(lens, oracle_lib.darr(*scene[i]), oracle_lib.darr(*ap[i]), s5, o5, lam, C.byref(it))
                    o["sensor"][k, i] = list(s5)
                    o["out"][k, i] = list(o5)
                    o["iters"][k, i] = it.value
        finally:
            orc.orc_lens_destroy(lens)
        for a in o.values():
            a.setflags(write=False)
        _aperture[key] = o
    return _aperture[key]
