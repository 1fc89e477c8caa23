"""The draw pass across vignetting_retries: the cases of tests/test_gpu_retries.py, importable without a GPU.

vignetting_retries (the camera's "Vignetting Quality", 1-500 in the reference's UI, default 15) is how many further aperture
draws an attempt of the polynomial-optics draw loop may use once a try is vignetted (src/lentil.h:592).  On the GPU it picks
code paths all through the pass (pota_amd/csrc/lentil_kernels.h): up to kAcceptWinRetries = 64 an accept step's results are
staged in an LDS window of 256 + retries words, above that every try reads global memory; accept_kernel walks an item with
accept_item_wide only if retries <= 64, the draw's record is at most 64 floats and the pass is not chromatic; a lean streamed
pass with more than 64 retries runs accept_kernel<1> / <2> where it otherwise runs <3>; the first batches, the result pool and
the first-batch model are sized from it.  Every case names its retry count R; the families put R on both sides of 64 for
each of the three walkers.

A case is a dict: `name`, `family`, `R`, what po_setup / make_stream take (`lens`, `W`, `H`, `M`, `S` = samples_override,
`f_hi`, `n_extra`, `seed`, `chroma` = abb_chromatic), `kinds` (the frame's AOV filter kinds, None: all gaussian) and
`lens_mode` (0: the lens's compiled kernel, 1: the table interpreter).  Two cases with the same stream_key() differ in R
(and lens_mode) only: their oracle lists can be compared, tests/test_retry_cases.py does.
"""
import common

WIN = 64          # kAcceptWinRetries (pota_amd/csrc/lentil_kernels.h; tests/test_retry_cases.py reads it there)

# double-gauss, 64 x 40, 9 visits per pixel, 1 % highlights, 32 draws each: 234 redistributed visits, and the oracle's lists
# at neighbouring retry counts all differ (7770 / 7769 / 7768 attempts at 63 / 64 / 65)
BASE = dict(lens="double_gauss_50mm", W=64, H=40, M=9, S=32, f_hi=0.01, n_extra=0, seed=0x5EED, chroma=0.0, kinds=None, lens_mode=0)


def _case(name, family, R, **kw):
    c = dict(BASE)
    c.update(kw)
    c.update(name=name, family=family, R=R)
    return c


CASES = []
# 1. the pass across retry counts (first pass of a context: chunked)
CASES += [_case("base-r%d" % R, "base", R) for R in (0, 1, 2, 15, 63, 64, 65, 200)]
# (draw counts from the CoC formula: down to 4 per item, a first batch is nearly all retries)
CASES += [_case("base-coc-r500", "base-coc", 500, S=0)]
# (petzval: hopeless visits fail every try whatever the count -- many failing attempts, later rounds)
CASES += [_case("petzval-r%d" % R, "petzval", R, lens="petzval_58mm") for R in (0, 65)]
CASES += [_case("tables-r%d" % R, "base", R, lens_mode=1) for R in (0, 65)]
# 2. walker selection.  Sixteen gaussian AOVs (65 floats a draw): accept_item whatever R is -- window at 0 and 64, global reads at 65
# (seed 0xA00A: with the default seed and fifteen extra columns the oracle's lists at 64 and 65 are the same list)
CASES += [_case("aov16-r%d" % R, "aov16", R, n_extra=15, seed=0xA00A) for R in (0, 64, 65)]
# chromatic aberration: accept_item_chroma on both sides
CASES += [_case("chroma-r%d" % R, "chroma", R, chroma=0.5, S=16, n_extra=2, kinds=[0, 0, 1]) for R in (0, 64, 65, 200)]
CASES += [_case("chroma-neg-r65", "chroma-neg", 65, chroma=-0.5, S=16, n_extra=2, kinds=[0, 0, 1])]
# record widths accept_item_wide had not seen: U = 4 G + 1 floats a draw, 64 / U draws per instruction
CASES += [_case("wide-g%d-r%d" % (G, R), "wide-g%d" % G, R, n_extra=G - 1) for G in (5, 6, 7, 8, 12) for R in (15, WIN)]
# ... and two frames that mix gaussian with closest AOVs (six gaussian: U = 25)
MIXED = {"a": [0, 1, 0, 0, 0, 0, 0, 1], "b": [0, 0, 0, 0, 0, 0, 1, 1]}
CASES += [_case("mixed-%s-r%d" % (k, R), "mixed-" + k, R, n_extra=7, kinds=MIXED[k]) for k in ("a", "b") for R in (15, WIN)]
# 3. second and later passes of a context: streamed.  96 x 64 with 48 draws and 0.2 % highlights streams.
# (seed 0xBEEF: 4930 / 4929 / 4928 attempts at 63 / 64 / 65 retries; the default seed's lists are one list from 63 on)
STREAMED = dict(W=96, H=64, S=48, f_hi=0.002, seed=0xBEEF)
CASES += [_case("streamed-r%d" % R, "streamed", R, **STREAMED) for R in (0, 3, 65)]
# the lean tail (first batches from the model, no second round): accept_kernel<3> at 64, <1> / <2> at 65 -- ready_accept is
# false for the retry count alone
CASES += [_case("lean-r%d" % R, "lean", R, **STREAMED) for R in (WIN, WIN + 1)]
# 4. the occlusion probe (an occluded try costs a retry)
CASES += [_case("probe-r%d" % R, "probe", R, f_hi=0.02) for R in (0, 65)]
# 5. no try at all: `tries <= vignetting_retries` is false from the start
CASES += [_case("negative-r-3", "negative", -3)]

BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# thin lens: the parameter is not read (64 x 40, 32 draws)
THIN_R = (-1, 0, 200)

# families whose neighbouring retry counts must give pairwise different oracle lists: a walker that looks at one try too
# few or too many at the window's edge then changes the list
BOUNDARY = {"base": (63, 64, 65), "aov16": (64, 65), "chroma": (64, 65), "lean": (63, 64, 65)}

# the sphere of tests/test_gpu_probe.py, between the lens and the far highlights (camera space, cm; radius last)
SPHERE = (6.0, 2.0, -70.0, 9.0)


def named(*families):
    return [c for c in CASES if c["family"] in families]


def ids(cases):
    return [c["name"] for c in cases]


def n_aovs(c):
    return 1 + c["n_extra"]


def stream_key(c):
    """everything of a case the oracle's run depends on, but R"""
    return (c["lens"], c["W"], c["H"], c["M"], c["S"], c["f_hi"], c["n_extra"], c["seed"], c["chroma"],
            tuple(c["kinds"]) if c["kinds"] else None, c["family"] == "probe")


def setup(c, R=None):
    """(params, lens table, visits, what must stay alive while they are used)"""
    p, model, table, keep = common.po_setup(c["W"], c["H"], lens=c["lens"], samples_override=c["S"],
                                            vignetting_retries=c["R"] if R is None else R, abb_chromatic=c["chroma"])
    visits, cols = common.make_stream(p, c["W"], c["H"], c["M"], f_hi=c["f_hi"], n_extra=c["n_extra"], seed=c["seed"])
    return p, table, visits, (model, keep, cols)


_ORACLE = {}      # (stream_key, R) -> frame: every run is made once per session and never changed


def oracle(orc, c, R=None):
    """The oracle's frame of the case (at another retry count, if given), computed once."""
    import numpy as np
    import oracle_lib
    R = c["R"] if R is None else R
    key = (stream_key(c), R)
    if key not in _ORACLE:
        p, table, visits, keep = setup(c, R)
        if c["family"] == "probe":
            sphere = np.array(SPHERE, np.float32)
            ref = common.ThreadedOracle(orc, p, table, visits, 4, n_aovs=n_aovs(c), kinds=c["kinds"],
                                        probe=(oracle_lib.sphere_occluder(orc), sphere.ctypes.data))
        else:
            ref = common.run_oracle(orc, p, table, visits, n_aovs=n_aovs(c), kinds=c["kinds"])
        _ORACLE[key] = ref
    return _ORACLE[key]


def sorted_log(ref):
    return common.sort_log(ref.log())
