"""The aperture-image tables the bokeh sampler is tested with (tests/test_bokeh_table_cases.py: the table against the oracle,
no GPU; tests/test_gpu_bokeh_image.py: the kernels against the oracle).  A plain module: no fixtures, fixed seeds; every table
is generated here, tests/golden/ gains nothing.

bokeh_sample (pota_amd/csrc/lentil_device.h, the reference's imageData::bokehSample) looks a row up in cdfRow, then a column in
that row's slice of cdfColumn, and maps both through rowIndices / columnIndices to a texel.  What it can get wrong, and the case
that is there for it:
  the binary search (upper_bound_f)   sizes 1, 2, 3 (the search's shortest arrays), 8 / 9 and 2047 / 2048 / 2049 (powers of two and
                                      their neighbours), and CDFs with plateaus -- runs of equal values the search must step over:
                                      an image with a black row and a black column (plateaus at the END of the sorted CDFs) and the
                                      crafted "plateau" tables (five equal values at the START and in the MIDDLE, which no image
                                      gives: its probabilities are sorted in descending order)
  the centring, (x - 1) / 2           even sizes against odd ones
  the clamps, r >= y and c >= x       reached only by u >= cdf[last].  An image's CDFs end within an ulp or so of 1, a draw is
                                      below 1: about one draw in 1e7.  The crafted "clamp" tables end their cdfRow at 0.75 and every
                                      row's cdfColumn at 0.5, so a quarter of the draws clamp the row and half of the others the
                                      column; their index arrays are seeded permutations, so that the clamped row and column are
                                      not row or column 0 (an index forgotten, or taken from the wrong array, shows)
  where cdfRow is read from           the solve kernels stage cdfRow in LDS while y <= kMaxBokehRows = 2048 (lentil_kernels.h) and
                                      read global memory above: 2047, 2048 (the last size staged), 2049
  ties in the host's sort             a constant image: every key of every sort is equal
  extreme lx, ly                      an image whose only lit texels are its four corners
  the channel stride                  an image with four channels

A crafted table is no image's: its arrays are made by hand, and both the oracle (orc_bokeh_from_tables) and the HIP library
(lentil_hip_set_bokeh) take them as they are.  Its index arrays are permutations -- rowIndices of 0 ... y - 1, columnIndices of
each row's own texels r * x ... r * x + x - 1 -- so every index the sampler forms stays inside the tables.

Out of scope: an all-black image.  Its total is 0, every probability NaN, and the reference then sorts with a comparator over
NaNs: there is no defined answer to match.
"""
import ctypes as C
import os

import numpy as np

import common
from pota_amd import _abi, bokeh

N_SAMPLES = 20000         # seed pairs per case: the sampler alone, bit for bit
LDS_ROWS = 2048           # kMaxBokehRows (pota_amd/csrc/lentil_kernels.h)
FIXTURE = os.path.join(common.ROOT, "tests", "golden", "example_bokeh_kernel_u8.npy")

# every entry of the list the table is there to cover; each case is the only one to name at least one of them
REQUIRED = (
    ["size:%d" % n for n in (1, 2, 3, 8, 9, 64, 2047, 2048, 2049)] +
    ["image:4-channels", "image:constant", "image:black-row-and-column", "image:corners", "image:fixture"] +
    ["crafted:clamp:16", "crafted:clamp:2049", "crafted:plateau:16", "crafted:plateau:2049"]
)

CASES = []


def _case(name, kind, size, note, covers, channels=3, seed=0, min_points=None):
    """kind: "random" / "constant" / "black_lines" / "corners" / "fixture" (images, through bokeh.build_tables) or "clamp" /
    "plateau" (crafted).  min_points: how many distinct aperture points N_SAMPLES draws must reach at least (the vacuity bar of
    tests/test_bokeh_table_cases.py): (size - 1)^2 / 2 from size 8 on, 2000 for the sizes with more texels than draws -- and what
    the image has for the images that light few texels."""
    if min_points is None:
        min_points = 2000 if size * size > N_SAMPLES else ((size - 1) ** 2 + 1) // 2 if size >= 8 else 1
    CASES.append(dict(name=name, kind=kind, size=size, channels=channels, seed=seed, note=note, covers=tuple(covers),
                      min_points=min_points, crafted=kind in ("clamp", "plateau")))


for _n in (1, 2, 3, 8, 9, 64, 2047, 2048, 2049):
    _case("size%d" % _n, "random", _n, {1: "the shortest search: one row, one column", 2: "the smallest even size: (x - 1) / 2 == 0",
                                        3: "the smallest odd size with a centre", 8: "a power of two, even centring",
                                        9: "odd centring beside size 8", 64: "more texels than any smaller case, fewer than draws",
                                        2047: "one below the LDS limit, odd", 2048: "y == kMaxBokehRows: the last size staged in LDS",
                                        2049: "y > kMaxBokehRows: cdfRow read from global memory"}[_n],
          ["size:%d" % _n], seed=0xB0CE + _n)
_case("rgba9", "random", 9, "four channels: the luminance strides over alpha", ["image:4-channels"], channels=4, seed=0xA1FA)
_case("constant8", "constant", 8, "every sort key ties", ["image:constant"])
_case("blacklines12", "black_lines", 12, "row 4 and column 7 black: plateaus at the end of cdfRow and of every cdfColumn",
      ["image:black-row-and-column"], seed=0xB1AC, min_points=61)           # 11 x 11 lit texels: half of them
_case("corners10", "corners", 10, "the four corners alone are lit: the extreme lx, ly of an even size", ["image:corners"], min_points=4)
_case("fixture", "fixture", 250, "the reference's example kernel, the one image every earlier test uses", ["image:fixture"])
for _n in (16, 2049):
    _case("clamp%d" % _n, "clamp", _n, "cdfRow ends at 0.75, every cdfColumn at 0.5; permuted indices", ["crafted:clamp:%d" % _n], seed=0xC1A0 + _n)
    _case("plateau%d" % _n, "plateau", _n, "five equal CDF values at the start and in the middle of cdfRow and of every cdfColumn",
          ["crafted:plateau:%d" % _n], seed=0x91A7 + _n,
          # (at size 16 nine of the sixteen positions of every CDF have no probability: 7 x 7 texels can be drawn, and all must be)
          min_points=49 if _n == 16 else None)

BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)

CLAMP_ROW_END, CLAMP_COLUMN_END = 0.75, 0.5
PLATEAU = 5               # equal consecutive CDF values in a plateau


def texels(case):
    """float32 [size, size, channels]: the image of an image case, as AiTextureLoad would deliver it"""
    n, kind = case["size"], case["kind"]
    if kind == "fixture":
        return np.load(FIXTURE).astype(np.float32) / np.float32(255)
    rng = np.random.default_rng(case["seed"])
    if kind == "random":
        return rng.random((n, n, case["channels"]), dtype=np.float32)
    if kind == "constant":
        return np.full((n, n, 3), 0.25, np.float32)
    if kind == "black_lines":
        t = (rng.random((n, n, 3), dtype=np.float32) * np.float32(0.9) + np.float32(0.1))
        t[4, :, :] = 0.0
        t[:, 7, :] = 0.0
        return t
    if kind == "corners":
        t = np.zeros((n, n, 3), np.float32)
        t[0, 0], t[0, n - 1], t[n - 1, 0], t[n - 1, n - 1] = 1.0, 0.5, 0.25, 0.75
        return t
    raise ValueError(kind)


def _permuted_indices(rng, n):
    """rowIndices: a permutation of the rows; columnIndices: for every row a permutation of its own texels r * n ... r * n + n - 1.
    Neither ends on row / column 0: what a clamp selects is the LAST entry."""
    rows = rng.permutation(n).astype(np.int32)
    cols = rng.permuted(np.tile(np.arange(n, dtype=np.int32), (n, 1)), axis=1)
    if n > 1:
        if rows[-1] == 0:
            rows[[0, -1]] = rows[[-1, 0]]
        z = np.flatnonzero(cols[:, -1] == 0)
        cols[z, -1], cols[z, 0] = cols[z, 0], 0
    cols = cols + (np.arange(n, dtype=np.int32) * n)[:, None]
    return rows, np.ascontiguousarray(cols.reshape(-1))


def plateau_cdf(n):
    """float32 [n]: a CDF that ends at exactly 1 with PLATEAU equal values at its start (all 0: increments 0 ... PLATEAU - 1 are
    zero) and PLATEAU in its middle (increments n // 2 ... n // 2 + PLATEAU - 2 are zero); strictly increasing elsewhere"""
    w = np.ones(n, np.float64)
    w[:PLATEAU] = 0.0
    w[n // 2:n // 2 + PLATEAU - 1] = 0.0
    cdf = (np.cumsum(w) / w.sum()).astype(np.float32)
    cdf[-1] = 1.0
    return cdf


def zero_increments(cdf):
    """positions of a CDF (a row of them: along the last axis) whose increment is zero: no draw may select them"""
    c = np.asarray(cdf, np.float32)
    return np.diff(c, prepend=np.float32(0.0), axis=-1) == 0


def _crafted(case):
    n = case["size"]
    rng = np.random.default_rng(case["seed"])
    rows, cols = _permuted_indices(rng, n)
    if case["kind"] == "clamp":
        ramp = np.arange(1, n + 1, dtype=np.float64) / n
        cdf_row, cdf_col = (CLAMP_ROW_END * ramp).astype(np.float32), (CLAMP_COLUMN_END * ramp).astype(np.float32)
    else:
        cdf_row = cdf_col = plateau_cdf(n)
    return dict(x=n, y=n, cdfRow=np.ascontiguousarray(cdf_row), rowIndices=rows,
                cdfColumn=np.ascontiguousarray(np.tile(cdf_col, n)), columnIndices=cols)


_built = {}


def tables(name):
    """the case's four tables: dict x, y, cdfRow, rowIndices, cdfColumn, columnIndices (numpy; built once per process and never
    written to -- the 2049 x 2049 ones are 34 MB each)"""
    if name not in _built:
        case = BY_NAME[name]
        t = _crafted(case) if case["crafted"] else bokeh.build_tables(texels(case))
        n = case["size"]
        assert t["x"] == t["y"] == n
        # every index the sampler can form stays inside the tables
        assert np.array_equal(np.sort(t["rowIndices"]), np.arange(n))
        ci = t["columnIndices"].reshape(n, n)
        assert np.array_equal(np.sort(ci, axis=1), np.arange(n * n, dtype=np.int64).reshape(n, n))
        for a in t.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _built[name] = t
    return _built[name]


def abi_table(t):
    """an _abi.BokehTable over the arrays of `t` (which must outlive it)"""
    bt = _abi.BokehTable()
    bt.x, bt.y = int(t["x"]), int(t["y"])
    for k in ("cdfRow", "rowIndices", "cdfColumn", "columnIndices"):
        setattr(bt, k, t[k].ctypes.data)
    return bt


def get(name):
    """(tables, _abi.BokehTable, note)"""
    t = tables(name)
    return t, abi_table(t), BY_NAME[name]["note"]


def oracle_bokeh(orc, name):
    """the oracle's OrcBokeh over the case's tables (orc_bokeh_destroy it)"""
    bt = abi_table(tables(name))
    return orc.orc_bokeh_from_tables(C.byref(bt))


def seed_pairs():
    """the N_SAMPLES (a, b) pairs orc_po_aperture_sample / lentil_hip_test_aperture_sample are called with: a pixel hash and an
    attempt number, as a pass forms them"""
    rng = np.random.default_rng(0xA9E7)
    a = rng.integers(0, 2 ** 32, N_SAMPLES, dtype=np.uint64).astype(np.uint32)
    b = rng.integers(0, 4000, N_SAMPLES, dtype=np.uint64).astype(np.uint32)
    return a, b


def sampler_params():
    """the camera the sampler alone is run with: polynomial optics, the image on, no blades"""
    p, model, table, keep = common.po_setup(64, 48, bokeh_enable_image=1)
    assert p.bokeh_aperture_blades <= 2 and p.enable_dof
    return p


_sampled = {}


def oracle_samples(orc, name):
    """fp64 [N_SAMPLES, 2]: orc_po_aperture_sample over seed_pairs() with the case's tables (computed once, never written to)"""
    if name not in _sampled:
        p = sampler_params()
        ob = oracle_bokeh(orc, name)
        a, b = seed_pairs()
        out = np.empty((a.shape[0], 2))
        tmp = (C.c_double * 2)()
        try:
            for i, (sa, sb) in enumerate(zip(a.tolist(), b.tolist())):
                orc.orc_po_aperture_sample(C.byref(p), ob, sa, sb, tmp)
                out[i] = tmp[0], tmp[1]
        finally:
            orc.orc_bokeh_destroy(ob)
        out.setflags(write=False)
        _sampled[name] = out
    return _sampled[name]


def texel_of(samples, n, aperture_radius):
    """(row, column) of the texel each aperture point came from: bokeh_sample's last lines undone.  lx = (column - (n - 1) / 2) /
    n * 2 and ly = -(row - (n - 1) / 2) / n * 2 in float32, times the aperture radius: the quotients are off an integer by some
    1e-7 * n, far from the 0.5 that would round elsewhere."""
    u = np.asarray(samples, np.float64) / float(aperture_radius)
    col = np.rint(u[:, 0] * n / 2.0).astype(np.int64) + (n - 1) // 2
    row = np.rint(-u[:, 1] * n / 2.0).astype(np.int64) + (n - 1) // 2
    assert (np.abs(u[:, 0] * n / 2.0 - np.rint(u[:, 0] * n / 2.0)) < 0.01).all()
    assert (np.abs(u[:, 1] * n / 2.0 - np.rint(u[:, 1] * n / 2.0)) < 0.01).all()
    return row, col
