"""The table of aperture-image cases (tests/bokeh_tables.py) against the oracle alone -- no GPU: what keeps
tests/test_gpu_bokeh_image.py from passing emptily, and the host library's tables against the oracle's.

For the seed pairs the GPU test uses: the crafted "clamp" tables do clamp (a quarter of the draws on the last row, half of the
others on their row's last column), the plateau tables' zero-probability rows and columns are never drawn, every size spreads
its draws over many texels; every entry of the list the table was written from is named by a case, and every case is the only
one to name one of them."""
import collections

import numpy as np
import pytest

import bokeh_tables
from pota_amd import _abi, bokeh

IMAGE_CASES = [c for c in bokeh_tables.CASES if not c["crafted"]]
IDS = [c["name"] for c in bokeh_tables.CASES]


def _oracle_tables(orc, tex):
    y, x, nch = tex.shape
    B = orc.orc_bokeh_create(tex.ctypes.data, x, y, nch)
    assert B
    out = dict(cdfRow=np.empty(y, np.float32), rowIndices=np.empty(y, np.int32), cdfColumn=np.empty(x * y, np.float32),
               columnIndices=np.empty(x * y, np.int32))
    orc.orc_bokeh_tables(B, *[out[k].ctypes.data for k in ("cdfRow", "rowIndices", "cdfColumn", "columnIndices")])
    orc.orc_bokeh_destroy(B)
    return out


@pytest.mark.parametrize("case", IMAGE_CASES, ids=[c["name"] for c in IMAGE_CASES])
def test_host_tables_equal_the_oracles(orc, case):
    """lentil_host_bokeh_probability against orc_bokeh_create, all four tables bit for bit.  (Both sort with std::sort and a
    comparator over the same fp32 keys; a difference here would be one of sort order among ties.)"""
    tex = np.ascontiguousarray(bokeh_tables.texels(case))
    assert tex.shape == (case["size"], case["size"], case["channels"])
    t = bokeh_tables.tables(case["name"])
    want = _oracle_tables(orc, tex)
    for k in ("cdfRow", "rowIndices", "cdfColumn", "columnIndices"):
        assert np.array_equal(t[k].view(np.uint32), want[k].view(np.uint32)), k
    # ... and they are a distribution: CDFs that end at 1 (fp32 sums: to a few ulps per addend)
    n = case["size"]
    assert np.all(np.diff(t["cdfRow"]) >= 0) and abs(float(t["cdfRow"][-1]) - 1.0) < 1e-6 * n * n


def test_every_entry_is_covered_and_every_case_needed():
    named = collections.Counter(t for c in bokeh_tables.CASES for t in c["covers"])
    assert set(named) == set(bokeh_tables.REQUIRED), (sorted(set(bokeh_tables.REQUIRED) - set(named)), sorted(set(named) - set(bokeh_tables.REQUIRED)))
    assert len(set(bokeh_tables.REQUIRED)) == len(bokeh_tables.REQUIRED)
    for c in bokeh_tables.CASES:
        assert any(named[t] == 1 for t in c["covers"]), "%s is the only cover of nothing" % c["name"]
        assert c["note"]
    assert 15 <= len(bokeh_tables.CASES) <= 24


def test_sizes_sit_on_both_sides_of_the_lds_limit():
    sizes = set(c["size"] for c in bokeh_tables.CASES)
    assert {bokeh_tables.LDS_ROWS - 1, bokeh_tables.LDS_ROWS, bokeh_tables.LDS_ROWS + 1} <= sizes
    assert any(c["size"] > bokeh_tables.LDS_ROWS for c in bokeh_tables.CASES if c["crafted"])
    assert any(c["size"] % 2 == 0 for c in bokeh_tables.CASES) and any(c["size"] % 2 for c in bokeh_tables.CASES)
    with open(bokeh_tables.common.ROOT + "/pota_amd/csrc/lentil_kernels.h") as f:
        assert "constexpr int kMaxBokehRows = %d;" % bokeh_tables.LDS_ROWS in f.read()


def test_get_yields_tables_an_abi_table_and_a_note():
    for c in bokeh_tables.CASES:
        if c["size"] > 250:
            continue
        t, bt, note = bokeh_tables.get(c["name"])
        assert isinstance(bt, _abi.BokehTable) and (bt.x, bt.y) == (c["size"], c["size"]) and note == c["note"]
        assert bt.cdfRow == t["cdfRow"].ctypes.data and bt.columnIndices == t["columnIndices"].ctypes.data
        assert t["cdfRow"].dtype == t["cdfColumn"].dtype == np.float32 and t["rowIndices"].dtype == t["columnIndices"].dtype == np.int32
        assert t["cdfRow"].shape == (c["size"],) and t["cdfColumn"].shape == t["columnIndices"].shape == (c["size"] ** 2,)


def _texels_drawn(orc, case):
    s = bokeh_tables.oracle_samples(orc, case["name"])
    assert s.shape == (bokeh_tables.N_SAMPLES, 2)
    return bokeh_tables.texel_of(s, case["size"], bokeh_tables.sampler_params().aperture_radius)


@pytest.mark.parametrize("case", bokeh_tables.CASES, ids=IDS)
def test_draws_stay_inside_and_spread(orc, case):
    n = case["size"]
    row, col = _texels_drawn(orc, case)
    assert row.min() >= 0 and row.max() < n and col.min() >= 0 and col.max() < n
    points = np.unique(row * n + col).size
    assert points >= case["min_points"], "%d distinct aperture points, %d asked for" % (points, case["min_points"])
    if n >= 8 and (case["kind"] in ("random", "clamp") or case["name"] == "plateau2049"):
        assert case["min_points"] >= min(2000, (n - 1) ** 2 / 2.0)


@pytest.mark.parametrize("name", ["clamp16", "clamp2049"])
def test_clamp_tables_clamp(orc, name):
    """cdfRow ends at 0.75, every cdfColumn at 0.5: a quarter of the draws take the clamped (last) row, half of the others
    their row's clamped column -- and neither is row / column 0.  (20 000 draws: the shares' standard errors are 0.3 % and
    0.4 %; at size 16 the last entry's own interval adds 0.75 / 16 and 0.5 / 16.)"""
    case = bokeh_tables.BY_NAME[name]
    t = bokeh_tables.tables(name)
    n = case["size"]
    assert float(t["cdfRow"][-1]) == bokeh_tables.CLAMP_ROW_END
    assert np.all(t["cdfColumn"].reshape(n, n)[:, -1] == np.float32(bokeh_tables.CLAMP_COLUMN_END))
    last_row = int(t["rowIndices"][-1])
    last_col = t["columnIndices"].reshape(n, n)[:, -1].astype(np.int64) - np.arange(n) * n
    assert last_row != 0 and np.all(last_col != 0) and np.all((last_col > 0) & (last_col < n))
    assert not np.array_equal(t["rowIndices"], np.arange(n))
    row, col = _texels_drawn(orc, case)
    on_row = row == last_row
    share = float(on_row.mean())
    assert 0.15 <= share <= 0.35, share
    rest = ~on_row
    on_col = col[rest] == last_col[row[rest]]
    share_col = float(on_col.mean())
    assert 0.40 <= share_col <= 0.60, share_col


@pytest.mark.parametrize("name", ["plateau16", "plateau2049", "blacklines12"])
def test_zero_probability_rows_and_columns_are_never_drawn(orc, name):
    case = bokeh_tables.BY_NAME[name]
    t = bokeh_tables.tables(name)
    n = case["size"]
    dead_pos = bokeh_tables.zero_increments(t["cdfRow"])
    dead_rows = t["rowIndices"][dead_pos]
    dead_cols = bokeh_tables.zero_increments(t["cdfColumn"].reshape(n, n))                 # [row, position in the row's CDF]
    if case["crafted"]:
        # the plateaus are where the case says: five equal values at the start and five in the middle
        c = t["cdfRow"]
        assert np.all(c[:bokeh_tables.PLATEAU] == 0) and c[bokeh_tables.PLATEAU] > 0
        mid = c[n // 2 - 1:n // 2 + bokeh_tables.PLATEAU - 1]
        assert mid.size == bokeh_tables.PLATEAU and np.all(mid == mid[0]) and c[n // 2 + bokeh_tables.PLATEAU - 1] > mid[0] > c[n // 2 - 2]
        assert int(dead_pos.sum()) == 2 * bokeh_tables.PLATEAU - 1 and float(c[-1]) == 1.0
        assert np.all(dead_cols.sum(axis=1) == 2 * bokeh_tables.PLATEAU - 1)
    else:
        assert list(dead_rows) == [4] and int(dead_pos.sum()) == 1
    row, col = _texels_drawn(orc, case)
    assert not np.isin(row, dead_rows).any()
    # the position of each drawn texel in its row's columnIndices
    ci = t["columnIndices"].reshape(n, n).astype(np.int64) - (np.arange(n) * n)[:, None]
    pos_of = np.empty((n, n), np.int64)
    np.put_along_axis(pos_of, ci, np.broadcast_to(np.arange(n), (n, n)), axis=1)
    assert not dead_cols[row, pos_of[row, col]].any()
    if not case["crafted"]:
        assert not (col == 7).any()


def test_corners_reach_the_extreme_points(orc):
    case = bokeh_tables.BY_NAME["corners10"]
    row, col = _texels_drawn(orc, case)
    n = case["size"]
    assert set(zip(row.tolist(), col.tolist())) == {(0, 0), (0, n - 1), (n - 1, 0), (n - 1, n - 1)}
    s = bokeh_tables.oracle_samples(orc, "corners10") / bokeh_tables.sampler_params().aperture_radius
    # an even size is not centred: (x - 1) / 2 == 4 of 10 leaves -0.8 ... 1.0
    assert s[:, 0].min() == np.float32(-4.0) / np.float32(10.0) * 2.0 and s[:, 0].max() == np.float32(5.0) / np.float32(10.0) * 2.0
    assert s[:, 1].max() == np.float32(4.0) / np.float32(10.0) * 2.0 and s[:, 1].min() == np.float32(-5.0) / np.float32(10.0) * 2.0


def test_refused_images(orc):
    """a non-square image, fewer than three channels, a null array and x <= 0: neither side makes tables of them"""
    host = bokeh.load_host_library()
    outs = [np.empty(64, np.float32), np.empty(64, np.int32), np.empty(64, np.float32), np.empty(64, np.int32)]
    ptrs = [o.ctypes.data for o in outs]
    with pytest.raises(ValueError):
        bokeh.build_tables(np.ones((4, 5, 3), np.float32))
    with pytest.raises(ValueError):
        bokeh.build_tables(np.ones((4, 4, 2), np.float32))
    with pytest.raises(ValueError):
        bokeh.build_tables(np.ones((0, 0, 3), np.float32))
    tex = np.ones((4, 4, 3), np.float32)
    assert host.lentil_host_bokeh_probability(None, 4, 4, 3, *ptrs) != 0
    assert host.lentil_host_bokeh_probability(tex.ctypes.data, 0, 0, 3, *ptrs) != 0
    assert host.lentil_host_bokeh_probability(tex.ctypes.data, -4, -4, 3, *ptrs) != 0
    assert host.lentil_host_bokeh_probability(tex.ctypes.data, 4, 4, 3, *ptrs) == 0
    wide = np.ones((4, 5, 3), np.float32)
    assert not orc.orc_bokeh_create(wide.ctypes.data, 5, 4, 3)
    assert not orc.orc_bokeh_create(tex.ctypes.data, 4, 4, 2)
    assert not orc.orc_bokeh_create(None, 4, 4, 3)
    assert not orc.orc_bokeh_create(tex.ctypes.data, 0, 0, 3)
    assert not orc.orc_bokeh_create(tex.ctypes.data, -4, -4, 3)
    B = orc.orc_bokeh_create(tex.ctypes.data, 4, 4, 3)
    assert B
    orc.orc_bokeh_destroy(B)
