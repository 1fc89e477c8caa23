"""The table of scan shapes (tests/scan_shapes.py) against the oracle alone -- no GPU: what keeps tests/test_gpu_scan_shapes.py
from passing emptily.  Every planted highlight is redistributed and has a draw accepted; most of each stream's pixels are
reached by no draw, so the bit-for-bit comparison there covers them; among those are pixels with flagged visits of their own
(their weight is that of M - skipped visits); every scan kernel is some case's expectation; every entry of the list the table
was written from is named by a case, and every case is the only one to name one of them."""
import collections

import numpy as np
import pytest

import scan_shapes
from pota_amd import capi

_analysed = {}


def _analyse(orc, case):
    """(planted visits without an accepted draw, pixels holding visits, ... of them undrawn, ... of them with flagged visits of their own)"""
    if case["name"] not in _analysed:
        built = scan_shapes.build(case)
        p, table, visits, cols = built
        ref = scan_shapes.oracle(orc, case, built)
        try:
            log = ref.log()
            assert int(ref.counters().visits) == int(visits.n)
        finally:
            ref.close()
        flagged = np.unique(log[:, 0])
        owner = scan_shapes.stream_pixels(case, cols)
        holding = np.unique(owner)
        undrawn = np.setdiff1d(holding, np.unique(log[:, 2]))
        own_flagged = np.intersect1d(np.unique(owner[flagged]), undrawn)
        _analysed[case["name"]] = (np.setdiff1d(cols["planted"], flagged), holding.size, undrawn.size, own_flagged.size)
    return _analysed[case["name"]]


@pytest.mark.parametrize("case", scan_shapes.CASES, ids=[c["name"] for c in scan_shapes.CASES])
def test_case_is_not_empty(orc, case):
    missing, holding, undrawn, own_flagged = _analyse(orc, case)
    assert missing.size == 0, "planted visits without an accepted draw: %s" % missing[:8]
    assert 2 * undrawn >= holding, "%d of %d pixels with visits are reached by no draw" % (undrawn, holding)
    if case["K"] == 0:
        assert own_flagged >= 1, "no undrawn pixel has a flagged visit of its own"


def test_groups_keep_skipped_weights_in_the_bit_exact_set(orc):
    """(the cases with extra AOVs: across each group's cases)"""
    groups = collections.Counter()
    for c in scan_shapes.CASES:
        groups[c["group"]] += _analyse(orc, c)[3]
    for group, n in sorted(groups.items()):
        assert n >= 1, group


def test_every_scan_kernel_is_expected_by_a_case():
    assert set(c["expect_kernel"] for c in scan_shapes.CASES) == set(capi.SCAN_NAMES)


def test_every_entry_is_covered_and_every_case_needed():
    named = collections.Counter(t for c in scan_shapes.CASES for t in c["covers"])
    assert set(named) == set(scan_shapes.REQUIRED), (sorted(set(scan_shapes.REQUIRED) - set(named)), sorted(set(named) - set(scan_shapes.REQUIRED)))
    assert len(set(scan_shapes.REQUIRED)) == len(scan_shapes.REQUIRED)
    for c in scan_shapes.CASES:
        assert any(named[t] == 1 for t in c["covers"]), "%s is the only cover of nothing" % c["name"]
    assert 60 <= len(scan_shapes.CASES) <= 80


def test_regions_and_tails_are_what_the_names_say():
    by = scan_shapes.BY_NAME
    for name, tiles, tail in (("beauty_64x3", 3, 0), ("beauty_65x3", 3, 3), ("beauty_63x1", 0, 63), ("beauty_37x7", 4, 3),
                              ("beauty_127x5", 9, 59), ("beauty_129x17", 34, 17), ("beauty_331x173", 894, 47)):
        x0, y0, ppr, rows, rs = by[name]["region"]
        assert divmod(ppr * rows, 64) == (tiles, tail), name
    for c in scan_shapes.CASES:
        x0, y0, ppr, rows, rs = c["region"]
        if c["name"].endswith("_exact") and c["name"].startswith("multi"):
            assert (ppr * rows) % c["ppt"] == 0
        if c["name"].endswith("_tail") and c["name"].startswith("multi") or c["name"].startswith("closest"):
            assert (ppr * rows) % c["ppt"] != 0 or c["ppt"] == 1
        if c["v_end"] is not None and c["M"]:
            assert c["v_end"] % c["M"] != 0
    # the four buckets tile their frame
    cover = np.zeros((48, 64), int)
    for b in scan_shapes.BUCKETS:
        x0, y0, ppr, rows, rs = by[b]["region"]
        cover[y0:y0 + rows, x0:x0 + ppr] += 1
    assert (cover == 1).all()
