"""The table of tests/scan_lean.py against the oracle alone -- no GPU: what keeps tests/test_gpu_scan_lean.py from passing
emptily.  Every planted visit the table expects to redistribute does, and has a draw accepted; every vetoed one does not; the
base stream around them redistributes nothing; and the plants sit where their names say: in whole tiles, open groups counted
per tile as the kernel counts them, busy and quiet tiles where the switch cases need them."""
import collections

import numpy as np
import pytest

import scan_lean
import scan_shapes

ALL = scan_lean.CASES + [scan_lean.large_case(M=m) for m in scan_lean.LARGE_M]
_analysed = {}


def _analyse(orc, case):
    if case["name"] not in _analysed:
        built = scan_lean.build(orc, case)
        p, table, visits, cols = built
        ref = scan_shapes.oracle(orc, scan_lean.as_scan_shape(case), built)
        try:
            log = ref.log()
            c = ref.counters()
            _analysed[case["name"]] = (np.unique(log[:, 0]), int(c.redistributed_visits), int(c.visits), int(visits.n),
                                       np.unique(log[:, 2]).size)
        finally:
            ref.close()
    return _analysed[case["name"]]


@pytest.mark.parametrize("case", ALL, ids=[c["name"] for c in ALL])
def test_plants_bite(orc, case):
    drawn, redistributed, seen, n, touched = _analyse(orc, case)
    assert seen == n
    want = [v for v, k in case["plants"] if scan_lean.expect(case, k)]
    veto = [v for v, k in case["plants"] if not scan_lean.expect(case, k)]
    assert want, "a case without a redistributed visit"
    missing = np.setdiff1d(want, drawn)
    assert missing.size == 0, "planted visits without an accepted draw: %s" % missing[:8]
    assert not np.isin(veto, drawn).any(), "vetoed visits with draws: %s" % np.intersect1d(veto, drawn)[:8]
    # nothing but the plants redistributes: the decision the kernel must reproduce is exactly the table's
    assert redistributed == len(want)
    # most pixels are reached by no draw: the bit-for-bit comparison covers them
    assert 2 * touched <= (case["W"] + 1) * (case["H"] + 1)


def _open_groups(case):
    """tile -> groups with an open visit (a closed base: the plants that are not junk; an open base: all of them)"""
    M = case["M"]
    per = collections.defaultdict(set)
    for v, k in case["plants"]:
        if not k.startswith("junk"):
            per[v // (64 * M)].add((v // 64) % M)
    return per


@pytest.mark.parametrize("case", ALL, ids=[c["name"] for c in ALL])
def test_plants_sit_in_whole_tiles(case):
    M = case["M"]
    n_full = case["W"] * case["rows"] // 64
    assert all(v // (64 * M) < n_full for v, _ in case["plants"])


def test_the_table_covers_what_it_is_there_for():
    names = set(scan_lean.BY_NAME)
    for m in (2, 3, 9):
        for tag in ("edges_m%d_64x4", "edges_m%d_64x17", "edges_m%d_65x17", "switch_m%d_64x17", "allopen_m%d_64x17"):
            assert tag % m in names
    for m in (2, 3, 9):
        # lanes 0 and 63, first and last group, first and last tile of a run, the tile before a partial last one
        c = scan_lean.BY_NAME["edges_m%d_65x17" % m]
        open_v = [v for v, k in c["plants"] if k == "open"]
        assert {v % 64 for v in open_v} >= {0, 63}
        assert {(v // 64) % m for v in open_v} >= {0, m - 1}
        tiles = {v // (64 * m) for v in open_v}
        assert {0, 3, 16} <= tiles and 65 * 17 // 64 == 17 and 65 * 17 % 64 != 0
        # a tile with every group open, and tiles with exactly one (the lean body's on-demand fetch, no change of body)
        per = _open_groups(c)
        assert any(len(g) == m for g in per.values()) and any(len(g) == 1 for g in per.values())
        # the switch cases: two busy tiles then at least QUIET_TILES closed ones in the same run's chain, and the reverse
        per = _open_groups(scan_lean.BY_NAME["switch_m%d_64x17" % m])
        busy = sorted(t for t, g in per.items() if len(g) >= scan_lean.BUSY_GROUPS)
        assert busy == [0, 1, 12, 13] and set(per) == set(busy) and scan_lean.QUIET_TILES <= 2
        assert scan_lean.BY_NAME["allopen_m%d_64x17" % m]["base"] == "open"
    kinds = collections.Counter()
    for tag, kw in (("default", {}), ("bidir", "enable_bidir_transmission"), ("skydome", "enable_skydome")):
        for name in ("vetoes_%s" % tag, "vetoes_m2_%s" % tag):
            c = scan_lean.BY_NAME[name]
            assert (c["kw"] == {kw: 1}) if kw else (c["kw"] == {})
            assert {k for _, k in c["plants"]} == {"open", "vi_x", "vi_y", "vi_z", "vi_w", "tr", "far", "far_zero", "band_off", "band_on"}
            kinds.update((k, scan_lean.expect(c, k)) for _, k in c["plants"])
    assert kinds[("tr", True)] and kinds[("tr", False)] and kinds[("far", True)] and kinds[("far", False)]
    assert {k for _, k in scan_lean.BY_NAME["junk"]["plants"]} == {"junk_nan", "junk_pos", "open"}


def test_the_counts_are_the_kernels():
    import ctypes as C
    from pota_amd import capi
    lib = capi.load_library()
    lib.lentil_hip_debug_scan_lean_counts.restype = C.c_int
    out = (C.c_uint32 * 3)()
    assert lib.lentil_hip_debug_scan_lean_counts(out) == 0
    assert (int(out[1]), int(out[2])) == (scan_lean.BUSY_GROUPS, scan_lean.QUIET_TILES)
    assert int(out[0]) == 6          # (M = 9 has a ring shorter than its tile, M = 3 and 2 one as long: the table's two kinds)


@pytest.mark.parametrize("M", scan_lean.LARGE_M)
def test_the_large_frame_gives_a_wave_a_sequence_of_runs(M):
    c = scan_lean.large_case(M=M)
    assert c["M"] == M
    n_full = c["W"] * c["rows"] // 64
    blocks = scan_lean.blocks_of(n_full, c["num_cu"])
    waves, per_chain = scan_lean.chain_runs(n_full, blocks)
    assert per_chain >= 2 and (n_full + 3) // 4 >= 2 * 2 * waves
    per = _open_groups(c)
    # chain 0 and the last chain: first tile, last tile (no next tile), and the first tile of the chain's second run
    for t in (0, waves - 1):
        assert 4 * t in per and 4 * (t + waves) + 3 in per and 4 * (t + waves) in per
    busy = sorted(t for t, g in per.items() if len(g) >= scan_lean.BUSY_GROUPS)
    # chain 5: busy, busy, then closed to the chain's end (six tiles); chain 9: closed first run, then busy, busy
    assert {20, 21, 4 * (9 + waves), 4 * (9 + waves) + 1} <= set(busy)
    assert not any(t in per for t in (22, 23, 36, 37, 38, 39)) and not any(4 * (5 + waves) + k in per for k in range(4))
    # ... so chain 5 is back in the lean body after tile 23, QUIET_TILES tiles behind the last busy one, with a run to go
    assert scan_lean.QUIET_TILES == 2 and per_chain == 2
