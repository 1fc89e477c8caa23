"""The table of cryptomatte shapes (tests/crypto_cases.py) against the oracle alone -- no GPU: what keeps
tests/test_gpu_crypto_shapes.py from passing emptily.  Per case what the case claims: its tiles and tail, the kernel the LDS
formula predicts, draws where draws are wanted and none where "direct-only" is claimed, the largest id count against the
table's width, ids that leave and re-enter a two-entry cache, exact ties, the share of ranked pixels the near-tie rule of
compare_ranks leaves out (at most 5 %), and -- the model the overflow case is judged by -- a pixel's own visits added one
after the other in fp32 equal the oracle bit for bit wherever no draw lands."""
import collections
import re

import numpy as np
import pytest

import crypto_cases as cc
import scan_shapes
from test_crypto import near_tie

SKIP_CAP = 0.05
_analysed = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _highlights(b):
    return scan_shapes.is_generated_highlight(b["cols"])


def _own_visits(case, b, hi):
    """frame pixel -> the visits of the stream that stay in it, in stream order"""
    own = collections.defaultdict(list)
    for v in np.flatnonzero(~hi):
        own[int(b["pix"][v])].append(int(v))
    return own


def _model_equals_oracle(case, b, fr, pixels, own, passes=1):
    for pix in pixels:
        for a in range(cc.N_CRYPTO):
            keys, sums, total, full = cc.own_visits_model(case, b, a, own.get(int(pix), []) * passes)
            rk, rw, rtot = fr.crypto_pixel(a, int(pix))
            order = np.argsort(np.array(keys, np.uint32).view(np.float32), kind="stable") if keys else []
            mk = np.array(keys, np.uint32).view(np.float32)[order] if keys else np.empty(0, np.float32)
            mw = np.array(sums, np.float32)[order] if keys else np.empty(0, np.float32)
            assert full == 0 and mk.shape == rk.shape and np.array_equal(mk, rk), (case["name"], pix, a)
            assert np.array_equal(_bits(mw), _bits(rw)) and _bits(total) == _bits(np.float32(rtot)), (case["name"], pix, a)


def _analyse(orc, case):
    if case["name"] in _analysed:
        return _analysed[case["name"]]
    b = cc.build(case)
    fr = cc.oracle_frame(orc, case, b)
    try:
        rc, log, np_ = fr.counters(), fr.log(), fr.np
        assert int(rc.visits) == b["n"] == cc.n_visits(case)
        hi = _highlights(b)
        assert int(hi.sum()) == int(rc.redistributed_visits)          # the generator's highlights are the redistributed visits
        assert np.isin(np.unique(log[:, 0]), np.flatnonzero(hi)).all()
        counts = np.array([[len(fr.crypto_pixel(a, p)[0]) for p in range(np_)] for a in range(cc.N_CRYPTO)])
        ranked = skipped = 0
        for a in range(cc.N_CRYPTO):
            for rank in case["ranks"]:
                rout, rhas = fr.crypto_rank(a, rank)
                assert np.array_equal(rhas, counts[a] > rank)
                for pix in np.flatnonzero(rhas):
                    k, w, tot = fr.crypto_pixel(a, int(pix))
                    ranked += 1
                    skipped += near_tie(w, tot, rank)
        holding = np.unique(b["pix"])
        undrawn = np.setdiff1d(holding, np.unique(log[:, 2]))
        own = _own_visits(case, b, hi)
        if case["columns"] != "overflow":
            some = np.unique(np.concatenate([undrawn[::max(1, undrawn.size // 200)], undrawn[-8:]])) if undrawn.size else undrawn
            _model_equals_oracle(case, b, fr, some, own)
        res = dict(b=b, rc=(int(rc.redistributed_visits), int(rc.accepted_draws)), log=log, counts=counts, ranked=ranked, skipped=skipped,
                   holding=holding, undrawn=undrawn, own=own, hi=hi)
    finally:
        fr.close()
    _analysed[case["name"]] = res
    return res


@pytest.mark.parametrize("case", cc.CASES, ids=[c["name"] for c in cc.CASES])
def test_case_is_what_it_claims(orc, case):
    r = _analyse(orc, case)
    red, acc = r["rc"]
    if case["direct_only"]:
        assert (red, acc) == (0, 0) and r["log"].shape[0] == 0
        assert r["undrawn"].size == r["holding"].size
    elif case["wants_draws"]:
        assert red > 0 and acc > 0
    assert r["undrawn"].size >= 1 or r["holding"].size == 1
    mx = int(r["counts"].max())
    if case["columns"] == "overflow":
        assert mx == case["S"] + 2
    elif case["name"].startswith("slots_exactly_full") or case["columns"] == "single":
        assert mx == case["S"]
    else:
        assert mx <= case["S"]
    share = r["skipped"] / max(r["ranked"], 1)
    print(case["name"], "tiles, tail", cc.tiles_and_tail(case), "kernel", cc.expect_kernel(case), "redistributed", red, "accepted", acc,
          "most ids", mx, "of", case["S"], "ranked", r["ranked"], "near ties %.2f %%" % (100 * share))
    assert r["ranked"] > 0
    if not case["direct_only"]:          # (the direct-only cases' ranks are compared bit for bit on every pixel: nothing is left out)
        assert share <= SKIP_CAP


def test_every_entry_is_covered():
    named = collections.Counter(t for c in cc.CASES for t in c["covers"])
    assert set(named) | set(cc.COVERED_ELSEWHERE) == set(cc.REQUIRED)
    assert len(set(cc.REQUIRED)) == len(cc.REQUIRED)
    for c in cc.CASES:
        assert c["covers"] or c["name"] in cc.BUCKETS, c["name"]
    for child in cc.CHILDREN.values():
        for word in re.findall(r"[a-z_0-9]+", child["select"]):
            assert word in ("and", "or", "test_crypto_shape", "test_buckets_into_one_frame") or word in cc.BY_NAME, word


def test_tiles_and_tails_are_what_the_names_say():
    for n, _ in cc.TAILS:
        for m in (1, 2, 9):
            c = cc.BY_NAME["tail_%d_m%d" % (n, m)]
            assert cc.tiles_and_tail(c) == divmod(n, 128) and cc.n_visits(c) == n * m
            assert cc.expect_kernel(c) == (cc.TILE, 1)
    # the column loads of a tile: 16 bytes per lane where the tile's pairs are a multiple of four and begin at one
    E = 3
    assert all((127 * m * E) & 3 for m in (1, 2, 9))                               # 127 pixels: the scalar load
    assert all((4 * m * E) & 3 == 0 and (128 * m * E) & 3 == 0 for m in (1, 2, 9))  # 132: the float4 load in a 4-pixel tile
    assert any((3 * m * E) & 3 for m in (1, 2, 9))                                 # 259: a 3-pixel tail
    assert cc.tiles_and_tail(cc.BY_NAME["lazy_whole"]) == (11, 80)
    assert cc.tiles_and_tail(cc.BY_NAME["grid_stride"]) == (302, 5)
    assert cc.tiles_and_tail(cc.BY_NAME["thinlens_tail"])[1] and cc.tiles_and_tail(cc.BY_NAME["chunked"])[1]
    assert cc.n_visits(cc.BY_NAME["truncated"]) % 9 == 8 and cc.n_visits(cc.BY_NAME["overflow_atomic"]) % 9 == 8


def test_kernels_follow_the_lds_formula():
    for M in range(1, 20):
        assert cc.tile_words(M, 3, 16) == 896 * M + 4608
    want = {"lds_m13": cc.TILE, "lds_m14": cc.OWNER, "lds_e1": cc.TILE, "lds_e64_s64": cc.OWNER, "lds_e4_s32_m6": cc.TILE, "lds_e4_s32_m7": cc.OWNER,
            "many20": cc.TILE, "many40": cc.OWNER, "truncated": cc.ATOMIC, "overflow_atomic": cc.ATOMIC}
    for name, k in want.items():
        assert cc.expect_kernel(cc.BY_NAME[name])[0] == k, name
    assert all(cc.tile_words(M, 64, 64) > 16384 for M in range(1, 4))
    for c in cc.CASES:
        k, variant = cc.expect_kernel(c)
        if c["name"].endswith("_tile"):
            assert k == cc.TILE, c["name"]
        if c["name"].endswith("_owner") or c["name"].endswith("_default"):
            assert k == cc.OWNER, c["name"]
        assert variant == (2 if c["name"] == "lazy_whole" else 1 if k == cc.TILE else 0)
    assert cc.expect_flushed(cc.BY_NAME["lazy_flush_region"]) and cc.expect_flushed(cc.BY_NAME["lazy_flush_slots5"])
    assert not cc.expect_flushed(cc.BY_NAME["lazy_whole"]) and not cc.expect_flushed(cc.BY_NAME["accumulate"])
    # both sides of a tile: exactly 64 KiB is taken, a word more is not
    assert cc.tile_words(13, 3, 16) * 4 <= 65536 < cc.tile_words(14, 3, 16) * 4
    assert cc.tile_words(6, 4, 32) * 4 <= 65536 < cc.tile_words(7, 4, 32) * 4


def test_accumulate_is_two_oracle_passes_into_one_frame(orc):
    case = cc.BY_NAME["accumulate"]
    r = _analyse(orc, case)
    fr = cc.oracle_frame(orc, case, r["b"], passes=2)
    try:
        rc = fr.counters()
        assert (int(rc.redistributed_visits), int(rc.accepted_draws)) == (2 * r["rc"][0], 2 * r["rc"][1])
        some = r["undrawn"][::7]
        assert some.size > 50
        _model_equals_oracle(case, r["b"], fr, some, r["own"], passes=2)
    finally:
        fr.close()


def test_buckets_tile_the_frame_and_draws_cross_them(orc):
    cover = np.zeros((48, 64), int)
    crossing = 0
    for name in cc.BUCKETS:
        case = cc.BY_NAME[name]
        x0, y0, ppr, rows, rs = case["region"]
        cover[y0:y0 + rows, x0:x0 + ppr] += 1
        r = _analyse(orc, case)
        crossing += int((~np.isin(r["log"][:, 2], r["holding"])).sum())
    assert (cover == 1).all()
    assert crossing > 20, crossing


def test_the_oracle_takes_a_stream_over_the_whole_buffers(orc):
    for name in ("lazy_whole", "lazy_flush_slots5"):
        case = cc.BY_NAME[name]
        r = _analyse(orc, case)
        p = r["b"]["p"]
        assert int(r["b"]["visits"].pixels_per_row) == int(p.xres) and r["holding"].size == int(p.xres) * int(p.yres)
        fr = cc.oracle_frame(orc, case, r["b"])
        try:
            last = int(p.xres) * int(p.yres) - 1
            assert fr.crypto_pixel(0, last)[2] > 0 or r["hi"][-case["M"]:].all()
            assert (r["counts"][0].reshape(int(p.yres), int(p.xres))[:, -1] > 0).any()
        finally:
            fr.close()


def test_rotating_ids_leave_two_registers_and_come_back(orc):
    for name in ("rotate_e1_tile", "rotate_e3_tile"):
        case = cc.BY_NAME[name]
        r = _analyse(orc, case)
        back = sum(cc.reenters_two_registers(case, r["b"], a, vs) for vs in r["own"].values() for a in range(cc.N_CRYPTO))
        assert back >= len(r["own"]), (name, back)
        # +0.0 and -0.0 in different visits of one pixel: one key
        h = r["b"]["hashes"][0]
        zeros = _bits(h)[h == 0.0]
        assert (zeros == 0).any() and (zeros == 0x80000000).any()


def test_ties_are_exact_and_the_oracle_keeps_them_in_id_order(orc):
    case = cc.BY_NAME["ties"]
    r = _analyse(orc, case)
    fr = cc.oracle_frame(orc, case, r["b"])
    try:
        tied = three = four = 0
        for pix in r["holding"]:
            for a in range(cc.N_CRYPTO):
                k, w, tot = fr.crypto_pixel(a, int(pix))
                order = [fr.crypto_rank(a, rank)[0][pix] for rank in (0, 2)]
                ids = [order[0][0], order[0][2], order[1][0]] + ([order[1][2]] if len(k) == 4 else [])
                wts = [order[0][1], order[0][3], order[1][1]] + ([order[1][3]] if len(k) == 4 else [])
                if len(k) == 3:
                    three += 1
                    assert len(set(_bits(w).tolist())) == 2 and wts[1] == wts[2] and ids[1] < ids[2]
                else:
                    four += 1
                    assert len(set(_bits(w).tolist())) == 1 and ids == sorted(ids)
                tied += 1
        assert three > 100 and four > 100
    finally:
        fr.close()


def test_overflow_model(orc):
    """the model of the overflow cases: on the pixels that meet no more than S ids it is the oracle bit for bit; on the others it
    counts the adds that find S ids placed"""
    case = cc.BY_NAME["overflow_tile"]
    r = _analyse(orc, case)
    fr = cc.oracle_frame(orc, case, r["b"])
    try:
        fits = [p for p in r["holding"] if r["counts"][:, p].max() <= case["S"]]
        over = [p for p in r["holding"] if r["counts"][:, p].max() > case["S"]]
        assert len(fits) > 100 and len(over) > 50
        _model_equals_oracle(case, r["b"], fr, fits, r["own"])
        full = sum(cc.own_visits_model(case, r["b"], a, r["own"][int(p)], slots=case["S"])[3] for p in over for a in range(cc.N_CRYPTO))
        assert full >= 2 * 2 * len(over)
    finally:
        fr.close()


def test_the_probe_bites(orc):
    case = cc.BY_NAME["probe"]
    r = _analyse(orc, case)
    fr = cc.oracle_frame(orc, dict(case, probe=False), r["b"])
    try:
        assert int(fr.counters().accepted_draws) != r["rc"][1]
    finally:
        fr.close()


def test_spectral_streams_cut_into_runs(orc):
    import spectral_pass_cases as sp
    for name in ("spectral_random", "spectral_blocks"):
        r = _analyse(orc, cc.BY_NAME[name])
        assert len(sp.runs(r["b"]["lam"])) >= 3 and len(set(r["b"]["lam"].tolist())) >= 3
