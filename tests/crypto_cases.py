"""The shapes the cryptomatte replay is tested at (tests/test_crypto_cases.py: the table against the oracle, no GPU;
tests/test_gpu_crypto_shapes.py: the kernels of csrc/lentil_crypto.h against the oracle).  A plain module: no fixtures, fixed
seeds, nothing random.

After a pass the adds of the visits that stay in their own pixel are replayed by one of three kernels
(include/lentil_hip.h, LENTIL_CRYPTO_DIRECT_*; crypto_enqueue_direct), and lentil_hip_debug_last_crypto says which:
  a last pixel short of visits, or visits_per_pixel == 0     crypto_direct_kernel: a lane per visit, atomics
  whole pixels, a tile of 128 pixels within 64 KiB of LDS    crypto_direct_tile_kernel<kTables> -- tile_words() 4-byte words,
                                                             r4(128 M) + 2 r4(128 M E) + 2 * 128 * (S + 1) + 256 against 16384
  whole pixels otherwise, or LENTIL_CRYPTO_TILE=0            crypto_direct_owner_kernel
kTables: 1 for the first pass behind a clear, 0 for a pass into tables that hold something, 2 where the clear was put off
(LENTIL_CRYPTO_LAZY_CLEAR=1) and the stream covers every pixel of the frame's buffers, in their order, with S a multiple of 4.
`expect` of a case is computed from that, never written down.

Streams are regions (x0, y0, pixels per row, rows, row stride) of a W x H frame's generated stream, cut out the way
tests/scan_shapes.py cuts them; `whole` streams are generated for the (W + 1) x (H + 1) buffers themselves.  Two cryptomatte
AOVs beside the beauty.  Columns (`columns`):
  generic     make_crypto_columns of tests/test_crypto.py: ids follow the pixel column, unused pairs, zero weights, -0.0
  narrow:P    the same over a frame-wide palette of P ids (no pixel can meet more than P)
  single      one id per pixel and AOV: +0.0 / -0.0 in turn (one key) and 7.5
  wide        E = 64 pairs per visit out of a palette of 64 ids
  rotate      a pixel's visits go round its ids A, B, C(, D), A = +0.0 and -0.0 in different visits: ids leave the tile kernel's
              two registers and come back
  ties        caches of weights 0.25 / 0.25 / 0.5 (or four times 0.25) over ids of both signs: equal sums, bit for bit
  many        every third pixel meets M * E distinct ids (20, 40), weights (k + 1) / 64 in a shuffled order: all distinct
  overflow    every third pixel meets S + 2 ids
The last five come with f_hi = 0: nothing is redistributed, every pixel holds the sequential sums of its own visits, and the GPU's
must be the oracle's bit for bit."""
import ctypes as C

import numpy as np

import scan_shapes
from pota_amd import capi
from test_crypto import UNUSED, make_crypto_columns

ATOMIC, OWNER, TILE = capi.CRYPTO_DIRECT_ATOMIC, capi.CRYPTO_DIRECT_OWNER, capi.CRYPTO_DIRECT_TILE
N_CRYPTO = 2
TP = 128                        # pixels per tile of crypto_direct_tile_kernel
SPHERE = (3.0, 1.0, -70.0, 9.0)  # the analytic occluder of the probed case: beside the axis, in front of the far highlights
EXACTLY_FULL_SLOTS = 10         # the oracle's largest id count over the frame of case "slots_exactly_full" (tests/test_crypto_cases.py)

TAILS = ((1, (1, 1)), (127, (127, 1)), (128, (32, 4)), (129, (43, 3)), (132, (33, 4)), (259, (37, 7)))
WIDTHS = (1, 5, 7, 12, 16, 33, 64)

REQUIRED = (
    ["tail:%d:M=%d" % (n, m) for n, _ in TAILS for m in (1, 2, 9)] +
    ["lds:E=3,S=16,M=13", "lds:E=3,S=16,M=14", "lds:E=1", "lds:E=64,S=64", "lds:E=4,S=32,M=6", "lds:E=4,S=32,M=7"] +
    # (64 slots never fit a tile, 2 * 128 * 65 words alone are more than 64 KiB: the width runs in the owner kernel as the
    # library chooses it and as LENTIL_CRYPTO_TILE=0 forces it)
    ["slots:%d:%s" % (s, k) for s in WIDTHS for k in (("tile", "owner") if s < 64 else ("default", "owner"))] +
    ["slots:exactly-full:tile", "slots:exactly-full:owner"] +
    ["pass:accumulate", "pass:buckets", "pass:lazy_whole", "pass:lazy_flush_region", "pass:lazy_flush_slots5", "pass:lazy_download_first"] +
    ["region:x0>0", "region:y0>0", "region:row_stride=2", "truncated:n-1", "inv_density"] +
    ["form:chunked", "form:streamed", "form:probe", "form:thinlens-tail", "form:spectral:random", "form:spectral:blocks"] +
    ["rank:ties", "rank:0-5", "rank:count-1", "rank:>=count", "rank:>=slots", "rank:20-ids", "rank:40-ids"] +
    ["rotate:E=1:tile", "rotate:E=1:owner", "rotate:E=3:tile", "rotate:E=3:owner"] +
    ["overflow:tile", "overflow:owner", "overflow:atomic"] +
    ["child:grid-stride", "child:flags=0"]
)

CASES = []


def r4(x):
    return (x + 3) & ~3


def tile_words(M, E, S):
    """LDS of one tile of crypto_direct_tile_kernel, in 4-byte words"""
    return r4(TP * M) + 2 * r4(TP * M * E) + 2 * TP * (S + 1) + 2 * TP


def _case(name, W, H, M=9, E=3, S=16, region=None, whole=False, v_end=None, camera="po", columns="generic", f_hi=0.015, tile=None,
          lazy=False, form="single", frames=1, ctx_env=None, probe=False, inv_density=False, spectral=None, ranks=(0, 2, 4),
          wants_draws=True, covers=()):
    """W x H: the frame.  region: the pixels the stream covers (None: the frame; whole: the (W + 1) x (H + 1) buffers).  v_end: the
    stream is cut off behind that many visits.  tile: what LENTIL_CRYPTO_TILE is set to (None: unset).  lazy:
    LENTIL_CRYPTO_LAZY_CLEAR=1.  form: what tests/test_gpu_crypto_shapes.py does with the case (single: `frames` times clear,
    pass, compare).  ctx_env: what the library reads when the context is created.  spectral: a case of
    tests/spectral_pass_cases.py whose stream and wavelengths are taken.  ranks: the ranks downloaded."""
    if whole:
        region = (0, 0, W + 1, H + 1, 1)
    CASES.append(dict(name=name, W=W, H=H, M=M, E=E, S=S, region=region or (0, 0, W, H, 1), whole=whole, v_end=v_end, camera=camera,
                      columns=columns, f_hi=f_hi, tile=tile, lazy=lazy, form=form, frames=frames, ctx_env=dict(ctx_env or {}),
                      probe=probe, inv_density=inv_density, spectral=spectral, ranks=tuple(ranks), wants_draws=wants_draws and f_hi > 0,
                      direct_only=f_hi == 0, covers=tuple(covers),
                      # what scan_shapes' helpers read
                      K=0, kinds=[0], lens="double_gauss_50mm", lens_mode=0))


# ---- tile tails: streams of ppr x rows pixels in the middle rows of a frame that leaves the draws room ------------------------
for _n, (_ppr, _rows) in TAILS:
    for _m in (1, 2, 9):
        _w = max(_ppr, 24)
        _case("tail_%d_m%d" % (_n, _m), _w, _rows + 8, M=_m, region=((_w - _ppr) // 2, 4, _ppr, _rows, 1),
              f_hi={1: 0.12, 2: 0.06, 9: 0.02}[_m], wants_draws=_n > 1, covers=["tail:%d:M=%d" % (_n, _m)],
              # (one pixel's draws carry scaled copies of one cache: its zero weights would tie wherever they land)
              columns="rotate" if _n == 1 else "generic")

# ---- the LDS boundary -----------------------------------------------------------------------------------------------------------
_case("lds_m13", 31, 9, M=13, covers=["lds:E=3,S=16,M=13"])
_case("lds_m14", 31, 9, M=14, covers=["lds:E=3,S=16,M=14"])
_case("lds_e1", 37, 11, E=1, covers=["lds:E=1"])
_case("lds_e64_s64", 21, 7, M=2, E=64, S=64, columns="wide", f_hi=0.04, covers=["lds:E=64,S=64"])
_case("lds_e4_s32_m6", 31, 9, M=6, E=4, S=32, covers=["lds:E=4,S=32,M=6"])
_case("lds_e4_s32_m7", 31, 9, M=7, E=4, S=32, covers=["lds:E=4,S=32,M=7"])

# ---- table widths, in the tile and in the owner kernel --------------------------------------------------------------------------
for _s in WIDTHS:
    _colm = {1: "single", 5: "narrow:5", 7: "narrow:7"}.get(_s, "generic")
    for _k, _t in ((("tile" if _s < 64 else "default"), None), ("owner", "0")):
        # (33 slots fit a tile up to M = 8)
        _case("slots%d_%s" % (_s, _k), 37, 19, M=9 if _s <= 16 else 5, S=_s, columns=_colm, tile=_t, ranks=(0, 1, 2, 4), covers=["slots:%d:%s" % (_s, _k)])
for _k, _t in (("tile", None), ("owner", "0")):
    _case("slots_exactly_full_%s" % _k, 37, 19, S=EXACTLY_FULL_SLOTS, tile=_t, covers=["slots:exactly-full:%s" % _k])

# ---- passes ---------------------------------------------------------------------------------------------------------------------
_case("accumulate", 37, 19, form="accumulate", covers=["pass:accumulate"])
BUCKETS = []
for _b in scan_shapes.BUCKETS:
    _case("crypto_" + _b, 64, 48, M=5, region=scan_shapes.BY_NAME[_b]["region"], form="bucket", covers=[])
    BUCKETS.append("crypto_" + _b)
# 48 x 31 buffers: 11 tiles and 80 pixels, so that variant 2 also meets a short tile
_case("lazy_whole", 47, 30, M=5, whole=True, lazy=True, frames=3, covers=["pass:lazy_whole"])
_case("lazy_flush_region", 45, 23, M=2, lazy=True, frames=2, covers=["pass:lazy_flush_region"])
_case("lazy_flush_slots5", 45, 23, M=2, S=5, columns="narrow:5", whole=True, lazy=True, frames=2, covers=["pass:lazy_flush_slots5"])
_case("lazy_download_first", 45, 23, M=2, lazy=True, form="lazy_download_first", covers=["pass:lazy_download_first"])

# ---- stream shapes --------------------------------------------------------------------------------------------------------------
_case("region_x0", 48, 24, region=(9, 0, 30, 12, 1), covers=["region:x0>0"])
_case("region_y0", 48, 24, region=(0, 7, 30, 12, 1), covers=["region:y0>0"])
_case("rowstride2", 32, 24, region=(3, 1, 20, 10, 2), covers=["region:row_stride=2"])
_case("truncated", 37, 19, v_end=37 * 19 * 9 - 1, covers=["truncated:n-1"])
_case("inv_density", 37, 19, inv_density=True, covers=["inv_density"])

# ---- forms of the pass ----------------------------------------------------------------------------------------------------------
_case("chunked", 70, 29, M=5, ctx_env={"LENTIL_STREAM": "0", "LENTIL_CHUNKS": "3"}, frames=2, covers=["form:chunked"])
_case("streamed", 45, 23, M=2, frames=3, covers=["form:streamed"])
_case("probe", 45, 23, M=9, probe=True, f_hi=0.03, covers=["form:probe"])
_case("thinlens_tail", 37, 19, M=5, camera="thinlens", covers=["form:thinlens-tail"])
for _a in ("random", "blocks"):
    _case("spectral_" + _a, 48, 32, spectral=("plain", "samples-4", _a), covers=["form:spectral:" + _a])

# ---- ranks ----------------------------------------------------------------------------------------------------------------------
_case("ties", 37, 7, E=4, columns="ties", f_hi=0.0, ranks=(0, 1, 2, 3, 4, 5, 16, 17),
      covers=["rank:ties", "rank:0-5", "rank:count-1", "rank:>=count", "rank:>=slots"])
_case("many20", 37, 7, M=5, E=4, S=32, columns="many", f_hi=0.0, ranks=(0, 1, 5, 17, 18, 19, 20), covers=["rank:20-ids"])
_case("many40", 37, 7, M=10, E=4, S=64, columns="many", f_hi=0.0, ranks=(0, 3, 16, 37, 38, 39, 40), covers=["rank:40-ids"])

# ---- the register cache ---------------------------------------------------------------------------------------------------------
for _e in (1, 3):
    for _k, _t in (("tile", None), ("owner", "0")):
        _case("rotate_e%d_%s" % (_e, _k), 37, 7, E=_e, columns="rotate", f_hi=0.0, tile=_t, ranks=(0, 1, 2, 3), covers=["rotate:E=%d:%s" % (_e, _k)])

# ---- overflow -------------------------------------------------------------------------------------------------------------------
_case("overflow_tile", 37, 7, E=2, S=5, columns="overflow", f_hi=0.0, form="overflow", covers=["overflow:tile"])
_case("overflow_owner", 37, 7, E=2, S=5, columns="overflow", f_hi=0.0, tile="0", form="overflow", covers=["overflow:owner"])
_case("overflow_atomic", 37, 7, E=2, S=5, columns="overflow", f_hi=0.0, v_end=37 * 7 * 9 - 1, form="overflow", covers=["overflow:atomic"])

# ---- children: what the library reads once per process --------------------------------------------------------------------------
# 263 x 147 pixels at M = 2: 302 tiles and a 5-pixel tail, walked by num_cu blocks (LENTIL_CRYPTO_TILE_BLOCKS=1)
_case("grid_stride", 263, 147, M=2, f_hi=0.004, covers=["child:grid-stride"])
# the child pytest processes of tests/test_gpu_crypto_shapes.py: env, the -k expression, how many tests that selects, and
# what their output must say
CHILDREN = {
    "grid_stride": dict(env={"LENTIL_CRYPTO_TILE_BLOCKS": "1"}, select="test_crypto_shape and grid_stride", tests=1,
                        says=["grid stride: "]),
    # LENTIL_CRYPTO_FLAGS=0: the decision is made again from the columns -- a tail, the buckets and the thin lens once more
    "flags0": dict(env={"LENTIL_CRYPTO_FLAGS": "0"}, select="(test_crypto_shape and (tail_259_m9 or thinlens_tail)) or test_buckets_into_one_frame",
                   tests=3, says=["flags decided from the columns: tail_259_m9", "flags decided from the columns: thinlens_tail",
                                  "flags decided from the columns: crypto_bucket3"]),
}
COVERED_ELSEWHERE = {"pass:buckets": "the four crypto_bucket* cases, one after the other (test_buckets_into_one_frame)",
                     "child:flags=0": "CHILDREN['flags0']"}

BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
_named = set(t for c in CASES for t in c["covers"]) | set(COVERED_ELSEWHERE)
assert _named == set(REQUIRED) and len(set(REQUIRED)) == len(REQUIRED), (sorted(set(REQUIRED) - _named), sorted(_named - set(REQUIRED)))
SINGLE = [c for c in CASES if c["form"] == "single"]


# ---- what a case expects --------------------------------------------------------------------------------------------------------
def n_visits(case):
    x0, y0, ppr, rows, rs = case["region"]
    n = ppr * rows * case["M"]
    return n if case["v_end"] is None else case["v_end"]


def tiles_and_tail(case):
    return divmod(n_visits(case) // case["M"], TP)


def fits_tile(case):
    return tile_words(case["M"], case["E"], case["S"]) * 4 <= 64 * 1024


def expect_kernel(case):
    """(kernel, kTables of the first pass behind a clear)"""
    if n_visits(case) % case["M"]:
        return ATOMIC, 0
    if case["tile"] == "0" or not fits_tile(case):
        return OWNER, 0
    return TILE, (2 if case["lazy"] and case["whole"] and case["S"] % 4 == 0 else 1)


def expect_flushed(case):
    """a wipe that was put off is flushed by the pass's own-pixel kernel unless that is variant 2"""
    return case["lazy"] and expect_kernel(case) != (TILE, 2)


# ---- columns --------------------------------------------------------------------------------------------------------------------
def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _random_weights(rng, n, E, unused=0.25, zero=0.1):
    w = rng.random((n, E)).astype(np.float32)
    w[rng.random((n, E)) < zero] = 0.0
    u = rng.random((n, E)) < unused
    u[:, 0] = False
    w[u] = UNUSED
    return w


def crypto_columns(case, n, ppr):
    """per cryptomatte AOV [n, E] ids and weights of a stream of n visits, ppr pixels per row"""
    M, E, S, kind = case["M"], case["E"], case["S"], case["columns"]
    v = np.arange(n)
    q, m = v // M, v % M
    rng = np.random.default_rng(0xC0DE + E + 7 * M)
    hashes, weights = [], []
    if kind == "generic":
        return make_crypto_columns(n, ppr, M, N_CRYPTO, E)
    for a in range(N_CRYPTO):
        ids = np.empty((n, E), np.float32)
        if kind == "single":
            ids[:] = 99.0 + np.arange(E)[None, :]
            ids[:, 0] = np.where(v % 2 == 1, np.float32(-0.0), np.float32(0.0)) if a == 0 else np.float32(7.5)
            w = rng.random((n, E)).astype(np.float32)
            w[:, 1:] = UNUSED
        elif kind.startswith("narrow:"):
            P = int(kind.split(":")[1])
            assert E <= P and P in (5, 7)                      # (prime: the steps 1 and 2 go round the whole palette)
            pal = (np.random.default_rng(P).standard_normal(P) * 1e3).astype(np.float32)
            pal[0] = 0.0
            base = ((q % ppr) // 6 + a) % P
            step = 1 + rng.integers(0, 2, n)
            for e in range(E):
                ids[:, e] = pal[(base + e * step) % P]
            ids[(ids == 0.0) & (v % 2 == 1)[:, None]] = np.float32(-0.0)
            w = _random_weights(rng, n, E)
        elif kind == "wide":
            P = 64
            assert E <= P <= S
            pal = ((np.arange(P) - 20) * 1.5 + a).astype(np.float32)
            for e in range(E):
                ids[:, e] = pal[(v * 7 + e) % P]
            w = _random_weights(rng, n, E, unused=0.5)
        elif kind == "rotate":
            K = 3 if E == 1 else E + 1
            pal = np.stack([np.zeros(n), 3.25 + q % 5, -11.5 - q % 3 - a, 1e6 + q % 7], 1).astype(np.float32)[:, :K]
            for e in range(E):
                ids[:, e] = pal[v, (m + q + e) % K]
            ids[(ids == 0.0) & ((m // K) % 2 == 1)[:, None]] = np.float32(-0.0)        # +0.0 and -0.0 in different visits
            w = rng.random((n, E)).astype(np.float32) + np.float32(0.01)
            if E > 2:
                w[(m + q) % 3 == 0, 2] = UNUSED
        elif kind == "ties":
            assert E == 4
            pal = np.array([-300.5, -2.0, 0.0, 1.5, 17.0, 1e6, -1e-3], np.float32)
            off = np.array([0, 1, 3, 4])
            four = q % 2 == 1                                   # four ids at 0.25 each; else 0.25 / 0.25 / 0.5 and an unused pair
            k = np.where(four, 4, 3)
            w = np.empty((n, E), np.float32)
            for e in range(E):
                j = (e + m) % k                                 # the cache's order goes round with the visit
                ids[:, e] = pal[(q + a + off[j]) % 7]
                w[:, e] = np.where(four | (j < 2), 0.25, 0.5)
            w[~four, 3] = UNUSED
            ids[~four, 3] = 5e5
            ids[(ids == 0.0) & (m % 2 == 1)[:, None]] = np.float32(-0.0)
        elif kind == "many":
            heavy = q % 3 == 0
            w = np.empty((n, E), np.float32)
            n_pix = (n + M - 1) // M
            perm = np.stack([np.random.default_rng(1000 * a + int(p)).permutation(M * E) for p in range(n_pix)])     # [pixel, M * E]
            for e in range(E):
                j = m * E + e
                ids[:, e] = np.where(heavy, (100.0 + 1.5 * j) * np.where(j % 2, -1.0, 1.0), 2.5 * (j % 6) - 5.0 + a)
                w[:, e] = (perm[q, j] + 1) / 64.0
        elif kind == "overflow":
            assert E == 2
            K = np.where(q % 3 == 1, S + 2, S - 1)
            for e in range(E):
                ids[:, e] = 13.0 * ((2 * m + e) % K) + q % 11 - 40.0 + a
            w = rng.random((n, E)).astype(np.float32) + np.float32(0.01)
        else:
            raise KeyError(kind)
        for e in range(1, E):                                  # ids inside one visit's cache are distinct, as a map's keys are
            for e2 in range(e):
                both = (w[:, e].view(np.uint32) != 0xFFFFFFFF) & (w[:, e2].view(np.uint32) != 0xFFFFFFFF)
                assert not (both & (ids[:, e] == ids[:, e2])).any(), (case["name"], e, e2)
        hashes.append(_f32(ids))
        weights.append(_f32(w))
    return hashes, weights


# ---- streams --------------------------------------------------------------------------------------------------------------------
def build(case):
    """dict: p, table, visits, cols, hashes, weights, n, pix (the frame pixel of every visit), lam (spectral: the wavelengths)"""
    if case["spectral"]:
        import list_draw_spectral_cases as ls
        kind, name, assignment = case["spectral"]
        s = ls.setup(kind, name)
        assert tuple(s["frame"]) == (case["W"], case["H"]) and int(s["visits"].visits_per_pixel) == case["M"]
        p, table, visits, cols, n = s["p"], s["table"], s["visits"], s["cols"], int(s["n"])
        keep, lam = s, ls.lambdas(kind, name, assignment)
    else:
        W, H, M = case["W"], case["H"], case["M"]
        x0, y0, ppr, rows, rs = case["region"]
        p, table, keep = scan_shapes.setup(case)
        gW, gH = (int(p.xres), int(p.yres)) if case["whole"] else (W, H)      # the frame the generator lays its visits over
        assert (int(p.xres), int(p.yres)) == (W + 1, H + 1)
        assert 0 <= x0 and x0 + ppr <= gW and 0 <= y0 and y0 + (rows - 1) * rs < gH, "the region leaves the frame"
        full = scan_shapes._generate(p, dict(case, W=gW, H=gH), 0, gW * gH * M, case["f_hi"])
        pixq = ((y0 + np.arange(rows) * rs)[:, None] * gW + (x0 + np.arange(ppr))[None, :]).ravel()
        vis = (pixq[:, None] * M + np.arange(M)[None, :]).ravel()[:n_visits(case)]
        cols = {k: np.ascontiguousarray(full[k][vis]) for k in ("rgba", "pos_z", "raydir_time", "volume_ignore", "transmission")}
        cols["extra"] = []
        n = int(vis.size)
        if case["inv_density"]:
            cols["inv_density"] = np.where((np.arange(n) // M) % 2 == 1, np.float32(1.0 / 16.0), np.float32(1.0 / 9.0)).astype(np.float32)
        visits, _ = capi.make_visits(cols, visits_per_pixel=M, pixels_per_row=ppr, pixel_x0=x0, pixel_y0=y0, pixel_row_stride=rs)
        lam = None
    x0, y0, ppr, rows, rs = case["region"]
    qq = np.arange(n, dtype=np.int64) // case["M"]
    pix = (y0 + (qq // ppr) * rs) * int(p.xres) + x0 + qq % ppr
    hashes, weights = crypto_columns(case, n, ppr)
    return dict(p=p, table=table, visits=visits, cols=cols, hashes=hashes, weights=weights, n=n, pix=pix, lam=lam, keep=keep,
                sphere=np.array(SPHERE, np.float32) if case["probe"] else None)


def oracle_into(orc, fr, case, b):
    """one oracle pass of the case's stream into frame fr (which accumulates)"""
    lens = orc.orc_lens_create(C.byref(b["table"])) if b["table"] is not None else None
    try:
        if b["lam"] is None:
            fr.run(lens, None, b["visits"])
        else:
            # the oracle's pass in which visit v is at lam[v]: the stream in runs of equal wavelength (tests/spectral_pass_cases.py);
            # cryptomatte weights do not depend on it
            import spectral_pass_cases as sp
            bw = float(fr.params.lambda_bw)
            for v0, v1, entry in sp.runs(b["lam"]):
                fr.params.lambda_bw = bw if entry == 0.0 else entry
                fr.run(lens, None, b["visits"], v0, v1)
            fr.params.lambda_bw = bw
    finally:
        if lens:
            orc.orc_lens_destroy(lens)


def oracle_frame(orc, case, b, passes=1):
    """the oracle's frame after `passes` passes of the case's stream, draw log kept.  The caller closes it."""
    import oracle_lib
    fr = oracle_lib.Frame(orc, type(b["p"]).from_buffer_copy(b["p"]), n_aovs=1, keep_log=True)
    fr.set_crypto(b["hashes"], b["weights"])
    if case["probe"]:
        fr.set_probe(oracle_lib.sphere_occluder(orc), b["sphere"].ctypes.data, None)
    for _ in range(passes):
        oracle_into(orc, fr, case, b)
    return fr


# ---- models ---------------------------------------------------------------------------------------------------------------------
def key_of(x):
    """what the tables compare: the id's bits, -0.0 as +0.0"""
    bits = int(np.float32(x).view(np.uint32))
    return 0 if bits == 0x80000000 else bits


def own_visits_model(case, b, a, pixel_visits, slots=None):
    """A pixel's own visits added one after the other, in fp32, in stream order: (keys in the order they were entered, their
    sums, the total, adds that found `slots` keys placed already).  pixel_visits: the visit ids of the pixel, highlights left
    out by the caller."""
    invd_col = b["cols"].get("inv_density")
    h, w = b["hashes"][a], b["weights"][a]
    keys, sums, total, full = [], [], np.float32(0.0), 0
    for v in pixel_visits:
        invd = np.float32(invd_col[v]) if invd_col is not None else np.float32(b["p"].inverse_sample_density)
        total = np.float32(total + invd)
        for e in range(case["E"]):
            cw = w[v, e]
            if cw.view(np.uint32) == 0xFFFFFFFF:
                continue
            k = key_of(h[v, e])
            add = np.float32(cw * invd)
            if k in keys:
                i = keys.index(k)
                sums[i] = np.float32(sums[i] + add)
            elif slots is not None and len(keys) >= slots:
                full += 1
            else:
                keys.append(k)
                sums.append(np.float32(np.float32(0.0) + add))
    return keys, sums, total, full


def first_slot(key, slots):
    """where the probing for a key starts in a table of `slots` entries (crypto_first_slot): the key's
    bits times 2654435761 modulo 2^32, its upper sixteen bits modulo slots; from there slot after slot, round the table"""
    return ((key * 2654435761 & 0xFFFFFFFF) >> 16) % slots


def placement(keys, slots):
    """the table of a pixel whose keys were entered in that order (no more than `slots`): [slots] uint32, 0xFFFFFFFF free"""
    table = np.full(slots, 0xFFFFFFFF, np.uint32)
    for k in keys:
        s = first_slot(k, slots)
        while table[s] != 0xFFFFFFFF:
            s = (s + 1) % slots
        table[s] = k
    return table


def reenters_two_registers(case, b, a, pixel_visits):
    """does an id leave a two-entry most-recently-used cache and come back, over the pixel's own visits?"""
    h, w = b["hashes"][a], b["weights"][a]
    regs, gone = [], set()
    for v in pixel_visits:
        for e in range(case["E"]):
            if w[v, e].view(np.uint32) == 0xFFFFFFFF:
                continue
            k = key_of(h[v, e])
            if k in regs:
                regs.remove(k)
                regs.append(k)
                continue
            if k in gone:
                return True
            regs.append(k)
            if len(regs) > 2:
                gone.add(regs.pop(0))
    return False
