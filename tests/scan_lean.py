"""The cases scan_dma2_kernel's two bodies are tested at (tests/test_scan_lean_cases.py: the table against the oracle, no GPU;
tests/test_gpu_scan_lean.py: the kernel against the oracle).  A plain module: no fixtures, fixed seeds, nothing random.

The kernel (csrc/lentil_kernels.h) decides a group of 64 visits from pos_z alone where the depth turns
every visit of the group off, and reads volume_ignore / transmission / raydir_time only for a group with an OPEN visit: one the
depth leaves to the other columns.  A wave runs its tiles (64 pixels, M groups) in a lean body (pos_z in the ring, the veto
columns fetched per open group) or in the full one (all three in the ring) and changes between them at tile boundaries: to
the full body after a tile with BUSY_GROUPS or more open groups, back after QUIET_TILES tiles in a row without.

A base stream is CLOSED (every visit on the focus plane: the depth turns it off) or OPEN (every visit far out of focus and
vetoed by lentil_ignore, volume_ignore.w = 1).  Into it visits are PLANTED: (visit id, kind) with

  open        the generator's highlight (all its columns: a sample behind the middle of the frame, far out of focus)
  vi_x .. vi_w  the highlight with one component of volume_ignore > 0
  tr          the highlight with transmission > 0: vetoed unless enable_bidir_transmission
  far         the highlight at infinite depth, its ray direction kept: redistributed under a skydome, vetoed without
  far_zero    the highlight at infinite depth without a ray direction: vetoed with or without a skydome
  band_off / band_on   the highlight moved to a depth inside one of the bands in which the kernel asks the function
              (coc_below_by_bands returns 2), where the function says "below 0.4" / "not below"
  junk_nan / junk_pos  a visit of the closed base with NaN / positive values in both veto columns: the depth has turned it
              off, the columns are never looked at, nothing changes

`expect(case, kind)` says which of them redistribute; test_scan_lean_cases.py holds the oracle to it.
Visit ids: tile * 64 * M + group * 64 + lane.  Tiles are handed out in runs of four; a wave's chain of tiles is one run, or,
in a frame of at least 4 x (waves of the grid) runs, a sequence of them (runs t and t + waves ...): see the kernel.
"""
import ctypes as C

import numpy as np

import common
import scan_shapes
from pota_amd import capi, workload

SAMPLES = 8            # samples_override: the oracle's solves stay cheap
SEED = 0x1EA7
BUSY_GROUPS = 2        # kBusyGroups, kQuietTiles of csrc/lentil_kernels.h: test_scan_lean_cases.py holds them to the library's
QUIET_TILES = 2        # (lentil_hip_debug_scan_lean_counts)
LARGE_M = (2, 3, 9)
NUM_CU = 256           # of an MI355X; test_gpu_scan_lean.py builds the large frame's case for the device it finds

VETOED = ("vi_x", "vi_y", "vi_z", "vi_w", "far_zero", "band_off", "junk_nan", "junk_pos")


def expect(case, kind):
    """does a planted visit of this kind redistribute?"""
    if kind in ("open", "band_on"):
        return True
    if kind == "tr":
        return bool(case["kw"].get("enable_bidir_transmission", 0))
    if kind == "far":
        return bool(case["kw"].get("enable_skydome", 0))
    assert kind in VETOED, kind
    return False


def vid(M, tile, group, lane):
    return (tile * M + group) * 64 + lane


def blocks_of(n_tiles, num_cu):
    """scan_dma2_kernel's grid for a launch over n_tiles tiles (scan_grid, csrc/lentil_scan.h)"""
    return max(1, min((n_tiles + 15) // 16, num_cu))


def chain_runs(n_full_tiles, blocks):
    """runs of the first-level sequences of a launch over n_full_tiles whole tiles: ticket t < waves holds runs t, t + waves, ...
    (R / 2 of them), or () where the frame is too small for sequences"""
    waves = blocks * 4
    n_runs = (n_full_tiles + 3) // 4
    R = n_runs // waves
    return waves, (R >> 1 if R >= 2 else 0)


CASES = []


def _case(name, W, rows, M, plants, base="closed", H=None, **kw):
    """a stream over the first `rows` rows of a W x H frame (H: at least 16 rows, so that the draws of the planted highlights,
    which land around the frame's middle, find room)"""
    H = H or max(rows, 16)
    assert len(set(v for v, _ in plants)) == len(plants), name
    CASES.append(dict(name=name, W=W, H=H, rows=rows, M=M, plants=list(plants), base=base, kw=kw))


def _edges(M, n_pixels, chains=None):
    """open visits at the places a pipelined tile body can drop: lanes 0 and 63, a tile's first and last group, a run's first
    and last tile (the last of a chain has no next tile), the tile before the stream's partial last one -- one open group
    per tile wherever possible, so that the wave stays in the lean body, and one tile with every group open"""
    n_full = n_pixels // 64
    last_run = ((n_full - 1) // 4) * 4
    out = {vid(M, 0, 0, 0): "open", vid(M, 1, 0, 63): "open", vid(M, 2, M - 1, 0): "open", vid(M, 3, M - 1, 63): "open",
           vid(M, last_run, M - 1, 5): "open", vid(M, n_full - 1, 0, 63): "open", vid(M, n_full - 1, M - 1, 63): "vi_w"}
    if n_full > 8:
        for g in range(M):                       # a busy tile in the middle of a run: the wave changes body behind it
            out[vid(M, 5, g, (7 * g) % 64)] = "open" if g % 2 == 0 else "vi_x"
        out[vid(M, 8, M // 2, 31)] = "open"
    for first, last in (chains or ()):           # first and last tile of a sequence of runs
        out[vid(M, first, 0, 0)] = "open"
        out[vid(M, last, M - 1, 63)] = "open"
        out[vid(M, last - 3, 0, 1)] = "open"    # the first tile of the sequence's last run: asked for from the run before
    return sorted(out.items())


def _switches(M, first_tile, reverse):
    """two busy tiles in a row then closed ones, or the reverse, from first_tile (the first of a run) on: 8 tiles"""
    busy = (first_tile + 4, first_tile + 5) if reverse else (first_tile, first_tile + 1)
    out = {}
    for t in busy:
        for k, g in enumerate(sorted(set((0, M - 1, M // 2)))[:max(BUSY_GROUPS, 2)] if M > 2 else (0, 1)):
            out[vid(M, t, g, (11 * k + t) % 64)] = "open"
            out[vid(M, t, g, (11 * k + t + 32) % 64)] = "vi_y"
    return out


for _m in (2, 3, 9):
    _case("edges_m%d_64x4" % _m, 64, 4, _m, _edges(_m, 64 * 4))                       # four whole tiles, one run
    _case("edges_m%d_64x17" % _m, 64, 17, _m, _edges(_m, 64 * 17))                    # runs of unequal length: 4 x 4 + 1
    _case("edges_m%d_65x17" % _m, 65, 17, _m, _edges(_m, 65 * 17))                    # 17 tiles and 17 pixels
    _sw = dict(_switches(_m, 0, False))
    _sw.update(_switches(_m, 8, True))
    assert QUIET_TILES <= 2                                                            # (tiles 2, 3 and 8 .. 11 are closed)
    _case("switch_m%d_64x17" % _m, 64, 17, _m, sorted(_sw.items()))
    # every visit open, nearly all of them vetoed: the full body from the second tile on; a few open ones are not
    _case("allopen_m%d_64x17" % _m, 64, 17, _m, [(vid(_m, 0, 0, 0), "open"), (vid(_m, 7, _m - 1, 63), "open"),
                                                  (vid(_m, 16, _m // 2, 33), "open"), (vid(_m, 9, 0, 17), "vi_x")], base="open")

# each veto on its own, on an open visit, one per tile (the wave stays in the lean body) and all in one tile (it leaves it)
_ALONE = ("open", "vi_x", "vi_y", "vi_z", "vi_w", "tr", "far", "far_zero", "band_off", "band_on")
for _tag, _kw in (("default", {}), ("bidir", dict(enable_bidir_transmission=1)), ("skydome", dict(enable_skydome=1))):
    _pl = [(vid(9, t, (2 * t) % 9, (5 * t + 3) % 64), k) for t, k in enumerate(_ALONE)]
    _pl += [(vid(9, 12, g, 9 + g), k) for g, k in enumerate(_ALONE[:9])]
    _case("vetoes_%s" % _tag, 64, 17, 9, _pl, **_kw)
    _case("vetoes_m2_%s" % _tag, 64, 17, 2, [(vid(2, t, t % 2, (5 * t + 3) % 64), k) for t, k in enumerate(_ALONE)], **_kw)
# garbage in the veto columns of visits the depth has turned off, beside an open visit or two
_case("junk", 64, 17, 9, [(vid(9, 0, 0, 0), "junk_nan"), (vid(9, 0, 8, 63), "junk_pos"), (vid(9, 1, 3, 7), "junk_nan"),
                          (vid(9, 1, 3, 8), "open"), (vid(9, 6, 4, 40), "junk_pos"), (vid(9, 16, 8, 63), "junk_nan"),
                          (vid(9, 15, 0, 0), "open")] + [(vid(9, 10, g, 20 + g), "junk_pos" if g % 2 else "junk_nan") for g in range(9)])


def large_case(num_cu=NUM_CU, M=2):
    """A frame of 4 x (waves of the grid) runs: a wave's first ticket is a SEQUENCE of two runs.  Planted: the edges of two such
    chains, and the body changes inside two others: two busy tiles then six closed -- the wave returns to the lean body in the
    middle of its chain, behind the first run's last tile, re-primes the ring there and runs lean tiles that have a next tile
    (M = 9: a ring of six slots, shorter than the tile; M = 3, 2: as long as the tile) --; and six closed then two busy."""
    W = 1024
    waves = 4 * num_cu
    rows = (4 * waves * 4 * 64 + W - 1) // W                    # 4 waves runs of four tiles
    n_full = W * rows // 64
    assert blocks_of(n_full, num_cu) == num_cu
    w, per_chain = chain_runs(n_full, num_cu)
    assert w == waves and per_chain == 2
    chains = [(4 * t, 4 * (t + waves) + 3) for t in (0, waves - 1)]
    plants = dict(_edges(M, W * rows, chains))
    plants.update(_switches(M, 4 * 5, False))                   # chain 5: tiles 20 .. 23, then run 5 + waves
    rev = {}
    for t in (4 * (9 + waves), 4 * (9 + waves) + 1):           # chain 9: closed run 9, then run 9 + waves opens busy
        rev[vid(M, t, 0, t % 64)] = "open"
        rev[vid(M, t, M - 1, (t + 32) % 64)] = "vi_y"
    plants.update(rev)
    return dict(name="large_m%d" % M, W=W, H=rows, rows=rows, M=M, plants=sorted(plants.items()), base="closed", kw={}, num_cu=num_cu)


BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def _bands(p):
    lib = capi.load_library()
    lib.lentil_hip_debug_scan_bands.restype = C.c_int
    lib.lentil_hip_debug_scan_bands.argtypes = [C.POINTER(type(p)), C.POINTER(C.c_float)]
    out = (C.c_float * 8)()
    assert lib.lentil_hip_debug_scan_bands(C.byref(p), out) == 0
    b = np.array(list(out), np.float32)
    return b[0:2], b[2:4], b[4:6], b[6:8]                       # in_lo[2], in_hi[2], out_lo[2], out_hi[2]


def band_depths(orc, p):
    """(cz the function calls below 0.4, cz it does not) where scan_dma2_kernel asks the function: inside an `out` interval
    and outside the `in` interval it surrounds (coc_below_by_bands returns 2)"""
    orc.orc_get_coc_thinlens.restype = C.c_float
    in_lo, in_hi, out_lo, out_hi = _bands(p)
    off = on = None
    for k in range(2):
        if not (out_lo[k] < in_lo[k] < in_hi[k] < out_hi[k]):
            continue
        strips = list(np.linspace(out_lo[k], in_lo[k], 10, dtype=np.float32)[1:-1]) + list(np.linspace(in_hi[k], out_hi[k], 10, dtype=np.float32)[1:-1])
        for z in strips:
            assert out_lo[k] <= z <= out_hi[k] and not (in_lo[k] <= z <= in_hi[k])
            coc = np.float32(orc.orc_get_coc_thinlens(C.byref(p), float(z)))
            if coc < np.float32(0.4):
                off = z if off is None else off
            else:
                on = z if on is None else on
    assert off is not None and on is not None, (in_lo, in_hi, out_lo, out_hi)
    return off, on


def as_scan_shape(case):
    """the case as tests/scan_shapes.py describes one (its setup / stream_pixels / frame_shape / oracle take it)"""
    return dict(name=case["name"], W=case["W"], H=case["H"], M=case["M"], K=0, kinds=[0], camera="po", lens="double_gauss_50mm",
                v_end=None, region=(0, 0, case["W"], case["rows"], 1), lens_mode=0, expect_kernel=scan_shapes.DMA2, ppt=64)


def build(orc, case):
    """(params, lens table, lentil_visits, columns); columns["planted"]: visit ids, columns["kinds"]: their kinds"""
    W, H, M, rows = case["W"], case["H"], case["M"], case["rows"]
    p, model, table, keep = common.po_setup(W, H, samples_override=SAMPLES, **case["kw"])
    shape = as_scan_shape(case)
    n = W * rows * M
    gen = lambda b, e, f: workload.generate(np, b, e, W, H, M, seed=SEED, f_hi=f, focus_dist=float(p.focus_distance) / 10.0,
                                            tan_half_fov=common.tan_half_fov(p))
    cols = gen(0, n, 1.0 if case["base"] == "open" else 0.0)
    cols.pop("extra")
    if case["base"] == "open":
        cols["volume_ignore"][:, 3] = 1.0
    v_src = ((H // 2) * W + W // 2) * M
    src = gen(v_src, v_src + 1, 1.0)
    assert bool(scan_shapes.is_generated_highlight(src)[0])
    names = ("rgba", "pos_z", "raydir_time", "volume_ignore", "transmission")
    z_off, z_on = band_depths(orc, p)
    for v, kind in case["plants"]:
        assert 0 <= v < n, (case["name"], v, n)
        if kind.startswith("junk"):
            assert case["base"] == "closed"
            bad = np.float32(np.nan) if kind == "junk_nan" else np.float32(0.75)
            cols["volume_ignore"][v] = bad
            cols["transmission"][v] = bad
            continue
        for k in names:
            cols[k][v] = src[k][0]
        if kind.startswith("vi_"):
            cols["volume_ignore"][v, "xyzw".index(kind[3])] = 0.5
        elif kind == "tr":
            cols["transmission"][v, 1] = 0.25
        elif kind in ("far", "far_zero"):
            cols["pos_z"][v, 3] = np.float32(1.0e30)
            if kind == "far_zero":
                cols["raydir_time"][v, :3] = 0.0
        elif kind in ("band_off", "band_on"):
            # along the same ray to the camera-space depth cz (world_to_camera is the identity, the unit cm: cz = z)
            f = np.float32(z_off if kind == "band_off" else z_on) / cols["pos_z"][v, 2]
            cols["pos_z"][v] = cols["pos_z"][v] * f
        else:
            assert kind == "open", kind
    visits, _ = capi.make_visits(cols, visits_per_pixel=M, pixels_per_row=W)
    cols["planted"] = np.asarray([v for v, _ in case["plants"]], np.int64)
    cols["kinds"] = [k for _, k in case["plants"]]
    cols["keep"] = (model, keep)
    return p, table, visits, cols
