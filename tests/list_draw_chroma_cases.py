"""The case table of the LENTIL_DRAWS_CHANNELS tests (tests/test_gpu_list_draws_chroma.py: lentil_hip_list_draws for polynomial
optics with abb_chromatic != 0 against the oracle; tests/test_list_draw_chroma_cases.py: the table itself against the oracle
alone, no GPU).  A plain module: no fixtures, fixed seeds; what it computes is computed once per process and never written to.

A case is a case of tests/list_draw_cases.py's kind (setup() and oracle_pass() there build and run it; frame 48x32 and f_hi 0.03
where not given) with abb_chromatic != 0.  Its expectation is the oracle's single-threaded pass with the draw log kept: an
attempt has up to three records, the channel (0, 1, 2 for the reference's -1, 0, 1) in bits 30-31 of `attempt`.
"""
import numpy as np

import list_draw_cases as lc
from pota_amd import _abi

CASES = {}
CHANNEL_SHIFT = 30
ATTEMPT_MASK = (1 << CHANNEL_SHIFT) - 1


def _case(name, **kw):
    """kw: what list_draw_cases._case takes"""
    assert name not in CASES and kw.get("abb_chromatic", 0.0) != 0.0
    CASES[name] = dict(name=name, kw=kw)


# both signs and the far end of the mode
_case("pos-16", samples=16, abb_chromatic=0.5)
_case("neg-16", abb_chromatic=-0.5)
_case("one-16", abb_chromatic=1.0)
# samples-N: a partial slab, the slab boundary, a 5 * samples that is no multiple of 64
for _s in (4, 63, 64, 65):
    _case("samples-%d" % _s, samples=_s, frame=(32, 24), f_hi=0.05 if _s < 63 else 0.02, abb_chromatic=0.5)
# short: highlights around the frame's edge -- counts that go down, visits that run into 5 * samples
_case("short-r0", samples=16, vignetting_retries=0, edge=(0.9, 1.25), abb_chromatic=0.5)
_case("short-r3", samples=16, vignetting_retries=3, edge=(0.7, 1.1), abb_chromatic=1.0)
# no try at all: every channel of every attempt fails
_case("retries-1", samples=16, vignetting_retries=-1, abb_chromatic=0.5)
# the other compiled-in lens, the interpreter
_case("petzval", samples=12, frame=(32, 24), lens="petzval_58mm", seed=0x51, abb_chromatic=0.5)
_case("interpreter", samples=24, lens_mode=1, path=_abi.DRAWS_PATH_INTERPRETER, abb_chromatic=0.5)
# aperture samplers
_case("bokeh-image", samples=20, bokeh="blacklines12", bokeh_enable_image=1, abb_chromatic=0.5)
_case("blades5-neg", samples=20, bokeh_aperture_blades=5, abb_chromatic=-0.5)
# fitted_bidir_add_energy
_case("add-energy", samples=16, bidir_add_energy=2.5, abb_chromatic=0.5)

ALL = sorted(CASES)
POSITION_CASES = ("pos-16", "one-16", "short-r3", "petzval", "interpreter", "bokeh-image")
OWN_FILM_CASES = ("pos-16", "neg-16", "add-energy")

_setups, _oracles = {}, {}


def _borrowed(name, fn):
    """fn(key) with the case entered into list_draw_cases' table as `key` for the call, and taken out again (what
    tests/test_list_draw_cases.py iterates stays what it was)"""
    key = "chroma:" + name
    saved = dict(lc.CASES)
    try:
        lc.CASES.clear()
        lc._case(key, **CASES[name]["kw"])
        return fn(key)
    finally:
        lc.CASES.clear()
        lc.CASES.update(saved)


def setup(name):
    """list_draw_cases.setup()'s dict"""
    if name not in _setups:
        s = dict(_borrowed(name, lc.setup))
        s["name"] = name
        _setups[name] = s
    return _setups[name]


def oracle_pass(orc, name):
    """list_draw_cases.oracle_pass()'s dict: log uint32 [n, 3] sorted by (visit, attempt | channel << 30), the counters, the
    exact sums"""
    if name not in _oracles:
        _oracles[name] = _borrowed(name, lambda key: lc.oracle_pass(orc, key))
    return _oracles[name]


def split_log(log):
    """(visit, attempt n, channel 0 ... 2) of a draw log, int64 each"""
    a = log[:, 1].astype(np.int64)
    return log[:, 0].astype(np.int64), a & ATTEMPT_MASK, a >> CHANNEL_SHIFT


def per_attempt(log):
    """(visit, attempt, successes 1 ... 3) per logged attempt, ordered by (visit, attempt)"""
    v, n, c = split_log(log)
    key, succ = np.unique(v << 32 | n, return_counts=True)
    return key >> 32, key & 0xFFFFFFFF, succ


def walk(log, samples):
    """The reference's rule walked in Python over every visit of the log: count += successes - 2 per attempt (an attempt that
    is not in the log had none) while count < samples and n < 5 * samples -> dict visit -> (attempts made, lowest count seen,
    final count, records).  The walk stops where the reference's loop stops: a visit that reached `samples` did so with an
    attempt of three successes, which is its last logged one; any other made all 5 * samples attempts."""
    av, an, asucc = per_attempt(log)
    out = {}
    if not av.size:
        return out
    bounds = np.flatnonzero(np.diff(av)) + 1
    for lo, hi in zip(np.concatenate([[0], bounds]), np.concatenate([bounds, [av.size]])):
        succ = dict(zip(an[lo:hi].tolist(), asucc[lo:hi].tolist()))
        count, n, low = 0, 0, 0
        while count < samples and n < 5 * samples:
            count += succ.get(n, 0) - 2
            low = min(low, count)
            n += 1
        out[int(av[lo])] = (n, low, count, int(asucc[lo:hi].sum()))
    return out
