"""scan_dma2_kernel's lean and full bodies (tests/scan_lean.py) against the oracle.

Each case, twice on one context (the first pass runs in chunks, the second blind and streamed): the pass started in
scan_dma2_kernel; counters and accepted-draw lists equal the oracle's -- which reads volume_ignore, transmission and
raydir_time of every visit and so decides what the kernel must decide from the depth and the columns it fetches on demand;
the frame is within the 1e-5 bar of the fp64 shadows; on every pixel no draw reaches, accumulators, weight and resolved image
are the oracle's bit for bit; and no streamed pass hit the stuck time-out.  tests/test_scan_lean_cases.py (no GPU) shows that
the planted visits redistribute, or do not, as the table says."""
import numpy as np
import pytest

import scan_lean
import scan_shapes
from pota_amd import capi
from test_gpu_scan_shapes import _check_against, _pass, _ran, _same_counters, _set_up

pytestmark = pytest.mark.gpu


def _run(orc, gpu_ctx_factory, case, after_pass=None):
    shape = scan_lean.as_scan_shape(case)
    built = scan_lean.build(orc, case)
    p, table, visits, cols = built
    ref = scan_shapes.oracle(orc, shape, built)
    try:
        want = [v for v, k in case["plants"] if scan_lean.expect(case, k)]
        assert int(ref.counters().redistributed_visits) == len(want) and np.isin(want, ref.log()[:, 0]).all()
        stuck0 = capi.process_stats()[1]
        ctx = gpu_ctx_factory()
        _set_up(ctx, shape, p, table)
        for again in (0, 1):
            c = _pass(ctx, visits)
            _ran(ctx, shape)
            _same_counters(c, ref)
            if again == 0:
                assert c.streamed == 0 and c.blind_chunks == 0
            if after_pass is not None:
                after_pass(ctx, c, again)
            _check_against(ctx, shape, cols, ref)
        assert capi.process_stats()[1] == stuck0, capi.process_stall_notes()
    finally:
        ref.close()


@pytest.mark.parametrize("case", scan_lean.CASES, ids=[c["name"] for c in scan_lean.CASES])
def test_scan_lean(orc, gpu_ctx_factory, case):
    _run(orc, gpu_ctx_factory, case)


@pytest.mark.parametrize("M", scan_lean.LARGE_M)
def test_scan_lean_sequences_of_runs(orc, gpu_ctx_factory, M):
    """A frame large enough that a wave's first ticket is a sequence of two runs (the grid is the device's: the case is
    built for its compute units, and the streamed pass's launch, lentil_hip_debug_last_scan, must be the grid it was built for)"""
    import torch
    case = scan_lean.large_case(torch.cuda.get_device_properties(0).multi_processor_count, M)
    n_full = case["W"] * case["rows"] // 64

    def grid(ctx, c, again):
        if again == 1:
            assert c.streamed == 1
            blocks = ctx.last_scan()[3]
            waves, per_chain = scan_lean.chain_runs(n_full, blocks)
            assert blocks == case["num_cu"] and per_chain >= 2, (blocks, waves, per_chain)

    _run(orc, gpu_ctx_factory, case, after_pass=grid)
