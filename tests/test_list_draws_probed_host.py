"""LENTIL_DRAWS_PROBED without a GPU: the constant in the header and in _abi, the binding's argument, and the two records'
layout still what tests/test_list_draws_host.py pins."""
import inspect

import test_list_draws_host as base
from pota_amd import _abi, capi


def test_the_flag_is_bit_1_in_the_header_and_in_abi():
    got = base._from_c('  printf("%u %u\\n", (unsigned)LENTIL_DRAWS_PROBED, (unsigned)LENTIL_DRAWS_DEVICE_POINTERS);')
    assert got == [_abi.DRAWS_PROBED, _abi.DRAWS_DEVICE_POINTERS] == [2, 1]
    assert inspect.signature(capi.Context.list_draws).parameters["probed"].default is False


def test_the_layouts_are_unchanged():
    assert base._layout("lentil_draw", base.DRAW_FIELDS) == [32, 0, 4, 8, 12, 16]
    assert base._declared("lentil_draw") == base.DRAW_FIELDS and base._declared("lentil_draw_list") == base.LIST_FIELDS
    assert _abi.Draw.itemsize == 32 and list(_abi.Draw.names) == base.DRAW_FIELDS
    base.test_draw_list_layout_matches_the_header()


def test_a_null_context_is_an_error_with_the_flag_too():
    lib = capi.load_library()
    req = _abi.DrawList()
    req.flags = _abi.DRAWS_PROBED
    assert lib.lentil_hip_list_draws(None, req) == _abi.ERR_INVALID
