"""CPU: the flood's default look-ahead (default_look_ahead in csrc/k_flood.hip, through the host-only ivx_flood_look_ahead) at
its switch point.  Behind a round whose list is at least as long as the length from which a round gets the full grid
(384 tiles: such a round outlasts the host's way to the next launch) nothing is queued ahead; behind a shorter one, one round."""
import ctypes

import pytest

LONG_LIST = 384


@pytest.fixture(scope="module")
def look_ahead():
    from invesalius3_amd import build

    lib = ctypes.CDLL(build.build())
    lib.ivx_flood_look_ahead.argtypes = [ctypes.c_int64, ctypes.POINTER(ctypes.c_int32)]
    lib.ivx_flood_look_ahead.restype = ctypes.c_int

    def call(n_list):
        out = ctypes.c_int32(-1)
        rc = lib.ivx_flood_look_ahead(n_list, ctypes.byref(out))
        return rc, out.value
    return call


@pytest.mark.parametrize("n_list,want", [(0, 1), (1, 1), (95, 1), (96, 1), (LONG_LIST - 1, 1), (LONG_LIST, 0), (LONG_LIST + 1, 0),
                                         (1536, 0), (8192, 0), (2 ** 32 - 1, 0), (2 ** 40, 0)])
def test_switch_point(look_ahead, n_list, want):
    assert look_ahead(n_list) == (0, want)


def test_bad_arguments_are_refused(look_ahead):
    from invesalius3_amd import build

    assert look_ahead(-1)[0] == -1  # IVX_EINVAL
    lib = ctypes.CDLL(build.build())
    lib.ivx_flood_look_ahead.argtypes = [ctypes.c_int64, ctypes.c_void_p]
    assert lib.ivx_flood_look_ahead(5, None) == -1
