"""Options "host_joins" / "host_join_budget_us" and lws_join_stats (include/lwsnet_hip.h) on the host: the option calls and the
counters touch no GPU.  (lws_clone needs a finalized source, hence a device: that the clone carries both options over is
tests/test_gpu_host_joins.py::test_clone_carries_both_options.)"""
import ctypes

from lwsnet_amd import _lib
from lwsnet_amd.weights import default_args


def _create(lib):
    a = default_args()
    cfg = _lib.LwsConfig((ctypes.c_int32 * 3)(*a.maxdisplist), a.layers_3d, a.channels_3d,
                         (ctypes.c_int32 * 3)(*a.growth_rate), 0, a.interp_align_mode)
    h = ctypes.c_void_p()
    assert lib.lws_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    return h


def test_names_defaults_and_ranges(hip_lib):
    h = _create(hip_lib)
    v = ctypes.c_int(123)
    assert hip_lib.lws_get_option(h, b"host_joins", ctypes.byref(v)) == 0 and v.value == -1
    assert hip_lib.lws_get_option(h, b"host_join_budget_us", ctypes.byref(v)) == 0 and v.value == 900
    for value in (0, 1, -1):
        assert hip_lib.lws_set_option(h, b"host_joins", value) == 0
        assert hip_lib.lws_get_option(h, b"host_joins", ctypes.byref(v)) == 0 and v.value == value
    for value in (-2, 2):
        assert hip_lib.lws_set_option(h, b"host_joins", value) == _lib.LWS_ERR_INVALID
        assert b"host_joins" in hip_lib.lws_last_error()
    assert hip_lib.lws_get_option(h, b"host_joins", ctypes.byref(v)) == 0 and v.value == -1      # a refused value changes nothing
    for value in (0, 1, 1000000):
        assert hip_lib.lws_set_option(h, b"host_join_budget_us", value) == 0
        assert hip_lib.lws_get_option(h, b"host_join_budget_us", ctypes.byref(v)) == 0 and v.value == value
    for value in (-1, 1000001):
        assert hip_lib.lws_set_option(h, b"host_join_budget_us", value) == _lib.LWS_ERR_INVALID
        assert b"host_join_budget_us" in hip_lib.lws_last_error()
    # clone of a handle that was never finalized: refused before anything is copied
    c = ctypes.c_void_p()
    assert hip_lib.lws_clone(h, ctypes.byref(c)) == _lib.LWS_ERR_STATE and not c
    assert hip_lib.lws_destroy(h) == 0


def test_debug_delay_side_arguments_on_the_host(hip_lib):
    """lws_debug_delay_side is host-side state: known bits, 0..250000 microseconds, a null handle refused."""
    h = _create(hip_lib)
    assert (_lib.LWS_DELAY_F4, _lib.LWS_DELAY_F2, _lib.LWS_DELAY_LEFT, _lib.LWS_DELAY_CHUNKS, _lib.LWS_DELAY_ALL) == (1, 2, 4, 8, 15)
    for segments, us in ((0, 0), (1, 1), (15, 250000), (4, 0), (0, 50000), (8, 50000)):
        assert hip_lib.lws_debug_delay_side(h, segments, us) == 0, (segments, us)
    for segments, us in ((16, 50000), (-1, 50000), (31, 50000), (4, -1), (4, 250001), (1 << 30, 0)):
        assert hip_lib.lws_debug_delay_side(h, segments, us) == _lib.LWS_ERR_INVALID, (segments, us)
        assert b"lws_debug_delay_side" in hip_lib.lws_last_error()
    assert hip_lib.lws_debug_delay_side(None, 4, 50000) == _lib.LWS_ERR_INVALID
    assert hip_lib.lws_destroy(h) == 0


def test_join_stats_on_the_host(hip_lib):
    h = _create(hip_lib)
    out = (ctypes.c_int64 * 12)(*[7] * 12)
    assert hip_lib.lws_join_stats(h, out, 0) == 0 and list(out) == [0] * 12
    assert hip_lib.lws_join_stats(h, None, 1) == 0                   # reset only
    assert hip_lib.lws_join_stats(None, out, 0) == _lib.LWS_ERR_INVALID
    assert hip_lib.lws_destroy(h) == 0
