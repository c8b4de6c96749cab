"""The case table of tests/test_gpu_stream_order.py is complete: every C-ABI function whose prototype ends in `void *stream`, read
from the headers with the reader lwsnet_amd._lib binds the library with, has a row or is excluded with a reason.  A new entry
point with a stream therefore fails here until it is held to that stream under a stalled device."""
import pytest

torch = pytest.importorskip("torch")

import stream_stall as SS  # noqa: E402
import test_gpu_stream_order as SO  # noqa: E402
from lwsnet_amd import _lib  # noqa: E402


def functions_with_a_stream():
    return {name for _, spellings, _ in _lib.ABI.values() for name, (_, params) in spellings.items() if params and params[-1] == "void *"}


def test_every_function_with_a_stream_has_a_row_or_a_reason():
    have = functions_with_a_stream()
    assert "lws_forward" in have and "lws_tsdf_points" in have and "lws_pool_submit" not in have        # the reader reads what it should
    assert not set(SO.TABLE) & set(SO.EXCLUDED)
    missing = have - set(SO.TABLE) - set(SO.EXCLUDED)
    assert not missing, f"no stream-order case for {sorted(missing)}"
    stale = (set(SO.TABLE) | set(SO.EXCLUDED)) - have
    assert not stale, f"{sorted(stale)} are not functions with a stream parameter"
    assert all(len(reason.split()) >= 5 for reason in SO.EXCLUDED.values()) and len(SO.EXCLUDED) <= 3
    assert set(SO.TABLE.values()) == set(SO.SCENARIOS)


def test_the_last_parameter_is_what_marks_a_stream():
    """`after_stream` of lws_pool_submit is not the last parameter: the pool has cases of its own."""
    protos = _lib.ABI["lwsnet_hip.h"][1]
    assert protos["lws_pool_submit"][1][-2:] == ["void *", "int64_t *"]
    assert protos["lws_lr_pairs"][1][-1] == "void *" and protos["lws_reserve"][1][-1] == "int"


def test_a_stall_is_bounded():
    assert 0 < SS.STALL_MS <= SS.MAX_STALL_MS <= 250.0
    with pytest.raises(AssertionError):
        SS.stall(None, SS.MAX_STALL_MS + 1.0)
    with pytest.raises(AssertionError):
        SS.stall(None, 0.0)
