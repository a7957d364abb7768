"""The walk plan's place in a view pack (include/lsr.h lsr_view_plan_pack_bytes, lsr_view_plan_layout):
host-only arithmetic, so it is checked without a GPU -- the plan's one segment, the R cover masks, follows
the geometry pack unchanged (lsr_view_pack_bytes), 16-byte aligned, and the pack grows by R bytes rounded
up to 16 and nothing else, for the three shapes tests/test_gpu_view_plan.py runs."""
import ctypes
import os

import pytest

from langsplat_amd import _native

# (W, H, P, capacity_rendered, num_rendered): the two view-cache shapes and the split-replay scene
SHAPES = [(70, 50, 1501, 9000, 7777), (17, 33, 302, 2048, 1001), (48, 32, 3000, 10400, 9288)]


def _up(n):
    return (n + 15) // 16 * 16


def _tiles(W, H):
    return ((W + 15) // 16) * ((H + 15) // 16)


def test_the_library_has_the_plan_entry_points():
    assert _native.has_view_plan()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lsr.h")).read()
    assert "lsr_view_plan_pack_bytes(" in header and "lsr_view_plan_layout(" in header
    assert "#define LSR_ABI_VERSION 18" in header  # additive: detected by symbol


@pytest.mark.parametrize("W,H,P,cap,R", SHAPES)
def test_plan_segments(W, H, P, cap, R):
    lay = _native.view_plan_layout(P, W, H, cap, R)
    T = _tiles(W, H)
    geometry = _native.view_pack_bytes(P, W, H, R)
    assert lay["tiles"] == T and lay["classes"] == 64 and lay["split_items"] == 4
    assert lay["word_plan_ready"] == 8 and lay["word_bwd_class"] == 16 + 64
    # the geometry pack is a prefix: the plan starts where a pack without one ends
    assert lay["pack_counters"] == 0 and lay["pack_cover"] == geometry
    assert lay["pack_cover"] % 16 == 0
    assert lay["pack_bytes"] == geometry + _up(R) == _native.view_plan_pack_bytes(P, W, H, R)
    assert lay["pack_bytes"] % 16 == 0 and lay["pack_bytes"] > geometry


@pytest.mark.parametrize("W,H,P,cap,R", SHAPES)
def test_set_arrays(W, H, P, cap, R):
    """Where lsr_view_save reads the plan from, and where the set keeps what else a compositing leaves
    for the backward: the state layout's own offsets, 16-byte aligned, and none of it depends on the
    view's count."""
    lay = _native.view_plan_layout(P, W, H, cap, R)
    st = _native.state_layout(P, W, H, cap)
    assert (lay["set_counters"], lay["set_final_T"], lay["set_n_contrib"]) == (st["counters"], st["final_T"],
                                                                               st["n_contrib"])
    for name in ("set_cover", "set_final_T", "set_n_contrib", "set_split_desc", "set_bwd_lists", "set_loss_code"):
        assert lay[name] % 16 == 0, name
    assert lay["set_cover"] >= 4 * cap  # after the point list of the set's capacity
    again = _native.view_plan_layout(P, W, H, cap, 0)
    assert all(again[k] == lay[k] for k in lay if k.startswith("set_"))
    assert lay["set_n_contrib"] - lay["set_final_T"] >= 4 * W * H


def test_sizes_grow_with_the_view_and_bad_arguments_are_refused():
    f = _native.view_plan_pack_bytes
    sizes = [f(300, 70, 50, R) for R in range(0, 40)]
    assert sizes == sorted(sizes) and sizes[0] < sizes[-1]
    for bad in ((0, 70, 50, 0), (1, 0, 50, 0), (1, 70, 0, 0), (1, 70, 50, -1)):
        assert f(*bad) == 0
    lib = _native.load()
    out = _native.LsrViewPlanOffsets()
    for bad in ((0, 70, 50, 10, 5), (1, 70, 50, 0, 0), (1, 70, 50, 10, 11), (1, 70, 50, 10, -1)):
        assert lib.lsr_view_plan_layout(*bad, ctypes.byref(out)) == 1, bad
    assert lib.lsr_view_plan_layout(1, 70, 50, 10, 5, None) == 1
