"""The grouping of cut records into POA windows, without a GPU: the cases of
polish_group_cases.py are pinned against the Python model through the host's
build_window_slices, and the device entries refuse bad arguments before any
device call.
"""
import ctypes as C

import numpy as np
import pytest

import polish_group_cases as gc
from claragenomicsanalysis_amd import cudapolish
from claragenomicsanalysis_amd._lib import load_library

CASES = gc.all_cases()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_host_grouping_equals_the_model(case):
    assert gc.host_slices(cudapolish, case) == gc.model_view(case)


def test_the_cases_cover_what_they_claim():
    by_name = {c["name"]: c for c in CASES}
    _, by_cap, by_quality = gc.model_view(by_name["seeded"])
    assert by_cap > 0 and by_quality > 0 and len(by_name["seeded"]["records"]) == 2000
    windows, by_cap, by_quality = gc.model_view(by_name["interleaved, 130 at cap 100"])
    assert by_cap == 31 and [len(w["slices"]) for w in windows] == [45, 100, 44]
    windows, by_cap, by_quality = gc.model_view(by_name["filter before cap"])
    assert (by_cap, by_quality) == (0, 3) and len(windows[0]["slices"]) == 4
    windows, by_cap, by_quality = gc.model_view(by_name["mean equal to the threshold"])
    assert by_quality == 3 and [len(w["slices"]) for w in windows] == [2, 3, 2, 1]
    _, _, by_quality = gc.model_view(by_name["quality alignment, threshold 200"])
    assert 0 < by_quality < len(by_name["quality alignment, threshold 200"]["records"])
    assert gc.model_view(by_name["quality alignment, threshold 0"])[2] == 0
    windows, _, _ = gc.model_view(by_name["two percent"])
    assert [len(w["slices"]) for w in windows] == [1, 2, 1]
    for cap in (1, 2, 5):
        windows, by_cap, _ = gc.model_view(by_name["cap %d" % cap])
        assert [len(w["slices"]) - 1 for w in windows] == [max(cap - 2, 0), cap - 1, cap - 1, cap - 1]
        assert by_cap == 1 + 2


REFUSED = gc.refused_calls()


@pytest.mark.parametrize("case", [c for _, c in REFUSED], ids=[name for name, _ in REFUSED])
def test_device_grouping_refuses_before_any_device_call(case):
    """These hold on a machine without a GPU: nothing reaches the device."""
    with pytest.raises(ValueError):
        cudapolish.build_window_slices_device(case["target_lengths"], case["query_lengths"], case["overlaps"],
                                              gc.segment_array(case), case["w"], case["cap"],
                                              quality_threshold=case["tenths"] / 10.0)


def test_device_grouping_refuses_other_arguments():
    c = gc.flags_case()
    with pytest.raises(ValueError):
        cudapolish.build_window_slices_device(c["target_lengths"], c["query_lengths"], c["overlaps"],
                                              gc.segment_array(c), c["w"], device_id=-1)
    with pytest.raises(TypeError):
        cudapolish.build_window_slices_device(c["target_lengths"], c["query_lengths"], c["overlaps"],
                                              gc.segment_array(c), c["w"], query_reads="ACGT")
    with pytest.raises(TypeError):
        cudapolish.window_slices_resident(c["overlaps"], ["ACGT"], ["ACGT"], 4)


def test_add_poa_groups_refuses_without_a_batch():
    """gwamd_poa_add_poa_groups_resident: the argument errors that need no batch on a device."""
    L = load_library()
    added = C.c_int32(7)
    counts = np.array([1], np.int32)
    status = np.zeros(4, np.int32)
    slices = np.zeros(1, cudapolish.SLICE_DTYPE)
    args = (None, 0, slices.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p), 1,
            status.ctypes.data_as(C.c_void_p), status.ctypes.data_as(C.c_void_p))
    assert L.gwamd_poa_add_poa_groups_resident(None, *args, C.byref(added)) == -1  # a NULL batch
    assert added.value == 0
    assert "batch is NULL" in cudapolish.load_library().gwamd_last_error().decode()
