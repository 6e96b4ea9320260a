"""cudapolish's window grouping on the GPU (polish_group.hip) against the host's
build_window_slices: every array of the view and both counters, on the cases of
polish_group_cases.py.  The host's view is itself pinned to the Python model in
test_polish_group_cpu.py.
"""
import pytest

import polish_group_cases as gc
from claragenomicsanalysis_amd import cudapolish
from claragenomicsanalysis_amd.cudamapper import DeviceReads

pytestmark = pytest.mark.gpu

CASES = gc.all_cases()


def device_view(case, **kwargs):
    """(windows, dropped_by_cap, dropped_by_quality) of build_window_slices_device."""
    segments = gc.segment_array(case)
    args = (case["target_lengths"], case["query_lengths"], case["overlaps"], segments, case["w"], case["cap"])
    if case["qualities"] is None and not kwargs.pop("resident_anyway", False):
        got = cudapolish.build_window_slices_device(*args, quality_threshold=case["tenths"] / 10.0, **kwargs)
    else:
        with DeviceReads(gc.query_texts(case), qualities=case["qualities"]) as reads:
            got = cudapolish.build_window_slices_device(*args, query_reads=reads,
                                                        quality_threshold=case["tenths"] / 10.0, **kwargs)
    assert got.slices.dtype == cudapolish.SLICE_DTYPE and len(got) == len(got.counts) == len(got.target)
    assert len(got.slices) == len(got.overlap) == len(got.t_begin) == len(got.t_end) == int(got.counts.sum())
    return got.windows(), got.dropped_by_cap, got.dropped_by_quality


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_device_grouping_equals_the_host(case):
    expected = gc.host_slices(cudapolish, case)
    got = device_view(case)
    print("windows %d, sequences %d, dropped by cap %d, by quality %d"
          % (len(got[0]), sum(len(w["slices"]) for w in got[0]), got[1], got[2]))
    assert got[1:] == expected[1:]
    assert got[0] == expected[0]


def test_seeded_case_drops_by_both_rules():
    case = gc.seeded_case()
    _, by_cap, by_quality = gc.model_view(case)
    assert by_cap > 0 and by_quality > 0
    assert device_view(case)[1:] == (by_cap, by_quality)


def test_reads_without_qualities_do_not_filter():
    """A handle that carries no qualities: no filter, whatever the threshold."""
    case = gc.quality_alignment_case(200, with_qualities=False)
    got = device_view(case, resident_anyway=True)
    assert got == gc.host_slices(cudapolish, case) and got[2] == 0


def test_the_same_input_gives_the_same_bytes():
    case = gc.seeded_case()
    with DeviceReads(gc.query_texts(case), qualities=case["qualities"]) as reads:
        runs = [cudapolish.build_window_slices_device(case["target_lengths"], case["query_lengths"],
                                                      case["overlaps"], gc.segment_array(case), case["w"],
                                                      case["cap"], query_reads=reads, quality_threshold=20.0)
                for _ in range(3)]
    for other in runs[1:]:
        for name in ("slices", "counts", "target", "index", "overlap", "t_begin", "t_end"):
            assert getattr(other, name).tobytes() == getattr(runs[0], name).tobytes()


def test_reads_of_another_set_are_refused():
    case = gc.flags_case()
    with DeviceReads(["ACGT"]) as reads:
        with pytest.raises(ValueError):
            cudapolish.build_window_slices_device(case["target_lengths"], case["query_lengths"], case["overlaps"],
                                                  gc.segment_array(case), case["w"], query_reads=reads)


def test_pool_is_returned():
    from claragenomicsanalysis_amd.cudaaligner import DeviceAllocator
    case = gc.seeded_case()
    expected = gc.host_slices(cudapolish, case)
    pool = DeviceAllocator(64 << 20)
    assert pool.used == 0
    with DeviceReads(gc.query_texts(case), qualities=case["qualities"]) as reads:
        args = (case["target_lengths"], case["query_lengths"], case["overlaps"], gc.segment_array(case), case["w"],
                case["cap"])
        got = cudapolish.build_window_slices_device(*args, query_reads=reads, quality_threshold=20.0, allocator=pool)
        assert pool.used == 0
        assert (got.windows(), got.dropped_by_cap, got.dropped_by_quality) == expected
        small = DeviceAllocator(16 << 10)  # the 2,000 records alone are 64,000 bytes
        with pytest.raises(RuntimeError):
            cudapolish.build_window_slices_device(*args, query_reads=reads, quality_threshold=20.0, allocator=small)
        assert small.used == 0
