"""The plain-Python model of cudapolish's window cut (tests/polish_model.py)
pinned by the hand-worked cases of tests/polish_cases.py, whose positions can
be checked by eye, and by a few properties of the grouping and stitching."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import polish_cases as pc  # noqa: E402
import polish_model as pm  # noqa: E402

CASES = pc.hand_cases()


@pytest.mark.parametrize("name,overlap,path,expected", CASES, ids=[c[0] for c in CASES])
def test_hand_case(name, overlap, path, expected):
    assert pm.segments(0, overlap, path, pc.W) == expected


def test_every_kind_of_hand_case_is_there():
    names = [c[0] for c in CASES]
    assert len(names) == 2 * (len(pc.HAND) + len(pc.MISFITS)) == 22
    assert sum(n.endswith(", reverse") for n in names) == 11


def test_record_counts_and_order():
    assert pm.window_count(0, 0, 4) == 0 and pm.window_count(5, 5, 4) == 0
    assert pm.window_count(0, 4, 4) == 1 and pm.window_count(0, 5, 4) == 2 and pm.window_count(3, 5, 4) == 2
    overlaps = [pc.overlap_of((0, 8, 0, 8), "+"), pc.overlap_of((0, 0, 4, 4), "+"), pc.overlap_of((3, 6, 5, 7), "-")]
    records = pm.window_segments(overlaps, [[0] * 8, [], [0, 3, 0]], 4)
    assert [(r[0], r[1]) for r in records] == [(0, 0), (0, 1), (2, 1)]


def test_not_aligned_records():
    got = pm.segments(3, pc.overlap_of((0, 8, 0, 8), "-"), [], 4, aligned=False)
    assert got == [(3, 0, 0, 0, 0, 0, pm.REVERSE | pm.EMPTY | pm.NOT_ALIGNED, 0),
                   (3, 1, 0, 0, 0, 0, pm.REVERSE | pm.EMPTY | pm.NOT_ALIGNED, 0)]


def test_a_misfit_leaves_its_neighbours_alone():
    overlaps = [pc.overlap_of((0, 8, 0, 8), "+")] * 3
    records = pm.window_segments(overlaps, [[0] * 8, [0] * 9, [0] * 8], 4)
    assert records[0:2] == pc.records_of(0, pc.HAND[0][3], False)
    assert records[2:4] == pc.misfit_records(1, False)
    assert records[4:6] == pc.records_of(2, pc.HAND[0][3], False)


def test_grouping_and_stitching():
    targets = ["ACGTACGTAC", "GG"]          # windows of 4: ACGT ACGT AC, and GG
    queries = ["TTTTACGAAGT", "AACC"]
    # query 0 [4, 11) on target 0 [0, 8): ACG-TACGT / ACGAAGT... positions are what the records say
    overlaps = [(0, 0, 4, 11, 0, 8, "+"), (1, 0, 0, 4, 4, 8, "-")]
    records = [(0, 0, 4, 7, 0, 3, 0, 0), (0, 1, 7, 11, 4, 8, 0, 0), (1, 1, 0, 4, 4, 8, pm.REVERSE, 0)]
    windows, dropped = pm.build_windows(targets, queries, overlaps, records, 4)
    assert dropped == 0
    assert [(w["target"], w["window"]) for w in windows] == [(0, 0), (0, 1), (0, 2), (1, 0)]
    assert windows[0]["sequences"] == ["ACGT", "ACG"] and windows[0]["t_end"] == [4, 3]
    assert windows[1]["sequences"] == ["ACGT", "AAGT", "GGTT"]  # AACC reverse-complemented
    assert windows[1]["overlap"] == [-1, 0, 1] and windows[1]["t_begin"] == [0, 0, 0]
    assert windows[2]["sequences"] == ["AC"] and windows[3]["sequences"] == ["GG"]
    polished, stats = pm.polish(targets, windows, lambda w: (0, "N" * len(w["sequences"])))
    assert polished == ["ACGT" + "NNN" + "AC", "GG"]
    assert stats == {"windows": 4, "backbone_by_rule": 3, "backbone_by_status": 0}
    polished, stats = pm.polish(targets, windows, lambda w: (4, ""))
    assert polished == targets and stats["backbone_by_status"] == 1


def test_two_percent_rule_and_cap():
    # w = 100: a piece of 2 bases is kept ((2) * 50 >= 100), one of 1 base is not
    targets, queries = ["A" * 100], ["CG"]
    overlaps = [(0, 0, 0, 2, 0, 100, "+")] * 4
    records = [(0, 0, 0, 2, 0, 2, 0, 0), (1, 0, 0, 1, 0, 1, 0, 0), (2, 0, 0, 2, 5, 7, 0, 0), (3, 0, 1, 2, 0, 1, 0, 0)]
    windows, dropped = pm.build_windows(targets, queries, overlaps, records, 100)
    assert windows[0]["overlap"] == [-1, 0, 2] and dropped == 0
    windows, dropped = pm.build_windows(targets, queries, overlaps, records, 100, max_sequences_per_window=2)
    assert windows[0]["overlap"] == [-1, 0] and dropped == 1
