"""The plain-Python overlapper model (tests/overlapper_model.py) against the
reference's known answers (tests/golden/overlapper_kat.json)."""
import json
import os

import pytest

import overlapper_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "overlapper_kat.json")))
FIELDS = GOLDEN["overlap_fields"]


def call(case):
    return model.get_overlaps(case["anchors"], case["min_residues"], case["min_overlap_len"],
                              case["min_bases_per_residue"], case["min_overlap_fraction"])


def check_expected_fields(overlaps, case):
    """overlaps: argument tuples of Overlap."""
    assert len(overlaps) == case["expected_size"]
    for o, want in zip(overlaps, case["expected_fields"]):
        got = dict(zip(FIELDS, o))
        for name, value in want.items():
            if name == "target_end_greater_than_target_start":
                assert got["target_end"] > got["target_start"]
            else:
                assert got[name] == value, name


@pytest.mark.parametrize("case", GOLDEN["anchor_cases"], ids=lambda c: c["name"])
def test_golden_anchor_cases(case):
    overlaps, counts = call(case)
    check_expected_fields(overlaps, case)
    assert counts["overlaps"] == len(overlaps) <= counts["groups"] <= counts["kept"] <= counts["chains"]


@pytest.mark.parametrize("case", GOLDEN["post_process_cases"], ids=lambda c: c["name"])
def test_golden_post_process_cases(case):
    out = model.post_process_overlaps(case["overlaps"], case["drop_fused_overlaps"])
    assert len(out) == case["expected_size"]
    assert out[:len(case["overlaps"])] == [tuple(o) for o in case["overlaps"]]


def test_chain_relation_is_adjacent_only():
    # 0 -> 140 -> 280: each step is within reach, the ends are not; one chain
    anchors = [(0, 1, 100 + 140 * i, 1000 + 140 * i) for i in range(3)]
    overlaps, counts = model.get_overlaps(anchors, 0, 0, 1000, 0.0)
    assert counts == dict(chains=1, kept=1, groups=1, overlaps=1)
    assert overlaps == [(0, 1, 100, 380, 1000, 1280, "+", 3, True)]


def test_group_spans_a_dropped_chain():
    a = [(0, 1, 100 + 10 * i, 1000 + 10 * i) for i in range(3)]
    short = [(0, 1, 400, 1300), (0, 1, 410, 1310)]
    b = [(0, 1, 700 + 10 * i, 1600 + 10 * i) for i in range(4)]
    overlaps, counts = model.get_overlaps(a + short + b, 0, 0, 1000, 0.0)
    assert counts == dict(chains=3, kept=2, groups=1, overlaps=1)
    assert overlaps == [(0, 1, 100, 730, 1000, 1630, "+", 7, True)]


def test_filter_edges():
    three = [(0, 1, 100, 100), (0, 1, 100, 100), (0, 1, 100, 100)]
    assert model.get_overlaps(three, 0, 0, 1000, 0.0)[0] == []  # 0 / 0 is NaN
    # target span 9 of query span 10: exactly the fraction, rejected
    nine_tenths = [(0, 1, 0, 0), (0, 1, 5, 5), (0, 1, 10, 9)]
    assert model.get_overlaps(nine_tenths, 0, 0, 1000, 0.9)[0] == []
    assert len(model.get_overlaps(nine_tenths, 0, 0, 1000, 0.89)[0]) == 1


def test_bad_input_is_refused():
    with pytest.raises(ValueError):
        model.get_overlaps([(0, 1, 5, 5), (0, 1, 4, 9)])
    with pytest.raises(ValueError):
        model.get_overlaps([(0, 1, 5, 1 << 31)])


def test_end_of_list_fusion_copies_the_last_but_one():
    o = [(1, 2, 0, 100, 0, 100, "+", 3, True), (1, 2, 110, 200, 110, 200, "+", 4, False),
         (1, 2, 210, 300, 210, 300, "+", 5, True)]
    out = model.post_process_overlaps(o)
    assert out[3:] == [(1, 2, 0, 300, 0, 300, "+", 12, False)]
    assert model.post_process_overlaps(o, True) == out[3:]
    # ended by a fourth overlap that cannot be merged: the fields of the fusion's last overlap
    out = model.post_process_overlaps(o + [(1, 3, 0, 100, 0, 100, "+", 3, True)])
    assert out[4:] == [(1, 2, 0, 300, 0, 300, "+", 12, True)]
