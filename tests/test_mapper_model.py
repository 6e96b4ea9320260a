"""Pins the pure-Python checker (tests/mapper_model.py) of the minimizer index
and the matcher to the reference's known answers
(tests/golden/mapper_kat.json, transcribed from
cudamapper/tests/Test_CudamapperIndexGPU.cu:1436-2360 and
cudamapper/src/index_gpu.cuh:358-381).  No library, no device."""
import json
import os

import pytest

import mapper_model as model

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "mapper_kat.json")))
ARRAYS = ("representations", "read_ids", "positions_in_reads", "directions_of_reads",
          "unique_representations", "first_occurrence_of_representations")
SCALARS = ("number_of_reads", "smallest_read_id", "largest_read_id", "number_of_basepairs_in_longest_read")


@pytest.mark.parametrize("case", GOLDEN["index_cases"], ids=lambda c: c["name"])
def test_model_reproduces_golden_index(case):
    idx = model.Index(case["reads"], case["kmer_size"], case["window_size"], case["first_read_id"],
                      case["past_the_last_read_id"], hash_representations=False,
                      filtering_parameter=case["filtering_parameter"])
    for name in ARRAYS + SCALARS:
        assert getattr(idx, name) == case[name], name


def test_model_filter_reproduces_worked_example():
    ex = GOLDEN["filter_example"]
    b, a = ex["before"], ex["after"]
    assert list(model.first_occurrences(b["representations"])) == \
        [b["unique_representations"], b["first_occurrence_of_representations"]]
    out = model.filter_arrays(b["representations"], b["read_ids"], b["positions_in_reads"],
                              b["directions_of_reads"], ex["filtering_parameter"])
    assert list(out) == [a[name] for name in ARRAYS]


# minimizer.cu:55-66 evaluated step by step in 64-bit unsigned arithmetic
@pytest.mark.parametrize("key,expected", [
    (0x0, 4290886808),
    (0x1, 3079993582),
    (0x2, 1865025060),
    (0xd, 3538353153),
    (0x3fffffff, 144284228),
    (0xffffffff, 3365156203),
    (0x123456789abcdef, 3533963898),
    (0xffffffffffffffff, 3365156203),
])
def test_hash_matches_reference_formula(key, expected):
    assert model.wang_hash(key) == expected


def test_base_codes():
    for ch, v in zip("ACGTacgt", [0, 1, 2, 3, 0, 1, 2, 3]):
        assert model.base_code(ord(ch)) == v
        assert model.complement_code(ord(ch)) == 3 - v
    # other bytes follow the same formulas; N reads as A on both strands
    assert model.base_code(ord("N")) == 0 and model.complement_code(ord("N")) == 0


def test_matcher_model_small():
    reads = ["AAAACTGAA", "GCCAAAG"]
    q = model.Index(reads, 2, 3, 0, 1, hash_representations=False)
    t = model.Index(reads, 2, 3, 1, 2, hash_representations=False)
    # shared representations: AA (query positions 0,1,2,7 x target 3,4) and AG (4 x 5)
    expected = sorted([(0, 1, qp, tp) for qp in (0, 1, 2, 7) for tp in (3, 4)] + [(0, 1, 4, 5)])
    assert model.match_anchors(q, t) == expected
    assert model.match_anchors(q, model.Index(reads, 2, 9, 0, 2, hash_representations=False)) == []
    with pytest.raises(RuntimeError):
        model.match_anchors(q, t, max_anchors=3)
