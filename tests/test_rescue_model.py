"""The plain-Python model of the overlap-end rescue (tests/rescue_model.py)
reproduces the reference's known answers (tests/golden/rescue_kat.json), and
the random set the GPU test runs (tests/rescue_cases.py) exercises every
outcome.  No GPU and no library."""
import json
import os

import numpy as np
import pytest

import rescue_cases
import rescue_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "rescue_kat.json")))


def golden_overlap(case):
    o = case["overlap"]
    return (0, 0, o["query_start"], o["query_end"], o["target_start"], o["target_end"], o["strand"], 0, False)


def positions(overlap):
    return dict(zip(("query_start", "query_end", "target_start", "target_end"), overlap[2:6]))


def test_reference_extension_case():
    case = GOLDEN["extension_case"]
    args = (case["query"], case["target"], case["extension"], case["required_similarity"])
    got = model.extend_overlap_by_sequence_similarity(golden_overlap(case), *args)
    assert positions(got) == case["expected"]
    # both ends are at their read's end after one round: three rounds give the same
    rescued, head, tail = model.rescue_one(golden_overlap(case), *args)
    assert rescued == got and head == [1, 0, 0] and tail == [24, 0, 0]


@pytest.mark.parametrize("case", GOLDEN["similarity_cases"], ids=lambda c: c["name"])
def test_reference_similarity_cases(case):
    got = model.similarity(case["a"], case["b"], case["kmer_size"])
    assert got.dtype == np.float32
    if "equals" in case:
        assert got == case["equals"]
    else:
        assert case["greater_than"] < got < case["less_than"]


def test_third_similarity_case_is_four_of_sixteen():
    case = GOLDEN["similarity_cases"][2]
    assert model.shared_and_union(case["a"], case["b"], case["kmer_size"]) == (4, 16)


@pytest.mark.parametrize("case", GOLDEN["kmer_cases"], ids=lambda c: repr(c["s"]))
def test_reference_kmer_cases(case):
    kmers = model.split_into_kmers(case["s"], case["kmer_size"])
    assert len(kmers) == case["count"]
    assert kmers[0] == case["first"].encode() and kmers[-1] == case["last"].encode()


def test_substrings_grow_with_their_index():
    # substr(i, i + k): the count grows with i and is clipped at the end
    assert model.split_into_kmers("AAACCTTCTCT", 4) == [b"AAAC", b"AACCT", b"ACCTTC", b"CCTTCTC", b"CTTCTCT",
                                                       b"TTCTCT", b"TCTCT", b"CTCT"]
    assert model.split_into_kmers("ACGT", 15) == [b"ACGT"] and model.split_into_kmers("", 15) == [b""]
    lengths = [len(s) for s in model.split_into_kmers(bytes(100), 15)]
    assert len(lengths) == 86 and lengths == [min(i + 15, 100 - i) for i in range(86)]


def test_complement_table_and_middle_base():
    assert model.COMPLEMENT == GOLDEN["complement"] and len(model.COMPLEMENT) == 26
    assert model.reverse_complement(b"AACG") == b"CGTT"
    assert model.reverse_complement(b"AACGT") == b"ACCTT"  # the middle C stays
    assert model.reverse_complement(b"ANRT") == b"ARNT"
    assert model.reverse_complement(b"Aa\x80\xffT") == b"A\xff\x80aT"
    assert model.reverse_complement(b"") == b"" and model.reverse_complement(b"A") == b"A"


def test_threshold_is_float32():
    flank = b"GATTACAGGCTTAACCGGATCTAGCATGCAATG"
    assert len(flank) == 33
    first = b"C" + flank[1:]  # only substring 0 holds the first base
    assert model.shared_and_union(flank, first) == (18, 20)
    quotient = np.float32(18) / np.float32(20)
    assert quotient == np.float32(0.9) and float(quotient) < 0.9  # equal to 0.9f, below the double 0.9
    assert model.accepted(flank, first, 0.9)
    second = flank[:1] + b"C" + flank[2:]  # substrings 0 and 1 hold the second base
    assert model.shared_and_union(flank, second) == (17, 21) and not model.accepted(flank, second, 0.9)


def test_empty_windows_are_similar():
    assert model.similarity(b"", b"") == 1
    o = (0, 0, 0, 10, 5, 15, "+", 0, False)
    assert model.extend_overlap_by_sequence_similarity(o, b"A" * 10, b"C" * 15, 100, 0.9) == o


def test_random_set_exercises_every_outcome():
    queries, targets, overlaps = rescue_cases.random_set()
    assert len(overlaps) == 400 and {o[6] for o in overlaps} == {"+", "-"}
    outcomes = rescue_cases.outcomes(queries, targets, overlaps)
    head_only = sum(1 for h, t, _ in outcomes if h and not t)
    tail_only = sum(1 for h, t, _ in outcomes if t and not h)
    both = sum(1 for h, t, _ in outcomes if h and t)
    neither = sum(1 for h, t, _ in outcomes if not h and not t)
    print("head only %d, tail only %d, both %d, neither %d, more than one round %d"
          % (head_only, tail_only, both, neither, sum(1 for o in outcomes if o[2])))
    assert min(head_only, tail_only, both, neither) >= 20
    assert sum(1 for o in outcomes if o[2]) >= 100
