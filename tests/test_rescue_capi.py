"""CPU checks of the overlap-end rescue's entry points
(include/gwamd_cudamapper.h): the host round reproduces the reference's known
answer and the model (tests/rescue_model.py) through C and through Python, and
gwamd_rescue_overlap_ends refuses every bad argument before any device call,
so all of this runs without a GPU."""
import ctypes as C
import json
import os
import re
import subprocess

import pytest

import rescue_cases
import rescue_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "claragenomicsanalysis_amd", "lib", "libgwamd.so")
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "rescue_kat.json")))
E_INVALID = -1
NAN = float("nan")
NAMES = ("gwamd_rescue_overlap_ends", "gwamd_rescue_overlap_ends_with_allocator",
         "gwamd_extend_overlap_by_sequence_similarity")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "claragenomicsanalysis_amd", "csrc")])
    from claragenomicsanalysis_amd import load_library
    return load_library()


def as_tuple(o):
    return (o.query_read_id, o.target_read_id, o.query_start, o.query_end, o.target_start, o.target_end, o.strand,
            o.num_residues, bool(o.overlap_complete))


def golden_case():
    case = GOLDEN["extension_case"]
    o = case["overlap"]
    overlap = (3, 4, o["query_start"], o["query_end"], o["target_start"], o["target_end"], o["strand"], 17, True)
    e = case["expected"]
    expected = (3, 4, e["query_start"], e["query_end"], e["target_start"], e["target_end"], o["strand"], 17, True)
    return case, overlap, expected


# ---- symbols --------------------------------------------------------------------

def test_symbols_are_declared_and_exported(L):
    header = open(os.path.join(ROOT, "include", "gwamd_cudamapper.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    exported = subprocess.check_output(["nm", "-D", "--defined-only", LIB]).decode()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert re.search(r" T %s$" % name, exported, flags=re.M), name
        assert getattr(L, name).argtypes is not None
    # the table at the top of the header maps the calls to the reference's
    table = header[:header.index("#ifndef GWAMD_CUDAMAPPER_H")]
    assert "gwamd_rescue_overlap_ends" in table and "overlapper.hpp:95-106" in table
    import claragenomicsanalysis_amd as pkg
    assert "rescue_overlap_ends" in pkg.__all__ and "extend_overlap_by_sequence_similarity" in pkg.__all__
    assert callable(pkg.rescue_overlap_ends) and callable(pkg.extend_overlap_by_sequence_similarity)


# ---- the host round ---------------------------------------------------------------

def test_host_round_reproduces_the_reference_through_c(L):
    from claragenomicsanalysis_amd.cudamapper import Overlap
    case, overlap, expected = golden_case()
    o = Overlap(*overlap)
    q, t = case["query"].encode(), case["target"].encode()
    rc = L.gwamd_extend_overlap_by_sequence_similarity(C.byref(o), q, len(q), t, len(t), case["extension"],
                                                       case["required_similarity"])
    assert rc == 0 and as_tuple(o) == expected
    # a second round has empty windows on both ends: similar, nothing to add
    assert L.gwamd_extend_overlap_by_sequence_similarity(C.byref(o), q, len(q), t, len(t), case["extension"],
                                                         case["required_similarity"]) == 0
    assert as_tuple(o) == expected


def test_host_round_reproduces_the_reference_through_python(L):
    from claragenomicsanalysis_amd import extend_overlap_by_sequence_similarity
    case, overlap, expected = golden_case()
    for kind in (str, str.encode):
        got = extend_overlap_by_sequence_similarity(overlap, kind(case["query"]), kind(case["target"]),
                                                    case["extension"], case["required_similarity"])
        assert as_tuple(got) == expected
    # at 0.9 and at an extension beyond every limit of the device entry point
    for extension, similarity in ((50, 0.9), (1000, 0.8), (-1, 0.8), (0, 0.0)):
        got = extend_overlap_by_sequence_similarity(overlap, case["query"], case["target"], extension, similarity)
        want = model.extend_overlap_by_sequence_similarity(overlap, case["query"], case["target"],
                                                           extension if extension >= 0 else 1 << 32, similarity)
        assert as_tuple(got) == want


def test_host_rounds_equal_the_model_on_the_random_set(L):
    from claragenomicsanalysis_amd import extend_overlap_by_sequence_similarity
    queries, targets, overlaps = rescue_cases.random_set()
    for o in overlaps:
        query, target = queries[o[0]], targets[o[1]]
        want = model.rescue_one(o, query, target)[0]
        cur = o
        if o[6] == "-":  # the caller's part of a Reverse overlap
            target = model.reverse_complement(target)
            cur = o[:4] + (len(target) - o[5], len(target) - o[4]) + o[6:]
        for _ in range(model.ROUNDS):
            cur = as_tuple(extend_overlap_by_sequence_similarity(cur, query, target, model.EXTENSION,
                                                                 model.SIMILARITY))
        if o[6] == "-":
            cur = cur[:4] + (len(target) - cur[5], len(target) - cur[4]) + cur[6:]
        assert cur == want


@pytest.mark.parametrize("length", [0, 1, 14, 15, 16, 29, 30, 31, 33, 63, 64, 65, 99, 100, 128, 300])
def test_host_round_window_lengths_and_repeats(L, length):
    from claragenomicsanalysis_amd import extend_overlap_by_sequence_similarity
    import random
    rng = random.Random(length)
    flanks = [rescue_cases.random_bases(rng, length), b"A" * length, (b"AC" * length)[:length],
              (b"ACGTT" * length)[:length]]
    core = rescue_cases.random_bases(rng, 40)
    for flank in flanks:
        others = [flank, flank[1:] + flank[:1]]
        others += [rescue_cases.substitute(flank, at, rng) for at in {0, 1, length // 2, length - 1}
                   if 0 <= at < length]
        for other in others:
            query, target = flank + core + other, other + core + flank
            o = (0, 0, length, length + 40, length, length + 40, "+", 0, False)
            for similarity in (0.9, 0.5):
                got = extend_overlap_by_sequence_similarity(o, query, target, length, similarity)
                assert as_tuple(got) == model.extend_overlap_by_sequence_similarity(o, query, target, length,
                                                                                   similarity)


def host_round(L, overlap=(0, 0, 2, 6, 2, 6, "+", 0, False), query=b"ACGTACGT", query_len=8, target=b"ACGTACGT",
               target_len=8, similarity=0.9, null_overlap=False):
    from claragenomicsanalysis_amd.cudamapper import Overlap
    o = Overlap(*overlap)
    return L.gwamd_extend_overlap_by_sequence_similarity(None if null_overlap else C.byref(o), query, query_len,
                                                         target, target_len, 100, similarity)


@pytest.mark.parametrize("kw", [dict(null_overlap=True), dict(query=None), dict(target=None), dict(query_len=-1),
                                dict(target_len=1 << 31), dict(similarity=NAN),
                                dict(overlap=(0, 0, 7, 6, 2, 6, "+", 0, False)),
                                dict(overlap=(0, 0, 2, 9, 2, 6, "+", 0, False)),
                                dict(overlap=(0, 0, 2, 6, 7, 6, "+", 0, False)),
                                dict(overlap=(0, 0, 2, 6, 2, 9, "+", 0, False))])
def test_host_round_refuses_bad_arguments(L, kw):
    assert host_round(L) == 0
    assert host_round(L, **kw) == E_INVALID and L.gwamd_last_error()


# ---- the device entry point, before any device call ---------------------------------

def offsets(*values):
    return (C.c_int64 * len(values))(*values)


def rescue(L, query_bases=b"ACGTACGTAC", query_offsets="default", num_queries=2, target_bases=b"ACGTACGTACGT",
           target_offsets="default", num_targets=2, overlaps=((1, 1, 1, 3, 2, 4, "+", 0, True),), n=None,
           extension=100, similarity=0.9, device_id=0, out="new", count="new", allocator="none"):
    from claragenomicsanalysis_amd.cudamapper import Overlap
    if query_offsets == "default":
        query_offsets = offsets(0, 4, 10)
    if target_offsets == "default":
        target_offsets = offsets(0, 6, 12)
    arr = None if overlaps is None else (Overlap * max(1, len(overlaps)))(*[Overlap(*o) for o in overlaps])
    n = len(overlaps) if n is None else n
    p, c = C.c_void_p(7), C.c_int64(7)
    args = [query_bases, query_offsets, num_queries, target_bases, target_offsets, num_targets, arr, n, extension,
            similarity, device_id]
    tail = [C.byref(p) if out == "new" else out, C.byref(c) if count == "new" else count]
    if allocator == "none":
        rc = L.gwamd_rescue_overlap_ends(*args, *tail)
    else:
        rc = L.gwamd_rescue_overlap_ends_with_allocator(*args, allocator, *tail)
    return rc, p, c


BAD_ARGUMENTS = {
    "null overlaps": dict(overlaps=None, n=1),
    "null query offsets": dict(query_offsets=None),
    "null target offsets": dict(target_offsets=None),
    "null query bases": dict(query_bases=None),
    "null target bases": dict(target_bases=None),
    "negative n": dict(n=-1),
    "negative queries": dict(num_queries=-1),
    "negative targets": dict(num_targets=-1),
    "query offsets fall": dict(query_offsets=offsets(0, 6, 4)),
    "target offsets fall": dict(target_offsets=offsets(0, 8, 6)),
    "negative offset": dict(query_offsets=offsets(-1, 4, 10)),
    "query read of 2^31": dict(query_offsets=offsets(0, 4, 4 + (1 << 31))),
    "target read of 2^31": dict(target_offsets=offsets(0, 1 << 31, (1 << 31) + 6)),
    "query id at the count": dict(overlaps=((2, 1, 1, 3, 2, 4, "+", 0, True),)),
    "target id at the count": dict(overlaps=((1, 2, 1, 3, 2, 4, "+", 0, True),)),
    "query id beyond one read": dict(num_queries=1),
    "no targets": dict(num_targets=0),
    "query start after end": dict(overlaps=((1, 1, 4, 3, 2, 4, "+", 0, True),)),
    "query end after the read": dict(overlaps=((1, 1, 1, 7, 2, 4, "+", 0, True),)),
    "target start after end": dict(overlaps=((1, 1, 1, 3, 5, 4, "+", 0, True),)),
    "target end after the read": dict(overlaps=((1, 1, 1, 3, 2, 7, "+", 0, True),)),
    "the second overlap": dict(overlaps=((1, 1, 1, 3, 2, 4, "+", 0, True), (0, 0, 1, 5, 2, 4, "-", 0, True))),
    "strand": dict(overlaps=((1, 1, 1, 3, 2, 4, "*", 0, True),)),
    "strand zero": dict(overlaps=((1, 1, 1, 3, 2, 4, "\0", 0, True),)),
    "negative extension": dict(extension=-1),
    "extension of 129": dict(extension=129),
    "similarity": dict(similarity=NAN),
    "device": dict(device_id=-1),
}


@pytest.mark.parametrize("name", sorted(BAD_ARGUMENTS))
def test_rescue_refuses_before_any_device_call(L, name):
    rc, p, c = rescue(L, **BAD_ARGUMENTS[name])
    assert rc == E_INVALID and L.gwamd_last_error()
    assert not p.value and c.value == 0


def test_null_out_pointers_and_allocator(L):
    assert rescue(L, out=None)[0] == E_INVALID
    assert rescue(L, count=None)[0] == E_INVALID
    rc, p, c = rescue(L, allocator=None)
    assert rc == E_INVALID and not p.value and c.value == 0 and b"allocator" in L.gwamd_last_error()


def test_no_overlaps_succeed_without_a_device(L):
    for kw in (dict(overlaps=()), dict(overlaps=None, n=0), dict(overlaps=(), extension=0, similarity=2.0),
               dict(overlaps=(), query_bases=None, query_offsets=None, num_queries=0, target_bases=None,
                    target_offsets=None, num_targets=0)):
        rc, p, c = rescue(L, **kw)
        assert rc == 0 and not p.value and c.value == 0
    from claragenomicsanalysis_amd import rescue_overlap_ends
    assert rescue_overlap_ends([], [b"ACGT"], [b"ACGT"]) == []
    assert rescue_overlap_ends([], [], []) == []
    # the arguments of an empty list are checked all the same
    assert rescue(L, overlaps=(), extension=129)[0] == E_INVALID
    assert rescue(L, overlaps=(), query_offsets=offsets(0, 6, 4))[0] == E_INVALID


def test_python_raises_value_error(L):
    from claragenomicsanalysis_amd import rescue_overlap_ends
    reads = [b"ACGTACGT", b"ACGTAC"]
    good = [(0, 1, 1, 3, 2, 4, "+", 0, True)]
    for overlaps, kw in (([(2, 1, 1, 3, 2, 4, "+", 0, True)], {}), ([(0, 1, 1, 9, 2, 4, "+", 0, True)], {}),
                         ([(0, 1, 1, 3, 2, 7, "-", 0, True)], {}), ([(0, 1, 1, 3, 2, 4, "x", 0, True)], {}),
                         (good, dict(extension=129)), (good, dict(extension=-1)),
                         (good, dict(required_similarity=NAN)), (good, dict(device_id=-1))):
        with pytest.raises(ValueError):
            rescue_overlap_ends(overlaps, reads, reads, **kw)
