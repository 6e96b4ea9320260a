"""CPU checks of the overlapper's entry points (include/gwamd_cudamapper.h):
gwamd_post_process_overlaps is host code and is compared with the model
(tests/overlapper_model.py); every argument limit of the device entry points is
refused before any device call, so these run without a GPU."""
import ctypes as C
import json
import os
import random
import subprocess

import pytest

import overlapper_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "claragenomicsanalysis_amd", "lib", "libgwamd.so")
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "overlapper_kat.json")))
E_INVALID = -1
NAN = float("nan")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "claragenomicsanalysis_amd", "csrc")])
    from claragenomicsanalysis_amd import load_library
    return load_library()


def as_tuples(overlaps):
    return [(o.query_read_id, o.target_read_id, o.query_start, o.query_end, o.target_start, o.target_end, o.strand,
             o.num_residues, bool(o.overlap_complete)) for o in overlaps]


def check_post_process(overlaps, drop):
    from claragenomicsanalysis_amd import post_process_overlaps
    got = as_tuples(post_process_overlaps(overlaps, drop))
    assert got == model.post_process_overlaps(overlaps, drop)
    return got


@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("case", GOLDEN["post_process_cases"], ids=lambda c: c["name"])
def test_post_process_golden(L, case, drop):
    got = check_post_process([tuple(o) for o in case["overlaps"]], drop)
    if not drop:
        assert len(got) == case["expected_size"]


def next_overlap(rng, prev, kind):
    """An overlap after prev on the same reads and strand whose gaps make it
    mergeable by one condition alone, or by none."""
    q, t, qs, qe, ts, te, strand, _, _ = prev
    length = rng.randint(50, 3000)
    if kind == "short_gap":  # both gaps below 500, of unlike size
        qg, tg = rng.randint(0, 499), rng.choice([0, 1, 499])
    elif kind == "ratio":  # long gaps of similar size beside short overlaps
        qg = rng.randint(5000, 9000)
        tg = qg - rng.randint(0, qg // 6)
        length = rng.randint(50, 400)
    elif kind == "relative":  # long unlike gaps, short beside the overlaps
        qg, tg = rng.randint(500, 900), rng.randint(1300, 1500)
        length = rng.randint(8000, 12000)
    else:  # long unlike gaps beside short overlaps
        qg, tg = rng.randint(600, 900), rng.randint(3000, 4000)
        length = rng.randint(50, 300)
    nqs = qe + qg
    if strand == "+":
        nts = te + tg
        return (q, t, nqs, nqs + length, nts, nts + length, strand, rng.randint(0, 50), rng.random() < 0.5)
    nte = ts - tg  # the reverse strand walks down the target
    return (q, t, nqs, nqs + length, nte - length, nte, strand, rng.randint(0, 50), rng.random() < 0.5)


def random_overlaps(rng):
    out = []
    for _ in range(rng.randint(1, 5)):  # runs on one read pair and strand
        strand = rng.choice("+-")
        start = rng.randint(100000, 200000)
        length = rng.randint(50, 12000)
        cur = (rng.randint(0, 3), rng.randint(4, 7), start, start + length, 500000, 500000 + length, strand,
               rng.randint(0, 50), rng.random() < 0.5)
        out.append(cur)
        for _ in range(rng.randint(0, 5)):
            cur = next_overlap(rng, cur, rng.choice(["short_gap", "ratio", "relative", "none"]))
            out.append(cur)
    return out


def test_post_process_random_lists(L):
    rng = random.Random(20250219)
    seen = dict(short_gap=0, ratio=0, relative=0, runs=0, ends_in_fuse=0, reverse=0, unmerged=0)
    for _ in range(200):
        overlaps = random_overlaps(rng)
        run = 0
        for a, b in zip(overlaps, overlaps[1:]):
            if model.mergeable(a, b):
                run += 1
                seen["runs"] += run == 2  # three overlaps or more in one fusion
                seen["reverse"] += a[6] == "-"
            else:
                run = 0
                seen["unmerged"] += a[:2] == b[:2] and a[6] == b[6]
        seen["ends_in_fuse"] += run > 0
        for drop in (False, True):
            got = check_post_process(overlaps, drop)
            assert drop or got[:len(overlaps)] == overlaps
    # each condition alone decides some pair
    prev = (0, 1, 1000, 2000, 50000, 51000, "+", 3, True)
    for kind in ("short_gap", "ratio", "relative"):
        for _ in range(20):
            nxt = next_overlap(rng, prev, kind)
            assert model.mergeable(prev, nxt), kind
            seen[kind] += 1
            check_post_process([prev, nxt], False)
    assert not model.mergeable(prev, next_overlap(rng, prev, "none"))
    assert all(v > 0 for v in seen.values()), seen


def test_post_process_arguments(L):
    p, n = C.c_void_p(), C.c_int64(5)
    assert L.gwamd_post_process_overlaps(None, 0, 0, C.byref(p), C.byref(n)) == 0
    assert n.value == 0 and not p.value
    assert L.gwamd_post_process_overlaps(None, -1, 0, C.byref(p), C.byref(n)) == E_INVALID
    assert L.gwamd_post_process_overlaps(None, 2, 0, C.byref(p), C.byref(n)) == E_INVALID
    assert L.gwamd_post_process_overlaps(None, 0, 0, None, C.byref(n)) == E_INVALID
    assert L.gwamd_post_process_overlaps(None, 0, 0, C.byref(p), None) == E_INVALID
    assert L.gwamd_last_error()


ANCHORS = (C.c_uint32 * 16)(*[v for i in range(4) for v in (0, 1, 10 * i, 10 * i)])


def get(L, anchors=ANCHORS, n=4, params=(20, 50, 50, 0.9), device_id=0, out="new", count="new"):
    p, c = C.c_void_p(7), C.c_int64(7)
    rc = L.gwamd_get_overlaps(anchors, n, *params, device_id, C.byref(p) if out == "new" else out,
                              C.byref(c) if count == "new" else count)
    return rc, p, c


@pytest.mark.parametrize("kw", [dict(n=-1), dict(n=(1 << 31) + 1), dict(params=(-1, 50, 50, 0.9)),
                                dict(params=(20, -5, 50, 0.9)), dict(params=(20, 50, -1, 0.9)),
                                dict(params=(20, 50, 50, NAN)), dict(anchors=None), dict(device_id=-1)])
def test_get_overlaps_refuses_before_any_device_call(L, kw):
    rc, p, c = get(L, **kw)
    assert rc == E_INVALID and L.gwamd_last_error()
    assert not p.value and c.value == 0


def test_null_out_pointers(L):
    assert get(L, out=None)[0] == E_INVALID
    assert get(L, count=None)[0] == E_INVALID
    p, c, a = C.c_void_p(), C.c_int64(), C.c_int64()
    assert L.gwamd_match_overlaps(None, None, -1, 20, 50, 50, 0.9, C.byref(p), C.byref(c), C.byref(a)) == E_INVALID
    assert L.gwamd_get_overlaps_with_allocator(ANCHORS, 4, 20, 50, 50, 0.9, 0, None, C.byref(p),
                                               C.byref(c)) == E_INVALID
    assert L.gwamd_match_overlaps_with_allocator(None, None, -1, 20, 50, 50, 0.9, None, C.byref(p), C.byref(c),
                                                 C.byref(a)) == E_INVALID
    assert L.gwamd_last_error()


def test_no_anchors_give_no_overlaps_without_a_device(L):
    rc, p, c = get(L, anchors=None, n=0)
    assert rc == 0 and not p.value and c.value == 0
    from claragenomicsanalysis_amd import get_overlaps
    assert get_overlaps([]) == []


def test_match_overlaps_of_empty_indices_and_bad_parameters(L):
    h = C.c_void_p()
    assert L.gwamd_index_create(b"ACGT", (C.c_int64 * 2)(0, 4), 1, 0, 0, 5, 3, 1, 1.0, 0, C.byref(h)) == 0
    try:
        p, c, a = C.c_void_p(7), C.c_int64(7), C.c_int64(7)
        assert L.gwamd_match_overlaps(h, h, -1, 20, 50, 50, 0.9, C.byref(p), C.byref(c), C.byref(a)) == 0
        assert not p.value and c.value == 0 and a.value == 0
        assert L.gwamd_match_overlaps(h, h, -1, 20, 50, 50, 0.9, C.byref(p), C.byref(c), None) == 0
        for bad in ((-1, 50, 50, 0.9), (20, -1, 50, 0.9), (20, 50, -1, 0.9), (20, 50, 50, NAN)):
            assert L.gwamd_match_overlaps(h, h, -1, *bad, C.byref(p), C.byref(c), C.byref(a)) == E_INVALID
        assert L.gwamd_match_overlaps(h, h, -2, 20, 50, 50, 0.9, C.byref(p), C.byref(c), C.byref(a)) == E_INVALID
        assert L.gwamd_match_overlaps(h, h, -1, 20, 50, 50, 0.9, None, C.byref(c), C.byref(a)) == E_INVALID
    finally:
        L.gwamd_index_free(h)


def test_free_of_null_is_a_no_op(L):
    L.gwamd_overlaps_free(None)


def test_python_raises_value_error(L):
    from claragenomicsanalysis_amd import get_overlaps
    anchors = [(0, 1, 10 * i, 10 * i) for i in range(4)]
    for kw in (dict(min_residues=-1), dict(min_overlap_len=-1), dict(min_bases_per_residue=-1),
               dict(min_overlap_fraction=NAN), dict(device_id=-1)):
        with pytest.raises(ValueError):
            get_overlaps(anchors, **kw)
