"""Argument checks of the minimizer index and matcher entry points
(include/gwamd_cudamapper.h).  Every limit is refused before any device call,
so these run without a GPU."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "claragenomicsanalysis_amd", "lib", "libgwamd.so")
E_INVALID = -1


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "claragenomicsanalysis_amd", "csrc")])
    from claragenomicsanalysis_amd import load_library
    return load_library()


READS = [b"ACGTACGTACGTACGTACGT", b"TTGACCA"]
BASES = b"".join(READS)
OFFSETS = (C.c_int64 * 3)(0, 20, 27)


def create(L, k=5, w=3, first=0, past=2, num_reads=2, filtering=1.0, bases=BASES, offsets=OFFSETS, out="new"):
    h = C.c_void_p()
    rc = L.gwamd_index_create(bases, offsets, num_reads, first, past, k, w, 1, filtering, 0,
                              C.byref(h) if out == "new" else out)
    return rc, h


def refused(L, **kw):
    rc, h = create(L, **kw)
    msg = L.gwamd_last_error()
    assert rc == E_INVALID, (kw, rc)
    assert msg and len(msg) > 0, kw
    assert not h.value
    return msg.decode()


@pytest.mark.parametrize("k", [0, -1, 33, 1000])
def test_kmer_size_limits(L, k):
    assert "kmer_size" in refused(L, k=k)


@pytest.mark.parametrize("w", [0, -3, 256, 100000])
def test_window_size_limits(L, w):
    assert "window_size" in refused(L, w=w)


@pytest.mark.parametrize("f", [-0.001, 1.001, float("nan"), float("inf")])
def test_filtering_parameter_limits(L, f):
    assert "filtering_parameter" in refused(L, filtering=f)


@pytest.mark.parametrize("first,past", [(-1, 1), (2, 1), (0, 3), (3, 3)])
def test_read_range_limits(L, first, past):
    assert "read" in refused(L, first=first, past=past)


def test_negative_read_count_and_bad_offsets(L):
    refused(L, num_reads=-1, past=0)
    refused(L, offsets=(C.c_int64 * 3)(0, 20, 10))
    refused(L, offsets=None)
    refused(L, bases=None)


def test_read_of_two_gib_is_refused(L):
    # positions share 32 bits with the direction in the sort payload; checked
    # on the offsets alone, the bases are never read
    refused(L, offsets=(C.c_int64 * 3)(0, 1 << 31, (1 << 31) + 7))


def test_null_out_pointers(L):
    rc, _ = create(L, out=None)
    assert rc == E_INVALID and L.gwamd_last_error()
    n = C.c_int64()
    p = C.c_void_p()
    assert L.gwamd_match_anchors(None, None, -1, C.byref(p), C.byref(n)) == E_INVALID
    assert L.gwamd_last_error()
    assert L.gwamd_index_info(None, None) == E_INVALID
    assert L.gwamd_index_copy(None, None, None, None, None, None, None) == E_INVALID
    assert L.gwamd_index_create_with_allocator(BASES, OFFSETS, 2, 0, 2, 5, 3, 1, 1.0, 0, None,
                                               C.byref(C.c_void_p())) == E_INVALID


def test_free_of_null_is_a_no_op(L):
    L.gwamd_index_free(None)
    L.gwamd_anchors_free(None)


def test_empty_range_needs_no_device(L):
    # first == past: the empty index, matched against itself
    from claragenomicsanalysis_amd.cudamapper import IndexInfo
    rc, h = create(L, first=1, past=1)
    assert rc == 0 and h.value
    try:
        info = IndexInfo()
        assert L.gwamd_index_info(h, C.byref(info)) == 0
        assert (info.num_elements, info.num_unique_representations, info.number_of_reads,
                info.smallest_read_id, info.largest_read_id, info.number_of_basepairs_in_longest_read) == \
            (0, 0, 0, 0, 0, 0)
        p, n = C.c_void_p(), C.c_int64(7)
        assert L.gwamd_match_anchors(h, h, -1, C.byref(p), C.byref(n)) == 0
        assert n.value == 0 and not p.value
        assert L.gwamd_match_anchors(h, h, -2, C.byref(p), C.byref(n)) == E_INVALID
        assert L.gwamd_match_anchors(h, h, -1, None, C.byref(n)) == E_INVALID
        assert L.gwamd_match_anchors(h, h, -1, C.byref(p), None) == E_INVALID
    finally:
        L.gwamd_index_free(h)


def test_python_classes_raise_value_error(L):
    from claragenomicsanalysis_amd import Index
    for kw in (dict(kmer_size=33, window_size=5), dict(kmer_size=5, window_size=0),
               dict(kmer_size=5, window_size=5, filtering_parameter=2.0),
               dict(kmer_size=5, window_size=5, first_read_id=1, past_the_last_read_id=0)):
        with pytest.raises(ValueError):
            Index(["ACGTACGTACGT"], **kw)
