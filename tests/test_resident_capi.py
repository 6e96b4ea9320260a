"""CPU checks of the entries for reads resident on the device
(include/gwamd_cudamapper.h): they are declared, exported and bound, and they
refuse what can be refused without a handle before any device call, so all of
this runs without a GPU.  The checks that need a handle are in
test_mapper_resident_gpu.py."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "claragenomicsanalysis_amd", "lib", "libgwamd.so")
E_INVALID = -1
NAMES = ("gwamd_device_reads_create", "gwamd_device_reads_free", "gwamd_device_reads_info",
         "gwamd_rescue_overlap_ends_resident", "gwamd_align_overlaps_resident",
         "gwamd_internal_gather_overlap_regions", "gwamd_index_host_copy_create", "gwamd_index_host_copy_to_device",
         "gwamd_index_host_copy_info", "gwamd_index_host_copy_free")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "claragenomicsanalysis_amd", "csrc")])
    from claragenomicsanalysis_amd import load_library
    return load_library()


def offsets(*values):
    return (C.c_int64 * len(values))(*values)


def test_symbols_are_declared_exported_and_bound(L):
    header = open(os.path.join(ROOT, "include", "gwamd_cudamapper.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    exported = subprocess.check_output(["nm", "-D", "--defined-only", LIB]).decode()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert re.search(r" T %s$" % name, exported, flags=re.M), name
        assert getattr(L, name).argtypes is not None
    table = header[:header.index("#ifndef GWAMD_CUDAMAPPER_H")]
    for name in ("gwamd_device_reads_create", "gwamd_rescue_overlap_ends_resident", "gwamd_align_overlaps_resident"):
        assert name in table
    import claragenomicsanalysis_amd as pkg
    assert "DeviceReads" in pkg.__all__ and isinstance(pkg.DeviceReads, type)
    for header_name in ("device_reads.hpp", "overlapper.hpp", "overlap_alignment.hpp"):
        text = open(os.path.join(ROOT, "include", "claraparabricks", "genomeworks", "cudamapper", header_name)).read()
        assert "DeviceReads" in text


def create(L, bases=b"ACGTACGTAC", offs="default", num_reads=2, device_id=0, out="new"):
    if offs == "default":
        offs = offsets(0, 4, 10)
    h = C.c_void_p(7)
    rc = L.gwamd_device_reads_create(bases, offs, num_reads, device_id, None, C.byref(h) if out == "new" else out)
    return rc, h


BAD_READS = {
    "null out": dict(out=None),
    "negative device": dict(device_id=-1),
    "negative count": dict(num_reads=-1),
    "null offsets": dict(offs=None),
    "null bases": dict(bases=None),
    "offsets fall": dict(offs=offsets(0, 6, 4)),
    "negative offset": dict(offs=offsets(-1, 4, 10)),
    "read of 2^31": dict(offs=offsets(0, 4, 4 + (1 << 31))),
}


@pytest.mark.parametrize("name", sorted(BAD_READS))
def test_create_refuses_before_any_device_call(L, name):
    rc, h = create(L, **BAD_READS[name])
    assert rc == E_INVALID and L.gwamd_last_error()
    assert not h.value or name == "null out"


def test_null_handles_are_refused(L):
    from claragenomicsanalysis_amd.cudamapper import Overlap
    arr = (Overlap * 1)(Overlap(0, 0, 0, 1, 0, 1))
    p, n, h = C.c_void_p(7), C.c_int64(7), C.c_void_p(7)
    rc = L.gwamd_rescue_overlap_ends_resident(None, None, arr, 1, 100, 0.9, None, C.byref(p), C.byref(n))
    assert rc == E_INVALID and b"NULL" in L.gwamd_last_error() and not p.value and n.value == 0
    # an empty list does not excuse a NULL handle, a negative count is refused with or without one
    assert L.gwamd_rescue_overlap_ends_resident(None, None, None, 0, 100, 0.9, None, C.byref(p), C.byref(n)) == E_INVALID
    assert L.gwamd_rescue_overlap_ends_resident(None, None, arr, -1, 100, 0.9, None, C.byref(p), C.byref(n)) == E_INVALID
    assert L.gwamd_rescue_overlap_ends_resident(None, None, arr, 1, 100, 0.9, None, None, C.byref(n)) == E_INVALID
    assert L.gwamd_rescue_overlap_ends_resident(None, None, arr, 1, 100, 0.9, None, C.byref(p), None) == E_INVALID
    assert L.gwamd_align_overlaps_resident(None, None, arr, 1, 1, C.byref(h)) == E_INVALID and not h.value
    assert L.gwamd_align_overlaps_resident(None, None, None, 0, 1, C.byref(h)) == E_INVALID
    assert L.gwamd_align_overlaps_resident(None, None, arr, 1, 1, None) == E_INVALID
    out, lens = (C.c_char * 64)(), (C.c_int32 * 2)()
    assert L.gwamd_internal_gather_overlap_regions(None, None, arr, 1, 16, out, lens) == E_INVALID
    assert L.gwamd_internal_gather_overlap_regions(None, None, None, 0, 16, out, lens) == E_INVALID
    assert L.gwamd_device_reads_info(None, C.byref(n), None, None) == E_INVALID
    L.gwamd_device_reads_free(None)


def test_python_refuses_one_handle_and_one_list():
    from claragenomicsanalysis_amd import cudamapper as cm
    fake = cm.DeviceReads.__new__(cm.DeviceReads)
    fake._handle, fake._lib = C.c_void_p(), None
    with pytest.raises(TypeError):
        cm.rescue_overlap_ends([], fake, [b"ACGT"])
    with pytest.raises(TypeError):
        cm.align_overlaps([], [b"ACGT"], fake)
    with pytest.raises(ValueError):  # closed
        cm.rescue_overlap_ends([], fake, fake)


def test_index_host_copy_refuses_null_handles(L):
    from claragenomicsanalysis_amd.cudamapper import IndexInfo
    h, info = C.c_void_p(7), IndexInfo()
    assert L.gwamd_index_host_copy_create(None, 0, 15, 10, C.byref(h)) == E_INVALID and not h.value
    assert L.gwamd_index_host_copy_create(None, 0, 15, 10, None) == E_INVALID
    h = C.c_void_p(7)
    assert L.gwamd_index_host_copy_to_device(None, 0, None, C.byref(h)) == E_INVALID and not h.value
    assert L.gwamd_index_host_copy_to_device(None, 0, None, None) == E_INVALID
    assert L.gwamd_index_host_copy_info(None, C.byref(info), None, None, None) == E_INVALID
    L.gwamd_index_host_copy_free(None)
