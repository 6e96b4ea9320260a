"""The index caches, the host copy of an index and the aligner's device-added
batches, checked from C++ on the GPU: tests/index_cache_check.cpp is compiled
against the public headers and libgwamd.so and run as a child process on the
reference's two small FASTA fixtures."""
import os
import random
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENARIOS = ["host_copy", "host_cache_not_the_same", "host_cache_the_same", "device_cache_not_the_same",
             "device_cache_the_same", "aligner_batches"]


def test_index_cache_check(tmp_path):
    exe = tmp_path / "index_cache_check"
    lib = os.path.join(ROOT, "claragenomicsanalysis_amd", "lib")
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-std=c++17", "-O1", "-Wall",
                           "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "claragenomicsanalysis_amd", "csrc"), "-I", "/opt/rocm/include",
                           "-x", "c++", os.path.join(ROOT, "tests", "index_cache_check.cpp"), "-L", lib, "-lgwamd",
                           "-Wl,-rpath," + lib, "-o", str(exe)])
    golden = os.path.join(ROOT, "tests", "golden")
    r = subprocess.run([str(exe), os.path.join(golden, "catcaag_aagcta.fasta"),
                        os.path.join(golden, "aaaactgaa_gccaaag.fasta")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == [word for name in SCENARIOS for word in ("ok", name)]


ARRAYS = ("representations", "read_ids", "positions_in_reads", "directions_of_reads", "unique_representations",
          "first_occurrence_of_representations")
GETTERS = ("number_of_reads", "smallest_read_id", "largest_read_id", "number_of_basepairs_in_longest_read")


def same_index(a, b):
    return all(np.array_equal(getattr(a, name), getattr(b, name)) for name in ARRAYS) and \
        all(getattr(a, name) == getattr(b, name) for name in GETTERS)


def test_python_index_host_copy_round_trip():
    from claragenomicsanalysis_amd import Index, IndexHostCopy, match_anchors
    from claragenomicsanalysis_amd.cudaaligner import DeviceAllocator
    rng = random.Random(9)
    genome = "".join(rng.choice("ACGT") for _ in range(1500))
    reads = [genome[s:s + 500] for s in (0, 200, 400, 700, 1000)] + ["ACGT"]
    with Index(reads, 15, 5, 1, 4) as index, Index(reads, 15, 5) as whole:
        assert len(index.representations) > 50 and (index.smallest_read_id, index.largest_read_id) == (1, 3)
        want = match_anchors(index, whole)
        assert len(want) > 50
        copy = IndexHostCopy(index, 1, 15, 5)
        assert (copy.first_read_id, copy.kmer_size, copy.window_size) == (1, 15, 5)
        assert (copy.num_elements, copy.number_of_reads, copy.number_of_basepairs_in_longest_read) == \
            (len(index.representations), 3, 500)
        pool = DeviceAllocator(1 << 20)
        with copy.copy_index_to_device(allocator=pool) as back:
            assert same_index(back, index)
            n, u = len(index.representations), len(index.unique_representations)
            assert pool.used == n * 17 + u * 8 + (u + 1) * 4
            # matching the copied-back index gives the anchors of the original
            assert np.array_equal(match_anchors(back, whole), want)
        assert pool.used == 0
    # the copy outlives the index it was made from
    with copy.copy_index_to_device() as back, Index(reads, 15, 5, 1, 4) as index:
        assert same_index(back, index)
    copy.close()
    with pytest.raises(ValueError):
        copy.copy_index_to_device()
    with pytest.raises(ValueError):
        IndexHostCopy(index, 1, 15, 5)  # a closed index
    # an empty index round-trips, and so does one of reads that are all too short
    for first, past in ((2, 2), (5, 6)):
        with Index(reads, 15, 5, first, past) as empty, IndexHostCopy(empty, first, 15, 5) as empty_copy:
            assert empty_copy.num_elements == 0
            with empty_copy.copy_index_to_device() as back:
                assert same_index(back, empty) and len(back.representations) == 0
    with Index(reads, 15, 5) as whole:
        for k, w in ((0, 5), (33, 5), (15, 0), (15, 256)):
            with pytest.raises(ValueError):
                IndexHostCopy(whole, 0, k, w)
