"""GPU checks of the (k,w)-minimizer index and the anchor matcher
(csrc/mapper_index.hip, mapper_match.hip) against the reference's known
answers (tests/golden/mapper_kat.json) and the plain-Python model
(tests/mapper_model.py, itself pinned by test_mapper_model.py).  All outputs
are integers and compared exactly."""
import json
import os
import random
import subprocess

import numpy as np
import pytest

import mapper_model as model
from claragenomicsanalysis_amd import Index, match_anchors
from claragenomicsanalysis_amd.cudamapper import ANCHOR_DTYPE, read_fasta

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "mapper_kat.json")))
ARRAYS = ("representations", "read_ids", "positions_in_reads", "directions_of_reads",
          "unique_representations", "first_occurrence_of_representations")
SCALARS = ("number_of_reads", "smallest_read_id", "largest_read_id", "number_of_basepairs_in_longest_read")
TILE = 2048  # windows per workgroup of the sketch kernel (kTile, mapper_index.hip)


def assert_index_equal(got, expected):
    """expected: a model.Index or a golden case (dict)."""
    for name in ARRAYS + SCALARS:
        want = expected[name] if isinstance(expected, dict) else getattr(expected, name)
        have = getattr(got, name)
        if name in ARRAYS:
            have = have.tolist()
        assert have == want, name


def check_against_model(reads, k, w, **kw):
    with Index(reads, k, w, **kw) as got:
        expected = model.Index(reads, k, w, **kw)
        assert_index_equal(got, expected)
        return expected


def random_read(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


@pytest.fixture(scope="module")
def reads8():
    rng = random.Random(20240611)
    return [random_read(rng, rng.randint(300, 700)) for _ in range(8)]


@pytest.mark.parametrize("case", GOLDEN["index_cases"], ids=lambda c: c["name"])
def test_golden_index(case):
    with Index(case["reads"], case["kmer_size"], case["window_size"], case["first_read_id"],
               case["past_the_last_read_id"], hash_representations=False,
               filtering_parameter=case["filtering_parameter"]) as idx:
        assert_index_equal(idx, case)


@pytest.mark.parametrize("k,w,hashed", [(15, 5, True), (5, 10, False), (32, 1, False), (1, 255, True),
                                        (1, 255, False)])
def test_model_parity_random_reads(reads8, k, w, hashed):
    m = check_against_model(reads8, k, w, hash_representations=hashed)
    assert len(m.representations) > 0
    if k == 32:  # full 64-bit keys
        assert max(m.representations) >= 1 << 63


@pytest.mark.parametrize("w", [2, 64])
@pytest.mark.parametrize("windows", [3 * TILE + 37, TILE, TILE + 1])
def test_tile_seams(w, windows):
    k = 15
    rng = random.Random(windows * 1000 + w)
    read = random_read(rng, windows + k - w)  # windows = n - k + w
    m = check_against_model([read], k, w)
    assert m.number_of_basepairs_in_longest_read == len(read)


def test_tile_seam_with_ties():
    # a constant read makes every window's minimizer its last k-mer, across the seams too
    read = "A" * (2 * TILE + 100)
    m = check_against_model([read], 5, 10, hash_representations=False)
    assert m.positions_in_reads == list(range(len(read) - 4))


def test_long_read_between_short_ones():
    rng = random.Random(5)
    reads = [random_read(rng, 300), random_read(rng, 2 * TILE + 900), random_read(rng, 200),
             random_read(rng, TILE + 15 - 5)]
    check_against_model(reads, 15, 5)


@pytest.mark.parametrize("read,k,w", [("A" * 300, 5, 10), ("AC" * 200, 4, 7), ("ACGT" * 100, 4, 4)])
def test_ties(read, k, w):
    for hashed in (False, True):
        m = check_against_model([read], k, w, hash_representations=hashed)
        if read[0] == read[1]:
            assert len(m.representations) == len(read) - k + 1  # every position is a sketch element


def test_short_read_in_the_middle_keeps_ids():
    rng = random.Random(6)
    reads = [random_read(rng, 200), random_read(rng, 18), random_read(rng, 150), "", random_read(rng, 19)]
    m = check_against_model(reads, 15, 5)  # one window covers 19 bases
    assert sorted(set(m.read_ids)) == [0, 2, 4] and m.number_of_reads == 5 and m.largest_read_id == 4
    m = check_against_model(reads, 15, 5, first_read_id=1, past_the_last_read_id=4)
    assert sorted(set(m.read_ids)) == [2] and m.number_of_reads == 3 and m.smallest_read_id == 1


def test_all_reads_too_short_gives_empty_index(reads8):
    reads = ["ACGTACGTAC", "ACGT", ""]
    m = check_against_model(reads, 8, 4)
    assert m.number_of_reads == 0 and m.first_occurrence_of_representations == []
    with Index(reads, 8, 4) as empty, Index(reads8, 15, 5) as full:
        for q, t in ((empty, full), (full, empty), (empty, empty)):
            a = match_anchors(q, t)
            assert a.dtype == ANCHOR_DTYPE and len(a) == 0


def test_non_acgt_bytes(reads8):
    rng = random.Random(7)
    read = random_read(rng, 400, "ACGTNacgtnRYKM-*")
    for hashed in (False, True):
        check_against_model([read, reads8[0].lower(), b"\x00\xff\x80ACGT" * 20], 7, 6, hash_representations=hashed)


@pytest.mark.parametrize("filtering", [0.02, 0.0, 0.5, 1.0])
def test_filtering(filtering):
    rng = random.Random(8)
    # three letters, biased towards A: a few representations hold most elements
    reads = [random_read(rng, rng.randint(200, 500), "AAAAAACCCG") for _ in range(6)]
    for hashed in (False, True):
        m = check_against_model(reads, 6, 4, hash_representations=hashed, filtering_parameter=filtering)
        unfiltered = model.Index(reads, 6, 4, hash_representations=hashed)
        if filtering == 0.0:
            assert m.representations == [] and m.number_of_reads == 6
        elif filtering == 0.02:
            assert 0 < len(m.representations) < len(unfiltered.representations)


def reverse_complement(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def genome_reads(genome, seed):
    rng = random.Random(seed)
    out = []
    for i in range(6):
        start = rng.randint(0, len(genome) - 500)
        r = genome[start:start + 500]
        out.append(reverse_complement(r) if i in (1, 4) else r)
    return out


@pytest.fixture(scope="module")
def matcher_reads():
    genome = random_read(random.Random(9), 2000)
    return genome_reads(genome, 10), genome_reads(genome, 11)


def anchors_array(tuples):
    return np.array(tuples, dtype=ANCHOR_DTYPE) if tuples else np.empty(0, ANCHOR_DTYPE)


@pytest.mark.parametrize("k,w,hashed", [(15, 5, True), (6, 3, False)])
def test_matcher_parity(matcher_reads, k, w, hashed):
    queries, targets = matcher_reads
    mq = model.Index(queries, k, w, hash_representations=hashed)
    mt = model.Index(targets, k, w, hash_representations=hashed)
    with Index(queries, k, w, hash_representations=hashed) as q, \
            Index(targets, k, w, hash_representations=hashed) as t:
        for (a, b), (ma, mb) in (((q, t), (mq, mt)), ((q, q), (mq, mq)), ((t, q), (mt, mq))):
            expected = anchors_array(model.match_anchors(ma, mb))
            got = match_anchors(a, b)
            assert len(expected) > 0
            assert got.tobytes() == expected.tobytes()


def test_matcher_sub_range_ids_are_global(matcher_reads):
    queries, targets = matcher_reads
    reads = queries + targets
    kw = dict(first_read_id=2, past_the_last_read_id=7)
    with Index(reads, 15, 5, **kw) as q, Index(reads, 15, 5, first_read_id=5) as t:
        expected = anchors_array(model.match_anchors(model.Index(reads, 15, 5, **kw),
                                                     model.Index(reads, 15, 5, first_read_id=5)))
        got = match_anchors(q, t)
        assert got.tobytes() == expected.tobytes()
        assert got["query_read_id"].min() == 2 and got["target_read_id"].max() == 11


def test_max_anchors_and_pool_accounting(matcher_reads):
    from claragenomicsanalysis_amd.cudaaligner import DeviceAllocator
    queries, targets = matcher_reads
    pool = DeviceAllocator(64 << 20)
    assert pool.used == 0
    with Index(queries, 15, 5, allocator=pool) as q:
        held = pool.used  # the six arrays of the index
        assert held == (8 + 4 + 4 + 1) * len(q.representations) + 8 * len(q.unique_representations) + \
            4 * len(q.first_occurrence_of_representations)
        with Index(targets, 15, 5) as t:
            n = len(match_anchors(q, t, allocator=pool))
            assert n > 1 and pool.used == held
            assert len(match_anchors(q, t, max_anchors=n, allocator=pool)) == n
            with pytest.raises(RuntimeError, match="max_anchors"):
                match_anchors(q, t, max_anchors=n - 1, allocator=pool)
            assert pool.used == held
            with pytest.raises(RuntimeError, match="max_anchors"):
                match_anchors(q, t, max_anchors=0)
    assert pool.used == 0
    # a pool too small for the index: an error, and nothing stays reserved
    small = DeviceAllocator(1024)
    with pytest.raises(RuntimeError, match="pool"):
        Index(queries, 15, 5, allocator=small)
    assert small.used == 0


def test_fasta_to_anchors_chain(tmp_path, matcher_reads):
    queries, _ = matcher_reads
    path = tmp_path / "reads.fasta"
    path.write_text("".join(">r%d\n%s\n" % (i, s) for i, s in enumerate(queries)))
    records = read_fasta(path, shuffle=False)
    with Index(records, 15, 5) as idx:
        assert_index_equal(idx, model.Index(queries, 15, 5))
        assert len(match_anchors(idx, idx)) >= len(idx.representations)


CPP_PROGRAM = r"""
#include <claraparabricks/genomeworks/cudamapper/index.hpp>
#include <claraparabricks/genomeworks/cudamapper/matcher.hpp>
#include <cstdio>
using namespace claragenomics;
int main(int argc, char** argv)
{
    auto parser    = io::create_kseq_fasta_parser(argv[1], 0, false);
    auto allocator = create_default_device_allocator();
    auto query     = cudamapper::Index::create_index(allocator, *parser, 0, 3, 15, 5);
    auto target    = cudamapper::Index::create_index(allocator, *parser, 2, parser->get_num_seqences(), 15, 5, true, 1.0);
    auto matcher   = cudamapper::Matcher::create_matcher(allocator, *query, *target);
    const device_buffer<cudamapper::representation_t>& r = query->representations();
    const device_buffer<cudamapper::SketchElement::DirectionOfRepresentation>& d = query->directions_of_reads();
    std::printf("%ld %ld %ld %ld %u %u %u %u %ld %d\n", long(r.size()), long(d.size()),
                long(target->unique_representations().size()),
                long(target->first_occurrence_of_representations().size()), target->number_of_reads(),
                target->smallest_read_id(), target->largest_read_id(), target->number_of_basepairs_in_longest_read(),
                long(matcher->anchors().size()), int(cudamapper::Index::maximum_kmer_size()));
    return matcher->anchors().data() != nullptr && allocator.budget()->used() > 0 ? 0 : 1;
}
"""


def test_cpp_surface(tmp_path, matcher_reads):
    queries, _ = matcher_reads
    fasta = tmp_path / "reads.fasta"
    fasta.write_text("".join(">r%d\n%s\n" % (i, s) for i, s in enumerate(queries)))
    src = tmp_path / "mapper_api.cpp"
    src.write_text(CPP_PROGRAM)
    exe = tmp_path / "mapper_api"
    lib = os.path.join(ROOT, "claragenomicsanalysis_amd", "lib")
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-std=c++17", "-O1",
                           "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
                           "-x", "c++", str(src), "-L", lib, "-lgwamd", "-Wl,-rpath," + lib, "-o", str(exe)])
    out = subprocess.check_output([str(exe), str(fasta)], timeout=120).decode().split()
    with Index(queries, 15, 5, 0, 3) as q, Index(queries, 15, 5, 2) as t:
        expected = [len(q.representations), len(q.directions_of_reads), len(t.unique_representations),
                    len(t.first_occurrence_of_representations), t.number_of_reads, t.smallest_read_id,
                    t.largest_read_id, t.number_of_basepairs_in_longest_read, len(match_anchors(q, t)), 32]
    assert [int(x) for x in out] == expected
    mq, mt = model.Index(queries, 15, 5, 0, 3), model.Index(queries, 15, 5, 2)
    assert expected[8] == len(model.match_anchors(mq, mt)) and expected[0] == len(mq.representations)
