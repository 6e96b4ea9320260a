"""Index descriptors and batches of indices (include/gwamd_cudamapper.h,
claragenomicsanalysis_amd.cudamapper): the C ABI, the plain-Python model
(tests/index_batcher_model.py) and the expected values of the reference's
gtests (tests/golden/index_batcher_kat.json) agree with one another.  Host
code only: no GPU."""
import json
import os
import random

import pytest

import index_batcher_model as model
from claragenomicsanalysis_amd import generate_batches_of_indices, group_reads_into_indices
from claragenomicsanalysis_amd.cudamapper import index_descriptor_hash, read_fasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
KAT = json.load(open(os.path.join(GOLDEN, "index_batcher_kat.json")))


def pairs(descriptors):
    return [tuple(d) for d in descriptors]


def normal(batches):
    return [{"query": pairs(b["query"]), "target": pairs(b["target"]),
             "device_batches": [{"query": pairs(d["query"]), "target": pairs(d["target"])}
                                for d in b["device_batches"]]} for b in batches]


@pytest.fixture(scope="module")
def reads():
    """The reads of the reference's two FASTA fixtures, as its tests load them."""
    out = {}
    for name, lengths in KAT["read_lengths"].items():
        records = read_fasta(os.path.join(GOLDEN, name), 1, shuffle=False)
        assert [len(s) for _, s in records] == lengths
        out[name] = records
    return out


# ---- descriptors ------------------------------------------------------------------------

def test_descriptor_hash_and_equality():
    d = KAT["descriptor"]
    h = d["hash"]
    assert index_descriptor_hash(h["first_read"], h["number_of_reads"]) == h["hash"] == 0xCF00000024
    assert model.descriptor_hash(h["first_read"], h["number_of_reads"]) == h["hash"]
    # equal descriptors hash alike, the reference's unequal ones do not
    for a, b in d["equal"]:
        assert index_descriptor_hash(*a) == index_descriptor_hash(*b)
    for a, b in d["not_equal"]:
        assert index_descriptor_hash(*a) != index_descriptor_hash(*b)
    assert index_descriptor_hash(0xFFFFFFFF, 0xFFFFFFFF) == 0xFFFFFFFFFFFFFFFF
    assert index_descriptor_hash(d["getters"]["first_read"], d["getters"]["number_of_reads"]) == 15 | 156 << 32


def test_group_reads_into_indices_known_answers(reads):
    for case in KAT["group_reads_into_indices"]:
        lengths = KAT["read_lengths"][case["file"]]
        want = pairs(case["expected"])
        assert model.group_reads_into_indices(lengths, case["max_basepairs_per_index"]) == want
        assert group_reads_into_indices(lengths, case["max_basepairs_per_index"]) == want
        assert group_reads_into_indices(reads[case["file"]], case["max_basepairs_per_index"]) == want


@pytest.mark.parametrize("lengths, limit, want", [
    ([12, 3, 4], 10, [(0, 0), (0, 1), (1, 2)]),         # read 0 over the limit: the reference's leading (0, 0)
    ([5], 10, [(0, 1)]),                                  # one read
    ([11], 10, [(0, 0), (0, 1)]),
    ([], 10, [(0, 0)]),                                   # no reads
    ([11, 12, 13], 10, [(0, 0), (0, 1), (1, 1), (2, 1)]),  # every read over the limit
    ([10, 10], 10, [(0, 1), (1, 1)]),                     # exactly the limit fits
    ([0, 0, 0], 0, [(0, 3)]),
    ([3, 4], 1000000, [(0, 2)]),
])
def test_group_reads_into_indices_edges(lengths, limit, want):
    assert model.group_reads_into_indices(lengths, limit) == want
    assert group_reads_into_indices(lengths, limit) == want
    assert group_reads_into_indices([b"A" * n for n in lengths], limit) == want


def test_group_reads_into_indices_default_limit():
    lengths = [400000, 400000, 400000, 1000001, 5]
    assert group_reads_into_indices(lengths) == model.group_reads_into_indices(lengths) == \
        [(0, 2), (2, 1), (3, 1), (4, 1)]


def test_group_reads_into_indices_refuses_bad_arguments():
    for lengths, limit in (([-1], 10), ([1 << 31], 10), ([1], -1), ([1], 1 << 32)):
        with pytest.raises(ValueError):
            group_reads_into_indices(lengths, limit)


# ---- batches ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(KAT["generate_batches_of_indices"]))
def test_generate_batches_known_answers(reads, name):
    case = KAT["generate_batches_of_indices"][name]
    p = case["params"]
    query = KAT["read_lengths"][case["query_file"]]
    target = query if p["same_query_and_target"] else KAT["read_lengths"][case["target_file"]]
    args = (p["query_indices_per_host_batch"], p["query_indices_per_device_batch"], p["target_indices_per_host_batch"],
            p["target_indices_per_device_batch"])
    tail = (p["query_basepairs_per_index"], p["target_basepairs_per_index"], p["same_query_and_target"])
    want = normal(case["batches"])
    assert len(want) in (6, 9)
    assert model.generate_batches_of_indices(*args, query, target, *tail) == want
    assert generate_batches_of_indices(*args, query, target, *tail) == want
    records = reads[case["query_file"]]
    other = records if p["same_query_and_target"] else reads[case["target_file"]]
    assert generate_batches_of_indices(*args, records, other, *tail) == want


def test_generate_batches_exceptions():
    e = KAT["exceptions"]
    assert len(e["cases"]) == 4
    query = KAT["read_lengths"][e["query_file"]]
    other = KAT["read_lengths"][e["other_file"]]
    host, device, basepairs = e["query_indices_per_host_batch"], e["query_indices_per_device_batch"], \
        e["query_basepairs_per_index"]
    good = (host, device, host, device, query, query, basepairs, basepairs, True)
    assert generate_batches_of_indices(*good) == model.generate_batches_of_indices(*good)
    for bad in ((host, device, 100, device, query, query, basepairs, basepairs, True),
                (host, device, host, 100, query, query, basepairs, basepairs, True),
                (host, device, host, device, query, other, basepairs, basepairs, True),
                (host, device, host, device, query, list(query), basepairs, basepairs, True),  # an equal copy is another parser
                (host, device, host, device, query, query, basepairs, 100, True)):
        with pytest.raises(ValueError):
            generate_batches_of_indices(*bad)
        with pytest.raises(ValueError):
            model.generate_batches_of_indices(*bad)
        # without same_query_and_target each of them is fine
        assert generate_batches_of_indices(*bad[:8], False) == model.generate_batches_of_indices(*bad[:8], False)
    for bad in ((0, device, 0, device), (host, 0, host, 0), (-1, device, -1, device)):
        with pytest.raises(ValueError):
            generate_batches_of_indices(*bad, query, query, basepairs, basepairs, True)
        with pytest.raises(ValueError):
            generate_batches_of_indices(*bad, query, other, basepairs, basepairs, False)


@pytest.mark.parametrize("per_host, per_device", [(1, 1), (1, 100), (100, 1), (100, 100), (3, 2), (2, 3)])
def test_counts_of_one_and_of_more_than_there_are_indices(per_host, per_device):
    lengths = KAT["read_lengths"]["20_reads.fasta"]
    n = len(model.group_reads_into_indices(lengths, 10))
    assert n == 11
    for same in (True, False):
        args = (per_host, per_device, per_host, per_device, lengths, lengths, 10, 10, same)
        got = generate_batches_of_indices(*args)
        assert got == model.generate_batches_of_indices(*args)
        sections = -(-n // per_host)
        assert len(got) == (sections * (sections + 1) // 2 if same else sections * sections)
        # every pair of indices is in exactly one device batch, or, in the triangle, it or its mirror is
        seen = [(q, t) for b in got for d in b["device_batches"] for q in d["query"] for t in d["target"]]
        assert len(seen) == len(set(seen))
        if same:
            index = model.group_reads_into_indices(lengths, 10)
            assert {tuple(sorted(p)) for p in seen} == {(a, b) for a in index for b in index if a <= b}
        else:
            assert len(seen) == n * n


def test_random_length_lists_against_the_model():
    rng = random.Random(20260)
    for trial in range(200):
        query = [rng.choice([0, 1, rng.randint(1, 30), rng.randint(1, 200)]) for _ in range(rng.randint(0, 40))]
        limit = rng.choice([0, 1, 10, 50, 100, 1000])
        assert group_reads_into_indices(query, limit) == model.group_reads_into_indices(query, limit)
        same = trial % 2 == 0
        target = query if same else [rng.randint(0, 120) for _ in range(rng.randint(0, 40))]
        per = [rng.randint(1, 6) for _ in range(4)]
        if same:
            per[2:] = per[:2]
        other_limit = limit if same else rng.choice([1, 10, 100])
        args = (per[0], per[1], per[2], per[3], query, target, limit, other_limit, same)
        assert generate_batches_of_indices(*args) == model.generate_batches_of_indices(*args)
