"""GPU checks of the overlap-end rescue (csrc/mapper_rescue.hip) against the
plain-Python model (tests/rescue_model.py, itself pinned by
test_rescue_model.py) and the reference's known answer
(tests/golden/rescue_kat.json).  The rescue is byte compares, integer counts
and one float32 division per end, so every field of every record is compared
exactly.  Every case is a handful of overlaps on short reads in one call."""
import json
import os
import random
import re
import subprocess

import numpy as np
import pytest

import mapper_model
import overlapper_model
import rescue_cases
import rescue_model as model
from claragenomicsanalysis_amd import (Index, match_overlaps, post_process_overlaps, rescue_overlap_ends)
from claragenomicsanalysis_amd.cudamapper import align_overlaps, format_paf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "rescue_kat.json")))
LENGTHS = [0, 1, 14, 15, 16, 29, 30, 31, 63, 64, 65, 99, 100]  # and 128 at extension 128
CORE = rescue_cases.random_bases(random.Random(5), 60)


def as_tuples(overlaps):
    return [(o.query_read_id, o.target_read_id, o.query_start, o.query_end, o.target_start, o.target_end, o.strand,
             o.num_residues, bool(o.overlap_complete)) for o in overlaps]


def check(overlaps, queries, targets, extension=100, similarity=0.9):
    """The GPU's rescue equals the model's in every field; returns it."""
    want = model.rescue_overlap_ends(overlaps, queries, targets, extension, similarity)
    got = as_tuples(rescue_overlap_ends(overlaps, queries, targets, extension, similarity))
    assert got == want
    return want


class Batch:
    """Overlaps on a query and a target read of their own, built from flanks
    around a shared core.  A Reverse overlap is given as the rounds see it and
    stored as the caller would: the target reverse complemented the reference's
    way (an involution) and the target positions mirrored."""

    def __init__(self):
        self.queries, self.targets, self.overlaps, self.labels = [], [], [], []

    def add(self, head_q, head_t, tail_q, tail_t, strand="+", core=CORE, label=None):
        query, target = head_q + core + tail_q, head_t + core + tail_t
        ts, te = len(head_t), len(head_t) + len(core)
        if strand == "-":
            target = model.reverse_complement(target)
            ts, te = len(target) - te, len(target) - ts
        i = len(self.overlaps)
        self.overlaps.append((i, i, len(head_q), len(head_q) + len(core), ts, te, strand, i % 7, i % 2 == 0))
        self.queries.append(query)
        self.targets.append(target)
        self.labels.append(label)

    def check(self, extension=100, similarity=0.9):
        return check(self.overlaps, self.queries, self.targets, extension, similarity)

    def gains(self, extension=100, similarity=0.9):
        """Per overlap, from the model: the bases gained at the head and at the tail."""
        out = []
        for o in self.overlaps:
            _, head, tail = model.rescue_one(o, self.queries[o[0]], self.targets[o[1]], extension, similarity)
            out.append((sum(head), sum(tail)))
        return out

    def gains_of(self, label, extension=100, similarity=0.9):
        return [g for g, l in zip(self.gains(extension, similarity), self.labels) if l == label]


def bases(rng, n):
    return rescue_cases.random_bases(rng, n)


# ---- the reference's known answer ---------------------------------------------------

def test_reference_fixture():
    case = GOLDEN["extension_case"]
    o, e = case["overlap"], case["expected"]
    overlap = (0, 0, o["query_start"], o["query_end"], o["target_start"], o["target_end"], o["strand"], 9, True)
    # three rounds give what the reference's one round gives: the windows left are empty
    got = check([overlap], [case["query"].encode()], [case["target"].encode()], case["extension"],
                case["required_similarity"])
    assert got == [(0, 0, e["query_start"], e["query_end"], e["target_start"], e["target_end"], "+", 9, True)]


# ---- window lengths -------------------------------------------------------------------

def variants(flank, rng, from_end):
    """The flank, and the flank with one substitution at the first, second, middle
    and last base of the window, which is the flank's last bases at a head
    (from_end) and its first bases at a tail."""
    n = len(flank)
    out = [flank]
    for at in sorted({0, 1, n // 2, n - 1}):
        if 0 <= at < n:
            out.append(rescue_cases.substitute(flank, n - 1 - at if from_end else at, rng))
    return out


@pytest.mark.parametrize("length", LENGTHS + [128])
def test_window_lengths(length):
    rng = random.Random(1000 + length)
    extension = 128 if length == 128 else 100
    room, by_extension = Batch(), Batch()
    for strand in "+-":
        # the window is the room to the read's end: on both reads, on the query alone, on the target alone
        for extra_q, extra_t in ((0, 0), (0, 7), (7, 0)):
            head, tail = bases(rng, length), bases(rng, length)
            for j, (h, t) in enumerate(zip(variants(head, rng, True), variants(tail, rng, False))):
                room.add(bases(rng, extra_q) + head, bases(rng, extra_t) + h, tail + bases(rng, extra_q),
                         t + bases(rng, extra_t), strand, label="changed" if j else "same")
        # the window is the extension, inside flanks of 150
        head, tail = bases(rng, 150), bases(rng, 150)
        pairs = zip(variants(head[150 - length:], rng, True), variants(tail[:length], rng, False))
        for j, (h, t) in enumerate(pairs):
            by_extension.add(head, head[:150 - length] + h, tail, t + tail[length:], strand,
                             label="changed" if j else "same")
    room.check(extension)
    assert room.gains_of("same", extension) == [(length, length)] * 6
    by_extension.check(length)
    reach = min(3 * length, 150)
    assert by_extension.gains_of("same", length) == [(reach, reach)] * 2
    if length >= 15:  # a substitution in the middle of a window is refused; shorter windows: any substitution
        assert (0, 0) in by_extension.gains_of("changed", length) and (0, 0) in room.gains_of("changed", extension)


# ---- the exact threshold ----------------------------------------------------------------

def test_exact_threshold():
    rng = random.Random(33)
    batch = Batch()
    for strand in "+-":
        flank = bases(rng, 33)
        first, second = rescue_cases.substitute(flank, 0, rng), rescue_cases.substitute(flank, 1, rng)
        assert model.shared_and_union(flank, first) == (18, 20) and model.shared_and_union(flank, second) == (17, 21)
        batch.add(flank, first, first, flank, strand)    # 18 / 20 == 0.9f: accepted
        batch.add(flank, second, second, flank, strand)  # 17 / 21: refused
    batch.check()
    assert batch.gains() == [(33, 33), (0, 0)] * 2
    # the threshold a little above 0.9f refuses both, a little below 17 / 21 accepts both
    above = float(np.nextafter(np.float32(0.9), np.float32(1)))
    below = float(np.nextafter(np.float32(17) / np.float32(21), np.float32(0)))
    batch.check(similarity=above)
    batch.check(similarity=float(np.float32(17) / np.float32(21)))
    batch.check(similarity=below)
    assert batch.gains(similarity=above) == [(0, 0)] * 4 and batch.gains(similarity=below) == [(33, 33)] * 4
    # thresholds nothing and everything passes
    batch.check(similarity=1.5)
    batch.check(similarity=0.0)
    batch.check(similarity=-1.0)


# ---- duplicate substrings ------------------------------------------------------------------

@pytest.mark.parametrize("unit", [b"A", b"AC", b"ACGTT"], ids=["homopolymer", "dinucleotide", "period5"])
def test_repeats(unit):
    rng = random.Random(len(unit))
    batch = Batch()
    for length in (15, 16, 17, 29, 30, 31, 45, 64, 65, 100):
        flank = (unit * length)[:length]
        shifted = (unit * length)[1:length + 1]
        other = (bytes(reversed(unit)) * length)[:length]
        for strand in "+-":
            batch.add(flank, flank, flank, flank, strand)
            batch.add(flank, shifted, shifted, flank, strand)
            batch.add(flank, other, flank, rescue_cases.substitute(flank, length // 3, rng), strand)
            batch.add(flank, flank[:length // 2] + bases(rng, length - length // 2), bases(rng, 7) + flank[7:],
                      flank, strand)
    for similarity in (0.9, 0.5, 0.2):
        batch.check(similarity=similarity)
    gains = batch.gains(similarity=0.5)
    assert any(g[0] for g in gains) and any(not g[0] for g in gains)


# ---- Reverse overlaps and the middle base ----------------------------------------------------

@pytest.mark.parametrize("base", "ACGT")
def test_middle_base_of_an_odd_target_flips_the_decision(base):
    """The targets are true reverse complements.  On a target of odd length the
    reference leaves the middle base uncomplemented; with that base second in a
    33-base window the window has 17 of 19 substrings left and is refused, while
    the even target next to it, one base longer at its far end, is accepted."""
    rng = random.Random(ord(base))
    flank = base.encode() * 2 + bases(rng, 31)
    flank = flank[:1] + base.encode() + flank[2:]
    # the rounds see tail windows query[60:93] and rc(target)[60:93]; base 61 is the middle of 123
    query = CORE + flank
    odd = rescue_cases.plain_reverse_complement(CORE + flank + bases(rng, 30))
    even = rescue_cases.plain_reverse_complement(CORE + flank + bases(rng, 31))
    assert len(odd) == 123 and len(odd) // 2 == 61 and len(even) == 124
    overlaps = [(0, 0, 0, 60, len(odd) - 60, len(odd), "-", 1, True),
                (0, 1, 0, 60, len(even) - 60, len(even), "-", 2, False)]
    got = check(overlaps, [query], [odd, even])
    assert got[0] == overlaps[0]
    assert got[1] == (0, 1, 0, 93, len(even) - 93, len(even), "-", 2, False)
    # the middle base in the head window of the mirrored layout
    query = flank + CORE
    odd = rescue_cases.plain_reverse_complement(bases(rng, 30) + flank + CORE)
    even = rescue_cases.plain_reverse_complement(bases(rng, 31) + flank + CORE)
    overlaps = [(0, 0, 33, 93, 0, 60, "-", 1, True), (0, 1, 33, 93, 0, 60, "-", 2, False)]
    got = check(overlaps, [query], [odd, even])
    # window base 31 of 33 is the middle here: the last but one
    assert got[1] == (0, 1, 0, 93, 0, 93, "-", 2, False)


def test_reverse_on_even_and_odd_targets():
    rng = random.Random(77)
    batch = Batch()
    for pad in range(8):  # target lengths of both parities, the middle base inside and outside the windows
        head, tail = bases(rng, 40 + pad), bases(rng, 35)
        batch.add(head, head, tail, tail, "-")
        batch.add(head, bases(rng, pad) + head, tail, tail + bases(rng, 2 * pad + 1), "-")
        batch.add(head, head, tail, tail, "-", core=bases(rng, 3 + pad))
    batch.check()
    gains = batch.gains()
    assert any(g == (0, 0) for g in gains) or any(g[0] and g[1] for g in gains)


# ---- bytes that are not A, C, G or T ----------------------------------------------------------

def test_other_bytes_inside_windows():
    rng = random.Random(4)
    batch = Batch()
    specials = [b"N", b"NNNN", b"RYKMSWBDHV", b"acgtn", b"\x80", b"\xff\xfe", b"\x00", b"@[", b"aAcCgGtT"]
    for strand in "+-":
        for special in specials:
            for length in (20, 64, 100):
                flank = bytearray(bases(rng, length))
                at = rng.randint(0, length - len(special))
                flank[at:at + len(special)] = special
                flank = bytes(flank)
                batch.add(flank, flank, flank, flank, strand)  # equal on both reads, whatever the byte
                batch.add(flank, flank.upper(), flank.swapcase(), flank, strand)
                batch.add(flank, flank.replace(special, bases(rng, len(special))), flank, flank, strand)
    batch.check()
    gains = batch.gains()
    assert all(g[0] > 0 and g[1] > 0 for g in gains[::3])
    assert any(g[0] == 0 for g in gains)
    # true reverse complements: a lower-case base is not complemented, so it no longer matches
    query = b"acgtacgtacgtacgtacgtacgt" + CORE + bases(rng, 24)
    targets = [rescue_cases.plain_reverse_complement(query.upper()),
               rescue_cases.plain_reverse_complement(query.upper())[:-24] + b"acgtacgtacgtacgtacgtacgt"[::-1]]
    n = len(query)
    overlaps = [(0, 0, 24, 84, n - 84, n - 24, "-", 0, True), (0, 1, 24, 84, n - 84, n - 24, "-", 0, True)]
    got = check(overlaps, [query], targets)
    assert got[0][2] == 24 and got[0][3] == n and got[1][2] == 0


# ---- rounds --------------------------------------------------------------------------------------

def test_rounds():
    rng = random.Random(8)
    batch = Batch()
    for strand in "+-":
        long_head, long_tail = bases(rng, 350), bases(rng, 350)
        batch.add(long_head, long_head, long_tail, long_tail, strand)  # 300 per end
        head, tail = bases(rng, 150), bases(rng, 130)
        batch.add(head, head, tail, tail, strand)  # the read's end in round 2: 100 + 50 and 100 + 30
        batch.add(bases(rng, 60) + head, head, tail, tail + bases(rng, 60), strand)  # one read's end
        far = rescue_cases.substitute(long_head, 350 - 150, rng)
        batch.add(long_head, far, long_tail, rescue_cases.substitute(long_tail, 249, rng), strand)  # refused in 2, in 3
        near = rescue_cases.substitute(long_head, 350 - 50, rng)
        batch.add(long_head, near, long_tail, long_tail, strand)  # head refused, tail accepted
        batch.add(long_head, long_head, long_tail, rescue_cases.substitute(long_tail, 50, rng), strand)
        batch.add(bases(rng, 200), bases(rng, 200), bases(rng, 200), bases(rng, 200), strand)  # neither
    batch.check()
    assert batch.gains() == [(300, 300), (150, 130), (150, 130), (100, 200), (0, 300), (300, 0), (0, 0)] * 2
    for extension, expected in ((128, (350, 350)), (50, (150, 150)), (1, (3, 3)), (0, (0, 0))):
        batch.check(extension)
        assert batch.gains(extension)[0] == expected


# ---- counts, read ids, the single-upload path ----------------------------------------------------------

@pytest.fixture(scope="module")
def many():
    """1,027 overlaps of the random recipe with the reads of both sides in one
    shuffled list: mixed strands and read ids."""
    queries, targets, overlaps = rescue_cases.random_set(seed=7, count=1027)
    rng = random.Random(70)
    order = list(range(2 * len(overlaps)))
    rng.shuffle(order)
    reads = [None] * len(order)
    for i, (query, target) in enumerate(zip(queries, targets)):
        reads[order[2 * i]], reads[order[2 * i + 1]] = query, target
    overlaps = [(order[2 * i], order[2 * i + 1]) + o[2:] for i, o in enumerate(overlaps)]
    rng.shuffle(overlaps)
    return reads, overlaps, model.rescue_overlap_ends(overlaps, reads, reads)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027])
def test_counts(many, n):
    reads, overlaps, want = many
    assert as_tuples(rescue_overlap_ends(overlaps[:n], reads, reads)) == want[:n]  # one object: uploaded once
    assert as_tuples(rescue_overlap_ends(overlaps[:n], reads, list(reads))) == want[:n]  # two copies
    assert want[:n] != overlaps[:n] or n == 1


def test_random_set():
    queries, targets, overlaps = rescue_cases.random_set()
    check(overlaps, queries, targets)


# ---- pool accounting ---------------------------------------------------------------------------------------

def test_pool_accounting(many):
    from claragenomicsanalysis_amd.cudaaligner import DeviceAllocator
    reads, overlaps, want = many
    pool = DeviceAllocator(64 << 20)
    held = DeviceAllocator(1 << 20)  # another pool is not touched
    assert pool.used == 0
    assert as_tuples(rescue_overlap_ends(overlaps[:50], reads, reads, allocator=pool)) == want[:50]
    assert pool.used == 0 and held.used == 0
    assert as_tuples(rescue_overlap_ends(overlaps[:50], reads, list(reads), allocator=pool)) == want[:50]
    assert pool.used == 0
    with pytest.raises(ValueError):
        rescue_overlap_ends(overlaps[:50], reads, reads, extension=129, allocator=pool)
    with pytest.raises(ValueError):
        rescue_overlap_ends([(len(reads), 0, 0, 0, 0, 0, "+", 0, True)], reads, reads, allocator=pool)
    assert pool.used == 0
    total = sum(len(r) for r in reads)
    for capacity in (1024, total - 1, total + 1024):  # not the bases; the bases but not the rest
        small = DeviceAllocator(capacity)
        with pytest.raises(RuntimeError, match="pool"):
            rescue_overlap_ends(overlaps[:50], reads, reads, allocator=small)
        assert small.used == 0
    assert as_tuples(rescue_overlap_ends(overlaps[:50], reads, reads, allocator=pool)) == want[:50]


# ---- end to end ------------------------------------------------------------------------------------------------

def test_index_to_paf():
    rng = random.Random(12)
    genome = rescue_cases.random_bases(rng, 9000)
    reads = []
    for i in range(12):
        start = rng.randint(0, len(genome) - 3000)
        read = genome[start:start + 3000]
        reads.append(rescue_cases.plain_reverse_complement(read) if i % 3 == 1 else read)
    queries, targets = reads[:6], reads[6:]
    k = 15
    with Index(queries, k, 5) as q, Index(targets, k, 5) as t:
        overlaps = match_overlaps(q, t)
    mq, mt = mapper_model.Index(queries, k, 5), mapper_model.Index(targets, k, 5)
    assert as_tuples(overlaps) == overlapper_model.get_overlaps(mapper_model.match_anchors(mq, mt))[0]
    processed = as_tuples(post_process_overlaps(overlaps))
    assert len(processed) > 3 and {o[6] for o in processed} == {"+", "-"}
    rescued = rescue_overlap_ends(processed, queries, targets)
    want = model.rescue_overlap_ends(processed, queries, targets)
    assert as_tuples(rescued) == want
    assert sum(1 for a, b in zip(want, processed) if a != b) > 3  # the overlapper leaves ends to rescue
    for a, b in zip(want, processed):
        assert a[2] <= b[2] and a[3] >= b[3] and a[4] <= b[4] and a[5] >= b[5]
    cigars = align_overlaps(rescued, queries, targets)
    assert len(cigars) == len(rescued)
    for o, cigar in zip(rescued, cigars):
        ops = [(int(n), op) for n, op in re.findall(r"(\d+)([MIDX=])", cigar)]
        assert "".join("%d%s" % x for x in ops) == cigar and ops
        # I is present in the target only, D in the query only (cudaaligner.hpp)
        assert sum(n for n, op in ops if op != "I") == o.query_end - o.query_start
        assert sum(n for n, op in ops if op != "D") == o.target_end - o.target_start
    qrecords = [("q%d" % i, s.decode()) for i, s in enumerate(queries)]
    trecords = [("t%d" % i, s.decode()) for i, s in enumerate(targets)]
    lines = format_paf(rescued, cigars, qrecords, trecords, k).splitlines()
    assert len(lines) == len(rescued)
    for o, text in zip(rescued, lines):
        cols = text.split("\t")
        assert cols[0] == "q%d" % o.query_read_id and cols[5] == "t%d" % o.target_read_id and cols[4] == o.strand
        assert (int(cols[2]), int(cols[3])) == (o.query_start, o.query_end)


# ---- C++ surface ---------------------------------------------------------------------------------------------------

CPP_PROGRAM = r"""
#include <claraparabricks/genomeworks/cudamapper/overlapper.hpp>
#include <cstdio>
#include <fstream>
#include <string>
using namespace claragenomics;
using namespace claragenomics::cudamapper;
static void print(const char* tag, const std::vector<Overlap>& overlaps)
{
    for (const Overlap& o : overlaps)
        std::printf("%s %u %u %u %u %u %u %c %u %d\n", tag, o.query_read_id_, o.target_read_id_,
                    o.query_start_position_in_read_, o.query_end_position_in_read_,
                    o.target_start_position_in_read_, o.target_end_position_in_read_, char(o.relative_strand),
                    o.num_residues_, int(o.overlap_complete));
}
int main(int argc, char** argv)
{
    auto query_parser  = io::create_kseq_fasta_parser(argv[1], 0, false);
    auto target_parser = io::create_kseq_fasta_parser(argv[2], 0, false);
    std::vector<Overlap> overlaps;
    std::ifstream in(argv[3]);
    Overlap o;
    char strand;
    int complete;
    while (in >> o.query_read_id_ >> o.target_read_id_ >> o.query_start_position_in_read_ >>
           o.query_end_position_in_read_ >> o.target_start_position_in_read_ >> o.target_end_position_in_read_ >>
           strand >> o.num_residues_ >> complete)
    {
        o.relative_strand  = strand == '-' ? RelativeStrand::Reverse : RelativeStrand::Forward;
        o.overlap_complete = complete != 0;
        overlaps.push_back(o);
    }
    std::vector<Overlap> a = overlaps, b = overlaps, empty;
    Overlapper::rescue_overlap_ends(a, *query_parser, *target_parser, 50, 0.5f);
    print("main", a);
    claraparabricks::genomeworks::cudamapper::Overlapper::rescue_overlap_ends(b, *query_parser, *target_parser, 100,
                                                                            0.9f);
    print("default", b);
    Overlapper::rescue_overlap_ends(empty, *query_parser, *target_parser, 100, 0.9f);
    std::printf("empty %zu\n", empty.size());
    Overlap one = overlaps[0];
    gw_string_view_t query(query_parser->get_sequence_by_id(one.query_read_id_).seq);
    gw_string_view_t target(target_parser->get_sequence_by_id(one.target_read_id_).seq);
    details::overlapper::extend_overlap_by_sequence_similarity(one, query, target, 50, 0.5f);
    print("round", {one});
    try
    {
        overlaps[0].query_read_id_ = 1000;
        Overlapper::rescue_overlap_ends(overlaps, *query_parser, *target_parser, 100, 0.9f);
    }
    catch (const std::invalid_argument& e)
    {
        std::printf("refused %s\n", e.what());
    }
    return 0;
}
"""


def test_cpp_surface(tmp_path):
    queries, targets, overlaps = rescue_cases.random_set(seed=3, count=40)
    overlaps = [o for o in overlaps if o[6] == "+"][:1] + overlaps
    qpath, tpath, opath = tmp_path / "queries.fasta", tmp_path / "targets.fasta", tmp_path / "overlaps.txt"
    qpath.write_text("".join(">q%d\n%s\n" % (i, s.decode()) for i, s in enumerate(queries)))
    tpath.write_text("".join(">t%d\n%s\n" % (i, s.decode()) for i, s in enumerate(targets)))
    opath.write_text("".join("%d %d %d %d %d %d %s %d %d\n" % o for o in overlaps))
    src = tmp_path / "rescue_api.cpp"
    src.write_text(CPP_PROGRAM)
    exe = tmp_path / "rescue_api"
    lib = os.path.join(ROOT, "claragenomicsanalysis_amd", "lib")
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-std=c++17", "-O1",
                           "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
                           "-x", "c++", str(src), "-L", lib, "-lgwamd", "-Wl,-rpath," + lib, "-o", str(exe)])
    out = subprocess.check_output([str(exe), str(qpath), str(tpath), str(opath)], timeout=120).decode().splitlines()
    printed = {}
    for text in out:
        tag, *f = text.split()
        if tag in ("empty", "refused"):
            printed[tag] = f
            continue
        printed.setdefault(tag, []).append((int(f[0]), int(f[1]), int(f[2]), int(f[3]), int(f[4]), int(f[5]), f[6],
                                            int(f[7]), bool(int(f[8]))))
    # the two numbers are ignored: every round runs with 100 and 0.9f
    want = model.rescue_overlap_ends(overlaps, queries, targets, 100, 0.9)
    assert printed["main"] == printed["default"] == want
    assert model.rescue_overlap_ends(overlaps, queries, targets, 50, 0.5) != want
    assert printed["empty"] == ["0"] and "refused" in printed
    o = overlaps[0]
    assert printed["round"] == [model.extend_overlap_by_sequence_similarity(o, queries[o[0]], targets[o[1]], 50, 0.5)]
    assert as_tuples(rescue_overlap_ends(overlaps, queries, targets)) == want
