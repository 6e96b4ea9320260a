"""GPU checks of the overlapper (csrc/mapper_overlap.hip) against the
plain-Python model (tests/overlapper_model.py, itself pinned by
test_overlapper_model.py) and the reference's known answers
(tests/golden/overlapper_kat.json).  Everything is integer arithmetic and two
float32 divisions, so every record is compared exactly, field by field."""
import json
import os
import random
import re
import subprocess

import numpy as np
import pytest

import mapper_model
import overlapper_model as model
from claragenomicsanalysis_amd import Index, get_overlaps, match_anchors, match_overlaps, post_process_overlaps
from claragenomicsanalysis_amd.cudamapper import ANCHOR_DTYPE, align_overlaps, format_paf, read_fasta

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "overlapper_kat.json")))
TILE = 2048  # anchors per workgroup of the chain-flag kernel (kOverlapTile, mapper_common.hpp)
BLOCK = 256  # chains, kept chains and groups per workgroup of levels 2 and 3 (kThreads, mapper_prims.hpp)
DEFAULT = (20, 50, 50, 0.9)
LOOSE = (3, 0, 1000, 0.0)
EVERYTHING = (0, 0, 1 << 40, 0.0)  # every group with a span on both reads


def as_tuples(overlaps):
    return [(o.query_read_id, o.target_read_id, o.query_start, o.query_end, o.target_start, o.target_end, o.strand,
             o.num_residues, bool(o.overlap_complete)) for o in overlaps]


def as_array(anchors):
    return np.array([tuple(a) for a in anchors], dtype=ANCHOR_DTYPE) if len(anchors) else np.empty(0, ANCHOR_DTYPE)


def check(anchors, params=DEFAULT):
    """The GPU's overlaps of the anchors equal the model's; returns them and the model's counts."""
    expected, counts = model.get_overlaps([tuple(a) for a in anchors], *params)
    got = as_tuples(get_overlaps(as_array(anchors), *params))
    assert got == expected
    return expected, counts


# ---- golden cases ------------------------------------------------------------

@pytest.mark.parametrize("case", GOLDEN["anchor_cases"], ids=lambda c: c["name"])
def test_golden_anchor_cases(case):
    params = (case["min_residues"], case["min_overlap_len"], case["min_bases_per_residue"],
              case["min_overlap_fraction"])
    got, _ = check(case["anchors"], params)
    assert len(got) == case["expected_size"]
    fields = GOLDEN["overlap_fields"]
    for o, want in zip(got, case["expected_fields"]):
        have = dict(zip(fields, o))
        for name, value in want.items():
            if name == "target_end_greater_than_target_start":
                assert have["target_end"] > have["target_start"]
            else:
                assert have[name] == value, name


def test_golden_case_from_tuples_and_defaults():
    case = GOLDEN["anchor_cases"][1]
    got = get_overlaps([tuple(a) for a in case["anchors"]], 0, 0, 1000)  # the fraction defaults to 0.9f
    assert as_tuples(got) == model.get_overlaps(case["anchors"], 0, 0, 1000)[0] and len(got) == 1


# ---- anchors of the matcher --------------------------------------------------

def random_read(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


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
    """The recipe of test_mapper_gpu.py: 6 + 6 reads of 500 from a 2,000-base genome."""
    genome = random_read(random.Random(9), 2000)
    return genome_reads(genome, 10), genome_reads(genome, 11)


@pytest.mark.parametrize("k,w,hashed", [(15, 5, True), (6, 3, False)])
def test_matcher_anchors(matcher_reads, k, w, hashed):
    queries, targets = matcher_reads
    strands = set()
    with Index(queries, k, w, hash_representations=hashed) as q, \
            Index(targets, k, w, hash_representations=hashed) as t:
        for a, b in ((q, t), (q, q)):
            anchors = match_anchors(a, b)
            for params in (DEFAULT, LOOSE):
                expected, counts = check(anchors.tolist(), params)
                assert all(v > 0 for v in counts.values()), counts
                if (k, w) == (6, 3):
                    assert counts["groups"] < counts["kept"] < counts["chains"], counts
                strands |= {o[6] for o in expected}
                # the same, with the anchors staying on the device
                got, num_anchors = match_overlaps(a, b, *params, return_num_anchors=True)
                assert as_tuples(got) == expected and num_anchors == len(anchors)
    assert strands == {"+", "-"}


# ---- seams, on hand-made anchors ----------------------------------------------

def make_chains(chains):
    """Anchors of chains given as (length, link): within a chain both positions
    rise by one; 'fuse' starts the next chain 200 further on both reads (a new
    chain whose first anchor fuses with the first anchor of the one before),
    'split' 200 further on the query and 600 on the target (a new group) and
    'pair' on the next target read."""
    out, t, qp, tp = [], 1, 0, 0
    for i, (length, link) in enumerate(chains):
        if i:
            if link == "pair":
                t, qp, tp = t + 1, 0, 0
            else:
                qp, tp = qp + 200, tp + (200 if link == "fuse" else 600)
        for j in range(length):
            if j:
                qp, tp = qp + 1, tp + 1
            out.append((0, t, qp, tp))
    return out


@pytest.mark.parametrize("n", [TILE - 1, TILE, TILE + 1, 3 * TILE + 37])
def test_one_chain_over_the_tiles(n):
    expected, counts = check(make_chains([(n, "pair")]), EVERYTHING)
    assert counts == dict(chains=1, kept=1, groups=1, overlaps=1)
    assert expected == [(0, 1, 0, n - 1, 0, n - 1, "+", n, True)]


def test_chain_heads_on_wave_and_tile_boundaries():
    # heads at 0, 64, 128, 512, TILE, TILE + 64, 2 * TILE and 3 * TILE
    lengths = [64, 64, 384, TILE - 512, 64, TILE - 64, TILE, 5]
    links = ["pair", "split", "fuse", "pair", "split", "fuse", "split", "pair"]
    anchors = make_chains(list(zip(lengths, links)))
    heads = [i for i in range(len(anchors)) if i == 0 or not model.same_chain(anchors[i - 1], anchors[i])]
    assert heads == [0, 64, 128, 512, TILE, TILE + 64, 2 * TILE, 3 * TILE]
    expected, counts = check(anchors, EVERYTHING)
    assert counts == dict(chains=8, kept=8, groups=6, overlaps=6)


@pytest.mark.parametrize("before,length,kept", [(TILE - 1, 3, True), (TILE - 2, 3, True), (TILE - 1, 2, False),
                                                (2 * TILE - 1, 3, True), (2 * TILE - 2, 3, True)])
def test_short_chain_across_a_tile_boundary(before, length, kept):
    expected, counts = check(make_chains([(before, "pair"), (length, "pair"), (5, "pair")]), EVERYTHING)
    assert counts == dict(chains=3, kept=2 + kept, groups=2 + kept, overlaps=2 + kept)
    assert ((0, 2, 0, length - 1, 0, length - 1, "+", length, True) in expected) == kept


def test_many_short_chains_and_groups_across_blocks():
    # 5,001 chains of three anchors: more chains than a tile has anchors, and
    # groups of three and four chains across the workgroups of levels 2 and 3
    rng = random.Random(3)
    chains, left = [], 0
    while len(chains) < 5001:
        if left == 0:
            left = rng.choice([3, 3, 4, 1])
            chains.append((3, rng.choice(["split", "pair"])))
        else:
            chains.append((3, "fuse"))
        left -= 1
    anchors = make_chains(chains)
    assert len(anchors) > 7 * TILE and len(chains) > TILE
    expected, counts = check(anchors, EVERYTHING)
    assert counts["chains"] == counts["kept"] == 5001 and counts["groups"] > 4 * BLOCK
    assert counts["overlaps"] == counts["groups"]
    # groups that hold the chains 255..256, 511..512, ... of level 2 and 3
    firsts = [i for i, c in enumerate(chains) if c[1] != "fuse"]
    crossing = [b for b in range(BLOCK, 5001, BLOCK) if b not in firsts]
    assert len(crossing) > 10
    assert {o[7] for o in expected} == {3, 9, 12}
    # with short chains dropped in between, on the same seams
    mixed = [(length if i % 7 else 2, link) for i, (length, link) in enumerate(chains)]
    expected, counts = check(make_chains(mixed), EVERYTHING)
    assert counts["kept"] < counts["chains"] and counts["groups"] > 4 * BLOCK


def test_group_spans_a_dropped_chain():
    anchors = make_chains([(4, "pair"), (2, "fuse"), (5, "fuse"), (3, "pair")])
    expected, counts = check(anchors, EVERYTHING)
    assert counts == dict(chains=4, kept=3, groups=2, overlaps=2)
    end = anchors[10]  # the last anchor of the third chain, beyond the dropped one
    assert expected[0] == (0, 1, 0, end[2], 0, end[3], "+", 9, True)


# ---- random sorted anchors ----------------------------------------------------

def random_anchors(rng, n, p_jump, p_down, p_dup):
    out = []
    while len(out) < n:
        q, t = rng.randint(0, 3), rng.randint(0, 3)
        qp, tp = rng.randint(0, 2000), rng.randint(50000, 60000)
        down = rng.random() < p_down
        for _ in range(rng.randint(1, 400)):
            out.append((q, t, qp, tp))
            if rng.random() < p_dup:
                continue
            dq = rng.choice([149, 150, 151, rng.randint(150, 600)]) if rng.random() < p_jump else rng.randint(0, 40)
            dt = rng.choice([149, 150, 151, rng.randint(150, 600)]) if rng.random() < p_jump else rng.randint(0, 40)
            qp, tp = qp + dq, max(0, tp - dt if down else tp + dt)
    return sorted(out[:n])


@pytest.mark.parametrize("seed", range(20))
def test_random_sorted_anchors(seed):
    rng = random.Random(1000 + seed)
    n = rng.choice([rng.randint(1, 300), rng.randint(TILE - 70, TILE + 70), rng.randint(3000, 10000)])
    anchors = random_anchors(rng, n, rng.choice([0.02, 0.1, 0.3]), rng.choice([0.0, 0.3, 1.0]),
                             rng.choice([0.0, 0.05, 0.5]))
    for params in (LOOSE, rng.choice([DEFAULT, (0, 0, 50, 0.5), (5, 100, 20, 0.8), EVERYTHING])):
        check(anchors, params)


def test_random_anchors_are_not_vacuous():
    rng = random.Random(77)
    _, counts = model.get_overlaps(random_anchors(rng, 8000, 0.1, 0.3, 0.05), *LOOSE)
    assert 0 < counts["overlaps"] < counts["groups"] < counts["kept"] < counts["chains"]


# ---- filter -------------------------------------------------------------------

def line(q, t, query_positions, target_positions):
    return [(q, t, a, b) for a, b in zip(query_positions, target_positions)]


@pytest.mark.parametrize("num,den,fraction,below", [(9, 10, 0.9, 0.89), (90, 100, 0.9, 0.89), (900, 1000, 0.9, 0.89),
                                                    (1, 2, 0.5, 0.49)])
def test_fraction_is_an_exact_float32_quotient(num, den, fraction, below):
    steps = max(2, den // 100)
    qs = [den * i // steps for i in range(steps + 1)]
    ts = [num * i // steps for i in range(steps + 1)]
    # target span num of query span den and the other way round: equal to the fraction, rejected
    for anchors in (line(0, 1, qs, ts), line(0, 1, ts, qs) if num > 1 else line(0, 1, [0, 0, 1], [0, 1, 2])):
        assert check(anchors, (0, 0, 1 << 40, fraction))[0] == []
        assert len(check(anchors, (0, 0, 1 << 40, below))[0]) == 1


def test_filter_edges():
    same = [(0, 1, 100, 100)] * 3
    assert check(same, (0, 0, 1000, 0.0))[0] == []  # 0 / 0
    assert check(line(5, 5, [0, 10, 20], [0, 10, 20]), EVERYTHING)[0] == []  # a read with itself
    assert len(check(line(5, 6, [0, 10, 20], [0, 10, 20]), EVERYTHING)[0]) == 1
    # query span 49 and 50 at min_overlap_len 50; the same for the target span
    assert check(line(0, 1, [0, 25, 49], [0, 25, 50]), (0, 50, 1000, 0.0))[0] == []
    assert check(line(0, 1, [0, 25, 50], [0, 25, 49]), (0, 50, 1000, 0.0))[0] == []
    assert len(check(line(0, 1, [0, 25, 50], [0, 25, 50]), (0, 50, 1000, 0.0))[0]) == 1
    # 149 / 3 = 49 and 150 / 3 = 50 bases per residue at min_bases_per_residue 50
    assert len(check(line(0, 1, [0, 70, 149], [0, 70, 149]), (0, 0, 50, 0.0))[0]) == 1
    assert check(line(0, 1, [0, 75, 150], [0, 75, 150]), (0, 0, 50, 0.0))[0] == []
    # min_residues at and above the chain's length
    assert len(check(line(0, 1, [0, 10, 20], [0, 10, 20]), (3, 0, 1000, 0.0))[0]) == 1
    assert check(line(0, 1, [0, 10, 20], [0, 10, 20]), (4, 0, 1000, 0.0))[0] == []
    # falling target positions: Reverse, start and end swapped
    assert check(line(0, 1, [0, 10, 20], [90, 80, 70]), EVERYTHING)[0] == [(0, 1, 0, 20, 70, 90, "-", 3, True)]


@pytest.mark.parametrize("n", [0, 1, 2])
def test_too_few_anchors(n):
    assert check([(0, 1, 10 * i, 10 * i) for i in range(n)], EVERYTHING)[0] == []


# ---- bad input ------------------------------------------------------------------

@pytest.mark.parametrize("at", [1, 5, 63, 64, 512, TILE, 2 * TILE + 9])
def test_unsorted_pair_is_refused(at):
    anchors = make_chains([(2 * TILE + 10, "pair")])
    q, t, qp, tp = anchors[at - 1]
    anchors[at - 1] = (q, t, qp + 5, tp) if at % 2 else (q, t + 1, qp, tp)  # above the anchor after it alone
    with pytest.raises(ValueError, match="sorted"):
        get_overlaps(as_array(anchors), *EVERYTHING)
    with pytest.raises(ValueError):
        model.get_overlaps(anchors, *EVERYTHING)


@pytest.mark.parametrize("field", [2, 3])
def test_position_of_two_to_the_31_is_refused(field):
    anchors = make_chains([(TILE + 5, "pair")])
    last = list(anchors[-1])
    last[field] = 1 << 31
    with pytest.raises(ValueError, match="2\\^31"):
        get_overlaps(as_array(anchors[:-1] + [tuple(last)]), *EVERYTHING)
    last[field] = (1 << 31) - 1
    check(anchors[:-1] + [tuple(last)], EVERYTHING)


# ---- pool accounting --------------------------------------------------------------

def test_pool_accounting(matcher_reads):
    from claragenomicsanalysis_amd.cudaaligner import DeviceAllocator
    queries, targets = matcher_reads
    pool = DeviceAllocator(64 << 20)
    with Index(queries, 15, 5, allocator=pool) as q:
        held = pool.used
        assert held > 0
        with Index(targets, 15, 5) as t:
            anchors = match_anchors(q, t)
            expected = model.get_overlaps(anchors.tolist(), *LOOSE)[0]
            assert as_tuples(get_overlaps(anchors, *LOOSE, allocator=pool)) == expected and pool.used == held
            assert as_tuples(match_overlaps(q, t, *LOOSE, allocator=pool)) == expected and pool.used == held
            assert as_tuples(match_overlaps(q, t, *LOOSE, max_anchors=len(anchors), allocator=pool)) == expected
            with pytest.raises(RuntimeError, match="max_anchors"):
                match_overlaps(q, t, *LOOSE, max_anchors=len(anchors) - 1, allocator=pool)
            assert pool.used == held
            small = DeviceAllocator(16 * len(anchors) + 64)  # the anchors fit, the overlapper's arrays do not
            with pytest.raises(RuntimeError, match="pool"):
                get_overlaps(anchors, *LOOSE, allocator=small)
            assert small.used == 0
            with pytest.raises(RuntimeError, match="pool"):
                match_overlaps(q, t, *LOOSE, allocator=small)
            assert small.used == 0
    assert pool.used == 0


# ---- end to end -------------------------------------------------------------------

def test_fasta_to_paf(tmp_path, matcher_reads):
    queries, targets = matcher_reads
    qpath, tpath = tmp_path / "queries.fasta", tmp_path / "targets.fasta"
    qpath.write_text("".join(">q%d\n%s\n" % (i, s) for i, s in enumerate(queries)))
    tpath.write_text("".join(">t%d\n%s\n" % (i, s) for i, s in enumerate(targets)))
    qrecords, trecords = read_fasta(qpath, shuffle=False), read_fasta(tpath, shuffle=False)
    k = 15
    with Index(qrecords, k, 5) as q, Index(trecords, k, 5) as t:
        overlaps = match_overlaps(q, t)
    mq, mt = mapper_model.Index(queries, k, 5), mapper_model.Index(targets, k, 5)
    assert as_tuples(overlaps) == model.get_overlaps(mapper_model.match_anchors(mq, mt))[0] and len(overlaps) > 1
    cigars = align_overlaps(overlaps, [s for _, s in qrecords], [s for _, s in trecords])
    assert len(cigars) == len(overlaps)
    for o, cigar in zip(overlaps, cigars):
        ops = [(int(n), op) for n, op in re.findall(r"(\d+)([MIDX=])", cigar)]
        assert "".join("%d%s" % x for x in ops) == cigar and ops
        # I is present in the target only, D in the query only (cudaaligner.hpp)
        assert sum(n for n, op in ops if op != "I") == o.query_end - o.query_start
        assert sum(n for n, op in ops if op != "D") == o.target_end - o.target_start
    paf = format_paf(overlaps, cigars, qrecords, trecords, k)
    lines = paf.splitlines()
    assert len(lines) == len(overlaps)
    for o, text in zip(overlaps, lines):
        cols = text.split("\t")
        assert cols[0] == "q%d" % o.query_read_id and cols[5] == "t%d" % o.target_read_id and cols[4] == o.strand
    for drop in (False, True):
        assert as_tuples(post_process_overlaps(overlaps, drop)) == \
            model.post_process_overlaps(as_tuples(overlaps), drop)


# ---- C++ surface ------------------------------------------------------------------

CPP_PROGRAM = r"""
#include <claraparabricks/genomeworks/cudamapper/index.hpp>
#include <claraparabricks/genomeworks/cudamapper/matcher.hpp>
#include <claraparabricks/genomeworks/cudamapper/overlapper_triggered.hpp>
#include <cstdio>
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
    auto parser       = io::create_kseq_fasta_parser(argv[1], 0, false);
    auto allocator    = create_default_device_allocator();
    hipStream_t stream = 0;
    auto query_index  = Index::create_index(allocator, *parser, 0, 6, 15, 5);
    auto target_index = Index::create_index(allocator, *parser, 6, parser->get_num_seqences(), 15, 5);
    auto matcher = Matcher::create_matcher(allocator,
                                           *query_index,
                                           *target_index,
                                           stream);

    std::vector<Overlap> overlaps;
    OverlapperTriggered overlapper(allocator,
                                   stream);
    overlapper.get_overlaps(overlaps, matcher->anchors());
    print("overlap", overlaps);
    std::vector<Overlap> loose;
    Overlapper& base = overlapper;
    base.get_overlaps(loose, matcher->anchors(), 3, 0, 1000, 0.0f);
    print("loose", loose);
    Overlapper::post_process_overlaps(loose);
    print("processed", loose);
    matcher.reset(nullptr);
    return 0;
}
"""


def test_cpp_surface(tmp_path, matcher_reads):
    queries, targets = matcher_reads
    fasta = tmp_path / "reads.fasta"
    fasta.write_text("".join(">r%d\n%s\n" % (i, s) for i, s in enumerate(queries + targets)))
    src = tmp_path / "overlapper_api.cpp"
    src.write_text(CPP_PROGRAM)
    exe = tmp_path / "overlapper_api"
    lib = os.path.join(ROOT, "claragenomicsanalysis_amd", "lib")
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-std=c++17", "-O1",
                           "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
                           "-x", "c++", str(src), "-L", lib, "-lgwamd", "-Wl,-rpath," + lib, "-o", str(exe)])
    out = subprocess.check_output([str(exe), str(fasta)], timeout=120).decode().splitlines()
    printed = {}
    for text in out:
        tag, *f = text.split()
        printed.setdefault(tag, []).append((int(f[0]), int(f[1]), int(f[2]), int(f[3]), int(f[4]), int(f[5]), f[6],
                                            int(f[7]), bool(int(f[8]))))
    reads = queries + targets
    with Index(reads, 15, 5, 0, 6) as q, Index(reads, 15, 5, 6) as t:
        default, loose = match_overlaps(q, t), match_overlaps(q, t, *LOOSE)
        anchors = match_anchors(q, t)
    assert printed["overlap"] == as_tuples(default) == model.get_overlaps(anchors.tolist())[0]
    assert printed["loose"] == as_tuples(loose) and len(loose) >= len(default) > 1
    assert printed["processed"] == as_tuples(post_process_overlaps(loose)) == \
        model.post_process_overlaps(as_tuples(loose))
