"""GPU check of gather_overlap_regions_kernel (csrc/mapper_gather.hip) through
its test hook, gwamd_internal_gather_overlap_regions, against slices of the
read strings: bytes [0, length) of every slot and both lengths are compared
exactly, and bytes [length, stride) of every slot are the zeros the hook put
there before the launch.  The kernel moves bytes, so there is no tolerance.

Two calls of about 200 overlaps over 6 reads per side.  Every region length of
LENGTHS begins at each of the source offsets 0..7 of its read on both sides,
which with reads that begin at any address covers every misalignment of the
kernel's word loads; the second call has every strand flipped, so each (length,
offset) is reverse-complemented once and copied once.

Those regions are at most 1,296 bytes, one piece of the kernel (one wave).  The
tests over gather_cases.case_sets() have regions of 4,080 to 12,300 bytes, up
to four pieces, one launch per case set; test_gather_cases_cpu.py shows which
chunks, pieces and leads they reach."""
import random

import pytest

import gather_cases
from claragenomicsanalysis_amd.cudamapper import DeviceReads, gather_overlap_regions
from gather_cases import COMPLEMENT, expected

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1025]
LONG = (0, 3, 5)  # the reads long enough for every region; 1, 2 and 4 have 0, 1 and 0 bases


def make_reads(seed):
    rng = random.Random(seed)
    reads = []
    for length in (1296, 0, 1, 1100, 0, 1040):
        read = bytearray(rng.choice(b"ACGT") for _ in range(length))
        for _ in range(length // 12):  # bytes the complement keeps
            read[rng.randrange(length)] = rng.choice(b"NnacgtRY\x80\xff\x00")
        reads.append(bytes(read))
    return reads


def make_overlaps(queries, targets):
    overlaps = []
    for li, length in enumerate(LENGTHS):
        for offset in range(8):
            q, t = LONG[(li + offset) % 3], LONG[(li + 2 * offset + 1) % 3]
            strand = "-" if (li + offset) % 2 else "+"
            overlaps.append((q, t, offset, offset + length, offset, offset + length, strand))
    last = len(queries) - 1
    for length in (1, 16, 17, 257):
        for strand in "+-":
            # from base 0 of read 0 and up to the last base of the last read: the two ends of the buffer
            overlaps.append((0, 0, 0, length, 0, length, strand))
            overlaps.append((last, last, len(queries[last]) - length, len(queries[last]),
                             len(targets[last]) - length, len(targets[last]), strand))
    for read in range(len(queries)):  # whole reads, the empty ones and the single bases among them
        for strand in "+-":
            overlaps.append((read, (read + 1) % len(targets), 0, len(queries[read]), 0,
                             len(targets[(read + 1) % len(targets)]), strand))
            overlaps.append((read, read, 0, len(queries[read]), 0, len(targets[read]), strand))
    # odd and even lengths on '-' around the middle base
    for length in (9, 10, 31, 32, 33):
        overlaps.append((3, 3, 2, 2 + length, 5, 5 + length, "-"))
    return overlaps


def check(overlaps, queries, targets, query_reads, target_reads, stride):
    want, want_lens = expected(overlaps, queries, targets, stride)
    seqs, lens = gather_overlap_regions(overlaps, query_reads, target_reads, stride)
    assert lens == want_lens
    assert len(seqs) == 2 * len(overlaps) * stride
    for slot, region in enumerate(want):
        got = seqs[slot * stride:slot * stride + len(region)]
        assert got == region, (slot, overlaps[slot // 2])
        # the hook clears the buffer and the kernel writes nothing outside a region
        rest = seqs[slot * stride + len(region):(slot + 1) * stride]
        assert rest.count(0) == len(rest), (slot, overlaps[slot // 2])


def test_complement_table():
    assert b"ACGTNacgt\x80".translate(COMPLEMENT) == b"TGCANacgt\x80"


def test_two_read_sets_and_a_stride_equal_to_the_longest_region():
    queries, targets = make_reads(1), make_reads(2)
    overlaps = make_overlaps(queries, targets)
    assert 180 <= len(overlaps) <= 230
    assert {o[6] for o in overlaps} == {"+", "-"}
    stride = max(max(o[3] - o[2], o[5] - o[4]) for o in overlaps)
    assert stride == 1296 and stride % 16 == 0
    with DeviceReads(queries) as q, DeviceReads(targets) as t:
        assert (q.number_of_reads, q.number_of_basepairs) == (6, sum(map(len, queries)))
        check(overlaps, queries, targets, q, t, stride)
        # n == 0 returns without a launch
        assert gather_overlap_regions([], q, t, 16) == (b"", [])


def test_one_read_set_on_both_sides_and_a_stride_that_is_no_multiple_of_16():
    reads = make_reads(3)
    flipped = [o[:6] + ("+" if o[6] == "-" else "-",) for o in make_overlaps(reads, reads)]
    with DeviceReads(reads) as r:
        for stride in (1301, 1297):
            assert stride % 16 and stride % 4
            check(flipped, reads, reads, r, r, stride)


def test_one_overlap_and_short_strides():
    reads = make_reads(4)
    with DeviceReads(reads) as r:
        for stride in (1, 2, 3, 5, 16, 17):
            overlaps = [(0, 3, k, k + stride, k + 1, k + 1 + stride, "+-"[k % 2]) for k in range(9)]
            check(overlaps[:1], reads, reads, r, r, stride)
            check(overlaps, reads, reads, r, r, stride)


# ---- regions of more than one piece (gather_cases.py) --------------------------------------------

@pytest.fixture(scope="module")
def long_sets():
    return gather_cases.case_sets()


def check_set(long_sets, name):
    queries, targets, overlaps, stride = long_sets[name]
    assert max(max(o[3] - o[2], o[5] - o[4]) for o in overlaps) > 2 * gather_cases.PIECE
    if queries is targets:
        with DeviceReads(queries) as r:
            check(overlaps, queries, targets, r, r, stride)
    else:
        with DeviceReads(queries) as q, DeviceReads(targets) as t:
            check(overlaps, queries, targets, q, t, stride)


@pytest.mark.parametrize("stride", gather_cases.STRIDES)
def test_regions_around_the_piece_seams(long_sets, stride):
    # 12301: targets at every odd lead and queries at every even one; 12304: lead 0, one chunk in
    # the last piece of a 12,300-byte region; 12288: lead 0, the last piece of a 12,288-byte region empty
    check_set(long_sets, "stride_%d" % stride)


def test_regions_around_the_piece_seams_with_targets_at_even_leads(long_sets):
    for stride in gather_cases.EVEN_LEAD_STRIDES:
        check_set(long_sets, "stride_%d" % stride)


def test_long_regions_of_one_read_set_on_both_sides_with_every_strand_flipped(long_sets):
    assert long_sets["one_read_set_flipped"][0] is long_sets["one_read_set_flipped"][1]
    check_set(long_sets, "one_read_set_flipped")


def test_one_long_reverse_overlap_is_four_pieces_per_slot(long_sets):
    for stride in gather_cases.STRIDES[:2]:
        assert len(long_sets["one_overlap_%d" % stride][2]) == 1
        check_set(long_sets, "one_overlap_%d" % stride)
