"""GPU checks of the entries that take reads resident on the device
(DeviceReads): rescue_overlap_ends and align_overlaps give, overlap by overlap
and field by field, what their host-read forms give on the same input; the
CIGARs also equal the aligner oracle's.  Both are integer results, compared
exactly.  The argument checks that need a handle, and so a device, are here
too; those that need none are in test_resident_capi.py."""
import ctypes as C
import random

import pytest

import rescue_cases
from claragenomicsanalysis_amd import DeviceReads, load_library, rescue_overlap_ends
from claragenomicsanalysis_amd import cudamapper as cm

pytestmark = pytest.mark.gpu

COMP = {"A": "T", "T": "A", "C": "G", "G": "C"}
NAN = float("nan")


def rc(s):
    return "".join(COMP.get(c, c) for c in reversed(s))


def as_tuples(overlaps):
    return [(o.query_read_id, o.target_read_id, o.query_start, o.query_end, o.target_start, o.target_end, o.strand,
             o.num_residues, bool(o.overlap_complete)) for o in overlaps]


# ---- rescue ----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def rescue_set():
    queries, targets, overlaps = rescue_cases.random_set()
    host = {numbers: as_tuples(rescue_overlap_ends(overlaps, queries, targets, *numbers))
            for numbers in ((100, 0.9), (50, 0.5))}
    assert host[(100, 0.9)] != host[(50, 0.5)] and host[(100, 0.9)] != overlaps
    return queries, targets, overlaps, host


def test_rescue_on_two_handles_equals_the_host_read_call(rescue_set):
    queries, targets, overlaps, host = rescue_set
    with DeviceReads(queries) as q, DeviceReads(targets) as t:
        # two calls on one pair of handles
        for numbers in ((100, 0.9), (50, 0.5)):
            assert as_tuples(rescue_overlap_ends(overlaps, q, t, *numbers)) == host[numbers]
        assert rescue_overlap_ends([], q, t) == []


def test_rescue_with_one_handle_on_both_sides(rescue_set):
    queries, targets, overlaps, host = rescue_set
    reads = queries + targets
    shifted = [(o[0], o[1] + len(queries)) + o[2:] for o in overlaps]
    with DeviceReads(reads) as r:
        for numbers in ((100, 0.9), (50, 0.5)):
            got = as_tuples(rescue_overlap_ends(shifted, r, r, *numbers))
            assert [(o[0], o[1] - len(queries)) + o[2:] for o in got] == host[numbers]


def test_device_reads_count_against_the_pool(rescue_set):
    from claragenomicsanalysis_amd.cudaaligner import DeviceAllocator
    queries, targets, overlaps, host = rescue_set
    total = sum(len(r) for r in queries)
    pool = DeviceAllocator(64 << 20)
    q = DeviceReads(queries, allocator=pool)
    held = pool.used
    # the bases, padded at both ends, and n + 1 offsets
    assert total + 8 * (len(queries) + 1) <= held <= total + 8 * (len(queries) + 1) + 48
    with DeviceReads(targets) as t:
        assert as_tuples(rescue_overlap_ends(overlaps[:50], q, t, allocator=pool)) == host[(100, 0.9)][:50]
    assert pool.used == held
    q.close()
    assert pool.used == 0
    with pytest.raises(ValueError):
        rescue_overlap_ends(overlaps[:5], q, q)  # closed
    small = DeviceAllocator(total - 1)
    with pytest.raises(RuntimeError, match="pool"):
        DeviceReads(queries, allocator=small)
    assert small.used == 0


# ---- alignment ---------------------------------------------------------------------------

def mutate(rng, s, err):
    out = []
    for c in s:
        r = rng.random()
        if r < err / 3:
            continue
        if r < 2 * err / 3:
            out.append(rng.choice("ACGT"))
        elif r < err:
            out.append(c + rng.choice("ACGT"))
        else:
            out.append(c)
    return "".join(out)


@pytest.fixture(scope="module")
def align_set():
    """About 40 overlaps of 50 to 3,000 bases on both strands, and regions of 0 and 1 bases."""
    rng = random.Random(41)
    targets = ["".join(rng.choice("ACGT") for _ in range(rng.randint(1500, 3200))) for _ in range(5)]
    queries, overlaps = [], []
    for i in range(38):
        ti = rng.randrange(len(targets))
        t = targets[ti]
        length = rng.choice([50, 51, 200, 1000, 1500, min(3000, len(t))]) if i < 12 else rng.randint(50, len(t))
        ts = rng.randint(0, len(t) - length)
        strand = "+-"[i % 2]
        region = t[ts:ts + length]
        body = mutate(rng, rc(region) if strand == "-" else region, 0.08)
        pre = "".join(rng.choice("ACGT") for _ in range(rng.randrange(40)))
        queries.append(pre + body + "".join(rng.choice("ACGT") for _ in range(rng.randrange(40))))
        overlaps.append(cm.Overlap(i, ti, len(pre), len(pre) + len(body), ts, ts + length, strand, i))
    for qlen, tlen, strand in ((0, 0, "+"), (0, 1, "-"), (1, 0, "+"), (1, 1, "-"), (1, 1, "+"), (0, 37, "-")):
        overlaps.append(cm.Overlap(3, 2, 5, 5 + qlen, 9, 9 + tlen, strand, 1))
    host = {e: cm.align_overlaps(overlaps, queries, targets, num_alignment_engines=e) for e in (1, 3)}
    return queries, targets, overlaps, host


@pytest.mark.parametrize("engines", [1, 3])
def test_align_on_handles_equals_the_host_read_call_and_the_oracle(align_set, engines):
    from oracle import oracle
    queries, targets, overlaps, host = align_set
    with DeviceReads(queries) as q, DeviceReads(targets) as t:
        cigars = cm.align_overlaps(overlaps, q, t, num_alignment_engines=engines)
        assert cm.align_overlaps([], q, t) == []
    assert len(cigars) == len(overlaps)
    assert cigars == host[engines]
    mq = max(o.query_end - o.query_start for o in overlaps)
    for o, c in zip(overlaps, cigars):
        qr = queries[o.query_read_id][o.query_start:o.query_end]
        tr = targets[o.target_read_id][o.target_start:o.target_end]
        assert c == oracle.cigar(oracle.align(qr, rc(tr) if o.strand == "-" else tr, oracle.ALIGN_HM, mq))


def test_an_overlap_past_the_aligners_limit_is_left_without_a_cigar_in_both_paths(align_set):
    from claragenomicsanalysis_amd.cudaaligner import max_lengths
    queries, targets, overlaps, host = align_set
    limit = max_lengths("hirschberg_myers")[0]
    queries = queries + ["ACGT" * (limit // 4) + "A"]
    assert len(queries[-1]) == limit + 1
    few = overlaps[:3] + [cm.Overlap(len(queries) - 1, 0, 0, limit + 1, 0, 100, "+", 1)] + overlaps[3:5]
    on_host = cm.align_overlaps(few, queries, targets)
    with DeviceReads(queries) as q, DeviceReads(targets) as t:
        resident = cm.align_overlaps(few, q, t)
    assert resident == on_host
    assert resident[3] == "" and all(resident[:3]) and all(resident[4:])
    assert resident[:3] + resident[4:] == host[1][:5]


# ---- argument checks that need a handle ------------------------------------------------------

@pytest.fixture(scope="module")
def handles():
    with DeviceReads([b"ACGTACGTAC", b"ACGTAC"]) as q, DeviceReads([b"ACGTACGTACGT", b"ACGTAC", b""]) as t:
        yield q, t


GOOD = (1, 1, 1, 3, 2, 4, "+", 0, True)
BAD_OVERLAPS = {
    "query id at the count": (2, 1, 1, 3, 2, 4, "+", 0, True),
    "target id at the count": (1, 3, 1, 3, 2, 4, "+", 0, True),
    "query start after end": (1, 1, 4, 3, 2, 4, "+", 0, True),
    "query end after the read": (1, 1, 1, 7, 2, 4, "+", 0, True),
    "target start after end": (1, 1, 1, 3, 5, 4, "+", 0, True),
    "target end after the read": (1, 1, 1, 3, 2, 7, "+", 0, True),
    "target end after an empty read": (1, 2, 1, 3, 0, 1, "-", 0, True),
    "strand": (1, 1, 1, 3, 2, 4, "*", 0, True),
    "strand zero": (1, 1, 1, 3, 2, 4, "\0", 0, True),
}


@pytest.mark.parametrize("name", sorted(BAD_OVERLAPS))
def test_bad_overlaps_are_refused_by_every_entry(handles, name):
    q, t = handles
    for overlaps in ([BAD_OVERLAPS[name]], [GOOD, BAD_OVERLAPS[name]]):
        with pytest.raises(ValueError):
            rescue_overlap_ends(overlaps, q, t)
        with pytest.raises(ValueError):
            cm.align_overlaps(overlaps, q, t)
        with pytest.raises(ValueError):
            cm.gather_overlap_regions([o[:7] for o in overlaps], q, t, 16)
    assert as_tuples(rescue_overlap_ends([GOOD], q, t)) == as_tuples(rescue_overlap_ends(
        [GOOD], [b"ACGTACGTAC", b"ACGTAC"], [b"ACGTACGTACGT", b"ACGTAC", b""]))


def test_bad_numbers_are_refused(handles):
    q, t = handles
    L = load_library()
    for kw in (dict(extension=129), dict(extension=-1), dict(required_similarity=NAN)):
        with pytest.raises(ValueError):
            rescue_overlap_ends([GOOD], q, t, **kw)
        with pytest.raises(ValueError):  # the arguments of an empty list are checked all the same
            rescue_overlap_ends([], q, t, **kw)
    arr = (cm.Overlap * 1)(cm.Overlap(*GOOD))
    p, n, h = C.c_void_p(7), C.c_int64(7), C.c_void_p(7)
    assert L.gwamd_rescue_overlap_ends_resident(q._handle, t._handle, arr, -1, 100, 0.9, None, C.byref(p),
                                                C.byref(n)) == -1
    assert not p.value and n.value == 0
    assert L.gwamd_rescue_overlap_ends_resident(q._handle, t._handle, None, 1, 100, 0.9, None, C.byref(p),
                                                C.byref(n)) == -1
    assert L.gwamd_align_overlaps_resident(q._handle, t._handle, arr, -1, 1, C.byref(h)) == -1 and not h.value
    assert L.gwamd_align_overlaps_resident(q._handle, t._handle, None, 1, 1, C.byref(h)) == -1
    with pytest.raises(RuntimeError):
        cm.align_overlaps([GOOD], q, t, num_alignment_engines=0)
    # the hook: a stride smaller than a region, below 1, a negative count, NULL outputs
    for stride in (1, 0, -1):
        with pytest.raises(ValueError):
            cm.gather_overlap_regions([GOOD[:7]], q, t, stride)
    assert cm.gather_overlap_regions([GOOD[:7]], q, t, 2) == (b"CGGT", [2, 2])
    out = (C.c_char * 64)()
    lens = (C.c_int32 * 2)()
    assert L.gwamd_internal_gather_overlap_regions(q._handle, t._handle, arr, -1, 16, out, lens) == -1
    assert L.gwamd_internal_gather_overlap_regions(q._handle, t._handle, arr, 1, 16, None, lens) == -1
    assert L.gwamd_internal_gather_overlap_regions(q._handle, t._handle, arr, 1, 16, out, None) == -1
    assert L.gwamd_internal_gather_overlap_regions(q._handle, t._handle, arr, 1, 1 << 31, out, lens) == -1
    with pytest.raises(TypeError):
        rescue_overlap_ends([GOOD], q, [b"ACGTACGTACGT", b"ACGTAC"])
