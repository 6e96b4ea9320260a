"""GPU checks of the entries that take reads resident on the device
(DeviceReads): rescue_overlap_ends and align_overlaps give, overlap by overlap
and field by field, what their host-read forms give on the same input; the
CIGARs also equal the aligner oracle's.  Both are integer results, compared
exactly.  Regions of more than one 4,096-byte piece of the gather kernel, the
long-mode aligner kernel and the pipelined align_all() on device-added pairs
have sets of their own.  The argument checks that need a handle, and so a device, are here
too; those that need none are in test_resident_capi.py."""
import ctypes as C
import random

import pytest

import gather_cases
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


# ---- alignment of regions longer than one piece of the gather kernel ------------------------------

HM = 0  # the algorithm align_overlaps creates its aligners with (test_aligner_plan.HM)


def aligner_plan(monkeypatch, env, max_q, max_t, batch):
    """The plan report (test_aligner_plan.plan, with this device's facts) of the aligner that
    align_overlaps creates for these three sizes; leaves `env` set until the test ends."""
    from test_aligner_plan import ENV_NAMES, _lib, plan
    for k in ENV_NAMES:  # (restored after the test)
        monkeypatch.setenv(k, "")
    p = plan(_lib(), env, [HM, max_q, max_t, batch, 0, 0, 0, 0, 0, 0, 0, 0])
    assert "error" not in p and p["kernel"] == 1, p
    return p


def sprinkle(rng, s, count):
    """Lower case, N and other letters that no complement changes, at `count` places."""
    s = list(s)
    for _ in range(count):
        s[rng.randrange(len(s))] = rng.choice("NnacgtRY")
    return "".join(s)


def oracle_cigars(overlaps, queries, targets):
    from oracle import oracle
    mq = max(o.query_end - o.query_start for o in overlaps)
    pairs = []
    for o in overlaps:
        tr = targets[o.target_read_id][o.target_start:o.target_end]
        pairs.append((queries[o.query_read_id][o.query_start:o.query_end], rc(tr) if o.strand == "-" else tr))
    return [oracle.cigar(states) for states in oracle.align_batch(pairs, oracle.ALIGN_HM, mq)[0]]


@pytest.fixture(scope="module")
def long_align_set():
    """Ten overlaps whose regions have 4,100 to 13,000 bases, on both strands, at 5 % errors,
    with lower case and N inside the regions of both sides."""
    rng = random.Random(43)
    targets = [sprinkle(rng, "".join(rng.choice("ACGT") for _ in range(13100)), 200) for _ in range(3)]
    queries, overlaps = [], []
    for i, length in enumerate((4200, 4300, 6000, 8191, 8200, 9000, 10000, 12000, 12289, 12800)):
        t = targets[i % 3]
        ts = rng.randint(0, len(t) - length)
        strand = "+-"[i % 2]
        region = t[ts:ts + length]
        body = sprinkle(rng, mutate(rng, rc(region) if strand == "-" else region, 0.05), 8)
        pre = "".join(rng.choice("ACGT") for _ in range(rng.randrange(40)))
        queries.append(pre + body + "".join(rng.choice("ACGT") for _ in range(rng.randrange(40))))
        overlaps.append(cm.Overlap(i, i % 3, len(pre), len(pre) + len(body), ts, ts + length, strand, i))
    for o in overlaps:
        for length in (o.query_end - o.query_start, o.target_end - o.target_start):
            assert gather_cases.PIECE < 4100 <= length <= 13000
        for region in (queries[o.query_read_id][o.query_start:o.query_end],
                       targets[o.target_read_id][o.target_start:o.target_end]):
            assert set("Nn") <= set(region) and set(region) & set("acgt")
    host = {e: cm.align_overlaps(overlaps, queries, targets, num_alignment_engines=e) for e in (1, 2)}
    return queries, targets, overlaps, host, oracle_cigars(overlaps, queries, targets)


@pytest.mark.parametrize("engines", [1, 2])
def test_long_regions_on_handles_equal_the_host_read_call_and_the_oracle(long_align_set, engines, monkeypatch):
    queries, targets, overlaps, host, want = long_align_set
    max_q = max(o.query_end - o.query_start for o in overlaps)
    max_t = max(o.target_end - o.target_start for o in overlaps)
    # the slots of the aligner's sequence buffer begin at every lead, not on 16-byte boundaries only
    assert max(max_q, max_t) % 16 != 0
    p = aligner_plan(monkeypatch, {}, max_q, max_t, len(overlaps) // engines)
    assert p["stride"] == max(max_q, max_t) and not p["launch_long_mode"]
    with DeviceReads(queries) as q, DeviceReads(targets) as t:
        cigars = cm.align_overlaps(overlaps, q, t, num_alignment_engines=engines)
    assert len(cigars) == len(overlaps) and all(cigars)
    assert cigars == host[engines]
    assert cigars == want
    assert any("I" in c and "D" in c for c in cigars)


def test_a_long_mode_overlap_on_handles_equals_the_host_read_call_and_the_oracle(monkeypatch):
    # a query region past the short-mode limit of 16,384 bases: the long-mode Hirschberg-Myers
    # kernel (striped sweeps, patterns in HBM) on sequences that the gather kernel wrote, the
    # target reversed; two short overlaps share the call and the aligner
    rng = random.Random(47)
    big_t = sprinkle(rng, "".join(rng.choice("ACGT") for _ in range(17300)), 40)
    big_q = sprinkle(rng, mutate(rng, rc(big_t[150:17150]), 0.03), 40)
    small_t = "".join(rng.choice("ACGT") for _ in range(900))
    queries = [mutate(rng, small_t[100:420], 0.05), big_q, mutate(rng, rc(small_t[500:800]), 0.05)]
    targets = [small_t, big_t]
    overlaps = [cm.Overlap(0, 0, 0, len(queries[0]), 100, 420, "+", 1),
                cm.Overlap(1, 1, 0, len(big_q), 0, len(big_t), "-", 2),
                cm.Overlap(2, 0, 0, len(queries[2]), 500, 800, "-", 3)]
    assert 16384 < len(big_q) < 17300
    p = aligner_plan(monkeypatch, {}, len(big_q), len(big_t), len(overlaps))
    assert p["long_mode"] == 1 and p["launch_long_mode"] == 1
    assert not aligner_plan(monkeypatch, {}, 16384, len(big_t), len(overlaps))["launch_long_mode"]
    on_host = cm.align_overlaps(overlaps, queries, targets)
    with DeviceReads(queries) as q, DeviceReads(targets) as t:
        resident = cm.align_overlaps(overlaps, q, t)
    assert all(resident) and resident == on_host
    assert resident == oracle_cigars(overlaps, queries, targets)


def test_pipelined_stages_on_device_added_pairs(monkeypatch):
    # align_all() in stages on a batch whose sequences were gathered on the device: the stages
    # upload the lengths only.  1,500 overlaps of about 300 bases and one engine make one batch
    # of many grids' worth of pairs at one workgroup per CU, as in test_aligner_gpu.py
    from claragenomicsanalysis_amd import synth
    qs, ts = synth.pairs(79, 1500, 300, 330, 10, 10, 10)
    queries = [q.decode() for q in qs]
    strands = ["-" if i % 3 == 1 else "+" for i in range(len(ts))]
    targets = [rc(t.decode()) if s == "-" else t.decode() for t, s in zip(ts, strands)]
    overlaps = [cm.Overlap(i, i, 0, len(queries[i]), 0, len(targets[i]), strands[i], i) for i in range(len(qs))]
    max_q, max_t = max(map(len, queries)), max(map(len, targets))
    res = {}
    for mode in ("1", "3"):
        env = {"GWAMD_DIAG": "1", "GWAMD_ALIGNER_GRID": "1", "GWAMD_ALIGNER_PIPELINE": mode}
        p = aligner_plan(monkeypatch, env, max_q, max_t, len(overlaps))
        assert p["stages"] == int(mode) and len(overlaps) >= 4 * p["slots"]
        with DeviceReads(queries) as q, DeviceReads(targets) as t:
            res[mode] = cm.align_overlaps(overlaps, q, t, num_alignment_engines=1)
        assert res[mode] == cm.align_overlaps(overlaps, queries, targets, num_alignment_engines=1)
    assert res["3"] == res["1"]
    assert res["1"] == oracle_cigars(overlaps, queries, targets)


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
