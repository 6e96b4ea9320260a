"""CPU checks of cudapolish's resident route: the grouping of segments into
slices (gwamd_build_window_slices) against the model and against
gwamd_build_windows, racon's mean-quality filter with its boundary, racon's
coverage trimming, FASTQ qualities through the parser, and the argument checks
of a read set with qualities that are made before any device call."""
import random

import numpy as np
import pytest

import polish_cases as pc
import polish_model as pm
import polish_resident_model as rm
from claragenomicsanalysis_amd import cudamapper, cudapolish


def segment_array(records):
    return np.array(records, dtype=cudapolish.SEGMENT_DTYPE) if records else np.zeros(0, cudapolish.SEGMENT_DTYPE)


def random_reads(rng, n, lo, hi, alphabet="ACGT"):
    return ["".join(rng.choice(alphabet) for _ in range(rng.randint(lo, hi))) for _ in range(n)]


def random_job(seed):
    """(targets, queries, overlaps, paths): random overlaps with paths that fit, both strands."""
    rng = random.Random(seed)
    targets = random_reads(rng, 4, 0, 90) + [""]
    targets[2] = "ACGTNACGTN" * 5  # no overlap touches target 2
    queries = random_reads(rng, 6, 30, 80, "ACGTNacgt")
    overlaps, paths = [], []
    for _ in range(40):
        t = rng.choice((0, 1, 3))
        q = rng.randrange(len(queries))
        if len(targets[t]) == 0:
            continue
        ts = rng.randint(0, len(targets[t]) - 1)
        te = rng.randint(ts, len(targets[t]))
        qs = rng.randint(0, len(queries[q]) - 1)
        qe = rng.randint(qs, len(queries[q]))
        overlaps.append((q, t, qs, qe, ts, te, rng.choice("+-")))
        paths.append(pc.random_path(rng, te - ts, qe - qs))
    return targets, queries, overlaps, paths


def random_qualities(rng, reads, lo=33, hi=60):
    return ["".join(chr(rng.randint(lo, hi)) for _ in r) for r in reads]


# ---- grouping ---------------------------------------------------------------------------------------


@pytest.mark.parametrize("with_qualities", [False, True])
def test_build_window_slices_equals_model(with_qualities):
    targets, queries, overlaps, paths = random_job(78)
    quals = random_qualities(random.Random(5), queries) if with_qualities else None
    seen_quality_drop = False
    for w in (7, 16, 50):
        records = pm.window_segments(overlaps, paths, w)
        for cap in (100, 3, 1):
            for threshold in (0.0, 10.0, 13.5):
                expected = rm.build_window_slices([len(t) for t in targets], [len(q) for q in queries], overlaps,
                                                  records, w, cap, quals, int(round(10 * threshold)))
                got = cudapolish.build_window_slices(targets, queries, overlaps, segment_array(records), w, cap,
                                                     query_qualities=quals, quality_threshold=threshold)
                assert got == expected, (w, cap, threshold)
                seen_quality_drop |= got[2] > 0
                # lengths alone give the same grouping: no base is looked at
                assert cudapolish.build_window_slices([len(t) for t in targets], [len(q) for q in queries], overlaps,
                                                      segment_array(records), w, cap, query_qualities=quals,
                                                      quality_threshold=threshold) == expected
    assert seen_quality_drop == with_qualities


def test_slices_reconstitute_build_windows():
    # the slices, cut from the host strings, are the sequences gwamd_build_windows copies
    jobs = [random_job(79)[:3] + (None,)]
    _, draft, reads, overlaps = pc.e2e_input(length=400, reads=5)
    jobs.append(([draft], reads, overlaps, None))
    for targets, queries, overlaps, _ in jobs:
        rng = random.Random(3)
        paths = [pc.random_path(rng, o[5] - o[4], o[3] - o[2]) for o in overlaps]
        for w in (16, 50, pc.E2E_W):
            records = segment_array(pm.window_segments(overlaps, paths, w))
            for cap in (100, 3):
                windows, dropped = cudapolish.build_windows(targets, queries, overlaps, records, w, cap)
                slices, by_cap, by_quality = cudapolish.build_window_slices(targets, queries, overlaps, records, w,
                                                                            cap)
                assert (by_cap, by_quality) == (dropped, 0)
                assert len(slices) == len(windows)
                for a, b in zip(slices, windows):
                    assert [rm.slice_bases((targets, queries), sl) for sl in a["slices"]] == b["sequences"]
                    assert {k: a[k] for k in ("target", "window", "overlap", "t_begin", "t_end")} == \
                        {k: b[k] for k in ("target", "window", "overlap", "t_begin", "t_end")}


def test_quality_filter_drops_and_keeps():
    # two segments of one query in one window: bases 0..9 of quality 5, bases 10..19 of quality 30
    targets, queries = ["A" * 20], ["C" * 20]
    quals = [chr(33 + 5) * 10 + chr(33 + 30) * 10]
    overlaps = [(0, 0, 0, 20, 0, 20, "+")]
    records = [(0, 0, 0, 10, 0, 10, 0, 0), (0, 0, 10, 20, 10, 20, 0, 0), (0, 0, 0, 20, 0, 20, 0, 0)]
    got, by_cap, by_quality = cudapolish.build_window_slices(targets, queries, overlaps, segment_array(records), 20,
                                                             query_qualities=quals, quality_threshold=10.0)
    # mean 5 dropped, mean 30 kept, mean 17.5 kept
    assert by_quality == 1 and by_cap == 0
    assert got[0]["slices"] == [(0, 0, 0, 20, 0), (1, 0, 10, 20, 0), (1, 0, 0, 20, 0)]
    assert (got, by_cap, by_quality) == rm.build_window_slices([20], [20], overlaps, records, 20, 100, quals, 100)
    # without qualities nothing is dropped, and a dropped segment does not count against the cap
    assert cudapolish.build_window_slices(targets, queries, overlaps, segment_array(records), 20)[2] == 0
    capped = cudapolish.build_window_slices(targets, queries, overlaps, segment_array(records), 20, 3,
                                            query_qualities=quals)
    assert capped[1:] == (0, 1) and len(capped[0][0]["slices"]) == 3


def test_quality_filter_boundary_mean_equals_threshold():
    # 4 bases of quality 10, 10, 10, 11 and threshold 10.2: sum 41, 410 >= 408 keeps; 10.3: 410 < 412 drops
    targets, queries = ["A" * 8], ["CCCC"]
    overlaps = [(0, 0, 0, 4, 0, 8, "+")]
    records = segment_array([(0, 0, 0, 4, 0, 4, 0, 0)])

    def dropped(quality, threshold):
        quals = ["".join(chr(33 + q) for q in quality)]
        return cudapolish.build_window_slices(targets, queries, overlaps, records, 8, query_qualities=quals,
                                              quality_threshold=threshold)[2]

    assert dropped([10, 10, 10, 10], 10.0) == 0  # the mean equals the threshold: kept
    assert dropped([10, 10, 10, 9], 10.0) == 1   # 9.75
    assert dropped([10, 10, 10, 11], 10.2) == 0  # 10.25
    assert dropped([10, 10, 10, 11], 10.3) == 1
    assert dropped([0, 0, 0, 0], 0.0) == 0


def test_build_window_slices_refusals():
    targets, queries = ["ACGTACGT"], ["ACGT"]
    overlaps = [(0, 0, 0, 4, 0, 8, "+")]
    ok = segment_array([(0, 0, 0, 4, 0, 4, 0, 0)])
    for bad in ((1, 0, 0, 4, 0, 4, 0, 0), (0, 2, 0, 4, 0, 4, 0, 0), (0, 0, 0, 5, 0, 4, 0, 0), (0, 0, 3, 2, 0, 4, 0, 0)):
        with pytest.raises(ValueError):
            cudapolish.build_window_slices(targets, queries, overlaps, segment_array([bad]), 4)
    with pytest.raises(ValueError):
        cudapolish.build_window_slices(targets, queries, overlaps, ok, 0)
    with pytest.raises(ValueError):
        cudapolish.build_window_slices(targets, queries, overlaps, ok, 4, 0)
    with pytest.raises(ValueError):
        cudapolish.build_window_slices(targets, queries, overlaps, ok, 4, query_qualities=["III"])
    with pytest.raises(ValueError):
        cudapolish.build_window_slices(targets, queries, overlaps, ok, 4, query_qualities=["II I"])
    with pytest.raises(ValueError):
        cudapolish.build_window_slices(targets, queries, overlaps, ok, 4, query_qualities=["IIII"],
                                       quality_threshold=-1.0)


# ---- trimming ---------------------------------------------------------------------------------------

TRIM_CASES = [
    # (consensus, coverage, sequences, expected)
    ("nothing to trim", "ACGTAC", [3, 4, 5, 5, 4, 3], 7, "ACGTAC"),
    ("both ends", "ACGTACGT", [0, 1, 2, 3, 3, 2, 1, 0], 5, "GTAC"),
    ("one end", "ACGTAC", [1, 1, 4, 4, 4, 4], 9, "GTAC"),
    ("no index reaches the average", "ACGT", [1, 2, 2, 1], 9, "ACGT"),
    ("a single qualifying index", "ACGT", [1, 5, 2, 1], 9, "ACGT"),
    ("two qualifying indices", "ACGT", [1, 5, 2, 5], 9, "CGT"),
    ("average 0 for two sequences", "ACGT", [0, 0, 0, 0], 2, "ACGT"),
    ("empty", "", [], 5, ""),
]


@pytest.mark.parametrize("case", TRIM_CASES, ids=[c[0] for c in TRIM_CASES])
def test_trim_consensus_hand_cases(case):
    _, consensus, coverage, sequences, expected = case
    assert rm.trim_consensus(consensus, coverage, sequences) == expected
    assert cudapolish.trim_consensus(consensus, coverage, sequences) == expected


def test_trim_consensus_equals_model_on_random_coverage():
    rng = random.Random(11)
    for _ in range(200):
        n = rng.randint(0, 30)
        consensus = "".join(rng.choice("ACGT") for _ in range(n))
        coverage = [rng.randint(0, 12) for _ in range(n)]
        sequences = rng.randint(1, 25)
        assert cudapolish.trim_consensus(consensus, coverage, sequences) == \
            rm.trim_consensus(consensus, coverage, sequences)
    with pytest.raises(ValueError):
        cudapolish.trim_consensus("ACGT", [1, 2, 3], 4)
    with pytest.raises(ValueError):
        cudapolish.trim_consensus("ACGT", [1, 2, 3, 4], 0)


# ---- FASTQ ------------------------------------------------------------------------------------------


def test_fastq_qualities_multi_line_and_crlf(tmp_path):
    path = tmp_path / "reads.fastq"
    path.write_bytes(b"@r0 first\r\nACGT\r\nAC\r\n+\r\nIIII\r\n#!\r\n"
                     b"@r1\nGGGTTT\n+r1\n@@@+++\n"  # a quality line that begins with '@'
                     b"@r2\nA\n+\n~\n")
    records, quals = cudamapper.read_fasta_with_qualities(path, shuffle=False)
    assert records == [("r0", "ACGTAC"), ("r1", "GGGTTT"), ("r2", "A")]
    assert quals == ["IIII#!", "@@@+++", "~"]
    assert cudamapper.read_fasta(path, shuffle=False) == records
    # the shuffled order and the length filter keep each quality with its record
    by_name = dict(zip((r[0] for r in records), quals))
    for shuffle, min_length in ((True, 0), (True, 2), (False, 6)):
        rec, q = cudamapper.read_fasta_with_qualities(path, min_length, shuffle)
        assert rec == cudamapper.read_fasta(path, min_length, shuffle)
        assert sorted(r[0] for r in rec) == [n for n, s in records if len(s) >= min_length]
        assert q == [by_name[r[0]] for r in rec]


def test_fasta_has_empty_qualities(tmp_path):
    path = tmp_path / "reads.fasta"
    path.write_bytes(b">t0 x\r\nACGT\r\nACG\r\n>t1\nTTTT\n")
    records, quals = cudamapper.read_fasta_with_qualities(path, shuffle=False)
    assert records == [("t0", "ACGTACG"), ("t1", "TTTT")] == cudamapper.read_fasta(path, shuffle=False)
    assert quals == ["", ""]


def test_shuffled_order_is_the_parsers(tmp_path):
    # 40 records: std::shuffle(std::mt19937(0)) of the records, which read_fasta has always given
    path = tmp_path / "many.fastq"
    path.write_text("".join("@r%d\n%s\n+\n%s\n" % (i, "ACGT"[i % 4] * (i + 1), chr(40 + i) * (i + 1))
                            for i in range(40)))
    rec, quals = cudamapper.read_fasta_with_qualities(path)
    assert rec == cudamapper.read_fasta(path)
    assert [r[0] for r in rec] != ["r%d" % i for i in range(40)]
    for (name, seq), q in zip(rec, quals):
        assert q == chr(40 + int(name[1:])) * len(seq)


# ---- argument checks that need no device ----------------------------------------------------------------


@pytest.mark.parametrize("byte", [32, 127, 0, 200])
def test_quality_byte_outside_printable_range_is_refused(byte):
    quals = [b"IIII", b"II" + bytes([byte]) + b"I"]
    with pytest.raises(ValueError, match="33..126"):
        cudamapper.DeviceReads(["ACGT", "ACGT"], qualities=quals)


def test_quality_length_and_count_are_checked():
    with pytest.raises(ValueError, match="quality characters"):
        cudamapper.DeviceReads(["ACGT", "ACG"], qualities=["IIII", "IIII"])
    with pytest.raises(ValueError, match="quality strings"):
        cudamapper.DeviceReads(["ACGT", "ACG"], qualities=["IIII"])


def test_c_entry_checks_qualities_before_any_device_call():
    import ctypes as C

    from claragenomicsanalysis_amd._lib import last_error, load_library
    L = load_library()
    offsets = (C.c_int64 * 3)(0, 4, 7)
    h = C.c_void_p()
    assert L.gwamd_device_reads_create_with_qualities(b"ACGTACG", b"IIII I!", offsets, 2, 0, None, C.byref(h)) == -1
    assert "33..126" in last_error() and not h.value
    assert L.gwamd_device_reads_create_with_qualities(b"ACGTACG", None, offsets, 2, 0, None, C.byref(h)) == -1
    assert "NULL" in last_error() and not h.value
    assert L.gwamd_device_reads_has_qualities(None) == -1
