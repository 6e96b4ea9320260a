"""cudapolish's window cut on the GPU against the plain-Python model
(tests/polish_model.py): every word of every record.

The kernel walks a path in tiles of 1,024 states (64 lanes x 16 bytes), one
wave per overlap, four waves per workgroup; the path lengths sit one below, at
and above one and two tiles, and the overlap counts below, at and above one
workgroup.  Host-order paths are packed on 16-byte boundaries; the aligner's
order (end -> start, strided) goes through gwamd_internal_window_segments_strided
with strides of 4, 8 and 12 mod 16, so path starts fall on every dword alignment
and the buffer's last 16-byte chunk crosses its end.
"""
import random

import numpy as np
import pytest

import polish_cases as pc
import polish_model as pm

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 15, 16, 17, 1023, 1024, 1025, 2047, 2048, 2049]
STRIDES = [2052, 2056, 2060]  # 4, 8 and 12 mod 16, each at least the longest path


def path_of_length(rng, length):
    """A fitting path of exactly `length` states and its two spans."""
    diagonal = rng.randint(0, length)
    gaps = length - diagonal
    target_only = rng.randint(0, gaps)
    tl, ql = diagonal + target_only, diagonal + gaps - target_only
    path = pc.random_path(rng, tl, ql, diagonal)
    assert len(path) == length
    return path, tl, ql


def length_cases(seed):
    rng = random.Random(seed)
    overlaps, paths = [], []
    for length in LENGTHS:
        for strand in "+-":
            path, tl, ql = path_of_length(rng, length)
            ts, qs = rng.randint(0, 100), rng.randint(0, 100)
            overlaps.append((0, 0, qs, qs + ql, ts, ts + tl, strand))
            paths.append(path)
    return overlaps, paths


def hand_set():
    cases = pc.hand_cases()
    return [c[1] for c in cases], [c[2] for c in cases]


def strided(paths, stride, fill=9):
    """The aligner's layout: path i end -> start at i * stride, the rest of a slot never read."""
    buf = np.full(len(paths) * stride, fill, np.int8)
    for i, p in enumerate(paths):
        buf[i * stride:i * stride + len(p)] = np.asarray(p[::-1], dtype=np.int64).astype(np.int8)
    return buf.tobytes(), [len(p) for p in paths]


def cut(cudapolish, overlaps, paths, w):
    return pc.as_tuples(cudapolish.window_segments(overlaps, paths, w))


@pytest.fixture(scope="module")
def cudapolish():
    from claragenomicsanalysis_amd import cudapolish
    return cudapolish


def test_hand_cases_host_order(cudapolish):
    overlaps, paths = hand_set()
    got = cut(cudapolish, overlaps, paths, pc.W)
    expected = []
    for i, case in enumerate(pc.hand_cases()):
        expected += [(i,) + r[1:] for r in case[3]]
    assert got == expected
    assert got == pm.window_segments(overlaps, paths, pc.W)


@pytest.mark.parametrize("stride", [20, 24, 28])
def test_hand_cases_aligner_order(cudapolish, stride):
    overlaps, paths = hand_set()
    buf, lens = strided(paths, stride)
    got = pc.as_tuples(cudapolish._window_segments_strided(overlaps, buf, lens, stride, pc.W))
    assert got == pm.window_segments(overlaps, paths, pc.W)


@pytest.mark.parametrize("w", [8, 16])
def test_tile_lengths_host_order(cudapolish, w):
    overlaps, paths = length_cases(100 + w)
    assert cut(cudapolish, overlaps, paths, w) == pm.window_segments(overlaps, paths, w)


@pytest.mark.parametrize("w", [8, 16])
@pytest.mark.parametrize("stride", STRIDES)
def test_tile_lengths_aligner_order(cudapolish, stride, w):
    overlaps, paths = length_cases(200 + w)
    buf, lens = strided(paths, stride)
    got = pc.as_tuples(cudapolish._window_segments_strided(overlaps, buf, lens, stride, w))
    assert got == pm.window_segments(overlaps, paths, w)


@pytest.mark.parametrize("count", [1, 3, 4, 5, 257])
def test_overlap_counts(cudapolish, count):
    rng = random.Random(count)
    overlaps, paths = [], []
    for _ in range(count):
        path, tl, ql = path_of_length(rng, rng.randint(0, 90))
        ts, qs = rng.randint(0, 50), rng.randint(0, 50)
        overlaps.append((0, 0, qs, qs + ql, ts, ts + tl, rng.choice("+-")))
        paths.append(path)
    expected = pm.window_segments(overlaps, paths, 8)
    assert cut(cudapolish, overlaps, paths, 8) == expected
    buf, lens = strided(paths, 92)  # 12 mod 16
    assert pc.as_tuples(cudapolish._window_segments_strided(overlaps, buf, lens, 92, 8)) == expected


@pytest.mark.parametrize("w", [1, 3, 7, 500, 1000003, (1 << 31) - 1])
def test_window_lengths(cudapolish, w):
    # the kernel divides by w with a reciprocal the host prepares
    rng = random.Random(w)
    overlaps, paths = [], []
    for _ in range(6):
        path, tl, ql = path_of_length(rng, rng.randint(1, 1500))
        ts = rng.choice((0, 5, w - 1, w, 2 * w + 3, (1 << 31) - 1 - tl))
        ts = max(0, min(ts, (1 << 31) - 1 - tl))
        overlaps.append((0, 0, 7, 7 + ql, ts, ts + tl, rng.choice("+-")))
        paths.append(path)
    assert cut(cudapolish, overlaps, paths, w) == pm.window_segments(overlaps, paths, w)


def misfit_call(rng):
    """Five overlaps over two tiles each, the second, third and fourth with a path that does not fit."""
    overlaps, paths = [], []
    for i in range(5):
        path, tl, ql = path_of_length(rng, 1500)
        if i == 1:    # one target state too many
            path.insert(700, 2)
            ql += 1   # (room for the longer path: the check of the length is against the two spans together)
        elif i == 2:  # one state short
            del path[800]
        elif i == 3:  # a bad byte
            path[1100] = 7
        overlaps.append((0, 0, 3, 3 + ql, 11, 11 + tl, "+-"[i % 2]))
        paths.append(path)
    return overlaps, paths


def test_misfits_in_the_middle_of_a_call(cudapolish):
    overlaps, paths = misfit_call(random.Random(31))
    expected = pm.window_segments(overlaps, paths, 16)
    flagged = sorted({r[0] for r in expected if r[6] & pm.BAD_PATH})
    assert flagged == [1, 2, 3]
    assert all(r[6] & pm.EMPTY and r[2:6] == (0, 0, 0, 0) for r in expected if r[0] in flagged)
    assert cut(cudapolish, overlaps, paths, 16) == expected
    buf, lens = strided(paths, 1512)  # 8 mod 16
    assert pc.as_tuples(cudapolish._window_segments_strided(overlaps, buf, lens, 1512, 16)) == expected


def test_pool_is_returned(cudapolish):
    from claragenomicsanalysis_amd.cudaaligner import DeviceAllocator
    pool = DeviceAllocator(64 << 20)
    overlaps, paths = length_cases(5)
    assert pool.used == 0
    got = pc.as_tuples(cudapolish.window_segments(overlaps, paths, 8, allocator=pool))
    assert pool.used == 0 and got == pm.window_segments(overlaps, paths, 8)
    small = DeviceAllocator(1 << 10)
    with pytest.raises(RuntimeError):
        cudapolish.window_segments(overlaps, paths, 8, allocator=small)
    assert small.used == 0


# ---- the resident route -------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def resident_input():
    """12 reads of about 1.2 kb against two targets, both strands, partial overlaps among them."""
    rng = random.Random(12)
    truth = ["".join(rng.choice("ACGT") for _ in range(1200)) for _ in range(2)]
    queries, overlaps = [], []
    for i in range(12):
        t = i % 2
        read = pc.mutate(rng, truth[t], 0.08)
        reverse = i % 3 == 0
        queries.append(pm.reverse_complement(read) if reverse else read)
        if i < 8:
            overlaps.append((i, t, 0, len(read), 0, 1200, "-" if reverse else "+"))
        else:  # a part of the read against a part of the target
            overlaps.append((i, t, 100, len(read) - 150, 130, 1010, "-" if reverse else "+"))
    overlaps.append((3, 1, 40, 40, 500, 500, "+"))  # nothing to align, no record
    overlaps.append((4, 0, 10, 10, 300, 420, "-"))  # a target span without a query base
    return truth, queries, overlaps


def test_resident_route(cudapolish, resident_input):
    from claragenomicsanalysis_amd.cudaaligner import CudaAlignerBatch
    from claragenomicsanalysis_amd.cudamapper import DeviceReads
    from oracle import oracle
    targets, queries, overlaps = resident_input
    with DeviceReads(queries) as q, DeviceReads(targets) as t:
        one = pc.as_tuples(cudapolish.window_segments_resident(overlaps, q, t, 16))
        two = pc.as_tuples(cudapolish.window_segments_resident(overlaps, q, t, 16, num_alignment_engines=2))
        with pytest.raises(ValueError):
            cudapolish.window_segments_resident(overlaps, q, t, 0)
        with pytest.raises(ValueError):
            cudapolish.window_segments_resident(overlaps, q, t, 16, num_alignment_engines=0)
        with pytest.raises(ValueError):
            cudapolish.window_segments_resident([(0, 0, 0, 5000, 0, 10, "+")], q, t, 16)
    assert one == two
    # the same regions through the public aligner, its paths downloaded
    batch = CudaAlignerBatch(1500, 1500, len(overlaps))
    for qi, ti, qs, qe, ts, te, strand in overlaps:
        assert batch.add_alignment(queries[qi][qs:qe], targets[ti][ts:te], False, strand == "-") == 0
    batch.align_all()
    paths = [a.alignment for a in batch.get_alignments()]
    assert one == pc.as_tuples(cudapolish.window_segments(overlaps, paths, 16))
    assert one == pm.window_segments(overlaps, pc.oracle_paths(oracle, queries, targets, overlaps), 16)
    assert not any(r[6] & (pm.BAD_PATH | pm.NOT_ALIGNED) for r in one)


def test_resident_route_with_an_overlap_past_the_aligners_limit(cudapolish, resident_input):
    """One overlap in the middle of the list is left out by the aligner's limits: every overlap
    after it has another index among the aligned ones than in the call, and with two engines one
    batch begins past the first aligned overlap."""
    from claragenomicsanalysis_amd.cudaaligner import max_lengths
    from claragenomicsanalysis_amd.cudamapper import DeviceReads
    from oracle import oracle
    targets, queries, overlaps = resident_input
    limit = max_lengths("hirschberg_myers")[0]
    queries = queries + ["ACGT" * (limit // 4) + "A"]
    assert len(queries[-1]) == limit + 1
    at = len(overlaps) // 2
    overlaps = overlaps[:at] + [(len(queries) - 1, 0, 0, limit + 1, 0, 100, "+")] + overlaps[at:]
    with DeviceReads(queries) as q, DeviceReads(targets) as t:
        one = pc.as_tuples(cudapolish.window_segments_resident(overlaps, q, t, 16, num_alignment_engines=1))
        two = pc.as_tuples(cudapolish.window_segments_resident(overlaps, q, t, 16, num_alignment_engines=2))
    assert one == two
    aligned = [i != at for i in range(len(overlaps))]
    paths = pc.oracle_paths(oracle, queries, targets, overlaps[:at]) + [[]] + \
        pc.oracle_paths(oracle, queries, targets, overlaps[at + 1:])
    expected = pm.window_segments(overlaps, paths, 16, aligned)
    assert [r for r in expected if r[0] == at] == [(at, j, 0, 0, 0, 0, pm.EMPTY | pm.NOT_ALIGNED, 0) for j in range(7)]
    assert one == expected


def test_cpp_interface(tmp_path):
    import subprocess
    r = subprocess.run([pc.build_cpp_check(tmp_path), "gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == [word for name in pc.CPP_HOST + pc.CPP_GPU for word in ("ok", name)]


# ---- end to end ---------------------------------------------------------------------------------------


def test_polish_end_to_end(cudapolish):
    """A 1,200-base truth, a draft at 4 % errors, 12 reads at 10 %, w = 200, full POA.  Through the
    oracle alone (model cut, oracle.poa_window) the draft of this seed is 42 edits from the truth
    and the polished sequence 0."""
    from oracle import oracle
    truth, draft, queries, overlaps = pc.e2e_input()
    polished, stats, windows, consensus, status = cudapolish.polish(
        [draft], queries, overlaps, window_length=pc.E2E_W, banded=False, return_windows=True)
    # (a) the windows are the model's, fed the oracle's paths
    records = pm.window_segments(overlaps, pc.oracle_paths(oracle, queries, [draft], overlaps), pc.E2E_W)
    expected, dropped = pm.build_windows([draft], queries, overlaps, records, pc.E2E_W)
    assert windows == expected and stats["dropped_by_cap"] == dropped == 0
    # (b) each consensus is the oracle's on that window
    size = stats["max_sequence_size"]
    results = [oracle.poa_window(w["sequences"], max_nodes=3 * size, max_consensus=2 * size, max_seqs=100)
               for w in windows]
    assert all(len(w["sequences"]) >= 3 for w in windows)
    assert status == [r.status for r in results] == [0] * len(windows)
    assert consensus == [r.consensus for r in results]
    model_polished, model_stats = pm.polish([draft], expected, lambda w: (0, results[expected.index(w)].consensus))
    assert polished == model_polished
    assert {k: stats[k] for k in model_stats} == model_stats
    # (c) a sanity bound: polishing brings the draft closer to the truth
    before, after = oracle.edit_distance(draft, truth), oracle.edit_distance(polished[0], truth)
    print("edit distance to the truth: draft %d, polished %d" % (before, after))
    assert after < before
