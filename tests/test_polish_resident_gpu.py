"""cudapolish.polish on its resident route: windows as slices of the resident
reads, base qualities as POA weights, racon's mean-quality filter and coverage
trimming, on polish_cases.e2e_input() (a 1,200-base truth, a draft at 4 %
errors, 12 reads at 10 %, w = 200, full POA)."""
import random

import numpy as np
import pytest

import polish_cases as pc
import polish_model as pm
import polish_resident_model as rm
from claragenomicsanalysis_amd import cudapolish
from oracle import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def job():
    truth, draft, queries, overlaps = pc.e2e_input()
    records = pm.window_segments(overlaps, pc.oracle_paths(oracle, queries, [draft], overlaps), pc.E2E_W)
    default = cudapolish.polish([draft], queries, overlaps, window_length=pc.E2E_W, banded=False,
                                return_windows=True)
    return truth, draft, queries, overlaps, records, default


def synthetic_qualities(draft, queries):
    """Seeded Phred + 33 strings: 20..40 everywhere, but 2..8 on bases 150..650 of
    reads 3 and 8, so that the segments those stretches cover have a mean below 10."""
    rng = random.Random(9)
    quals = []
    for i, q in enumerate(queries):
        values = [rng.randint(20, 40) for _ in q]
        if i in (3, 8):
            values[150:650] = [rng.randint(2, 8) for _ in values[150:650]]
        quals.append("".join(chr(33 + v) for v in values))
    target = ["".join(chr(33 + rng.randint(5, 30)) for _ in draft)]
    return quals, target


def test_device_windows_equal_the_default_route(job):
    _, draft, queries, overlaps, _, default = job
    polished, stats, windows, consensus, status = default
    got = cudapolish.polish([draft], queries, overlaps, window_length=pc.E2E_W, banded=False, return_windows=True,
                            device_windows=True)
    assert got[0] == polished
    assert got[1] == stats and stats["dropped_by_quality"] == 0 and stats["trimmed_bases"] == 0
    assert [w["sequences"] for w in got[2]] == [w["sequences"] for w in windows]
    for key in ("target", "window", "overlap", "t_begin", "t_end"):
        assert [w[key] for w in got[2]] == [w[key] for w in windows]
    assert all(w["weights"] == [[1] * len(s) for s in w["sequences"]] for w in got[2])
    assert got[3] == consensus and got[4] == status


def test_qualities_weigh_filter_and_trim(job):
    truth, draft, queries, overlaps, records, default = job
    quals, target_quals = synthetic_qualities(draft, queries)
    polished, stats, windows, consensus, status = cudapolish.polish(
        [draft], queries, overlaps, window_length=pc.E2E_W, banded=False, return_windows=True,
        query_qualities=quals, target_qualities=target_quals, quality_threshold=10.0)
    # (a) windows, weights and the filter's count are the model's
    expected, by_cap, by_quality = rm.build_window_slices([len(draft)], [len(q) for q in queries], overlaps, records,
                                                          pc.E2E_W, 100, quals, 100)
    assert by_quality >= 1 and by_cap == 0  # the filter does drop something here
    assert (stats["dropped_by_quality"], stats["dropped_by_cap"]) == (by_quality, by_cap)
    assert len(windows) == len(expected)
    sets, qualities = ([draft], queries), (target_quals, quals)
    for got, want in zip(windows, expected):
        assert {k: got[k] for k in want} == want
        assert got["sequences"] == [rm.slice_bases(sets, sl) for sl in want["slices"]]
        assert got["weights"] == [rm.slice_weights(qualities, sl) for sl in want["slices"]]
    assert sum(len(w["slices"]) for w in windows) == sum(len(w["sequences"]) for w in default[2]) - by_quality
    # (b) each consensus is the oracle's with those weights
    size = stats["max_sequence_size"]
    results = [oracle.poa_window([s.encode() for s in w["sequences"]],
                                 weights=[np.array(x, np.int8) for x in w["weights"]], max_nodes=3 * size,
                                 max_consensus=2 * size, max_seqs=100) for w in windows]
    assert all(len(w["sequences"]) >= 3 for w in windows)
    assert status == [r.status for r in results] == [0] * len(windows)
    assert consensus == [r.consensus for r in results]
    assert polished == ["".join(r.consensus for r in results)] and stats["trimmed_bases"] == 0
    # (c) trim=True is the model's trimming of the oracle's coverage
    trimmed, trim_stats = cudapolish.polish([draft], queries, overlaps, window_length=pc.E2E_W, banded=False,
                                            query_qualities=quals, target_qualities=target_quals, trim=True)
    parts = [rm.trim_consensus(r.consensus, r.coverage, len(w["sequences"])) for r, w in zip(results, windows)]
    assert trimmed == ["".join(parts)]
    assert trim_stats["trimmed_bases"] == sum(len(r.consensus) for r in results) - len(trimmed[0])
    # (d) for the record, not asserted: nobody has measured which of the two is closer
    print("edit distance to the truth: draft %d, unweighted %d, weighted %d, weighted and trimmed %d"
          % (oracle.edit_distance(draft, truth), oracle.edit_distance(default[0][0], truth),
             oracle.edit_distance(polished[0], truth), oracle.edit_distance(trimmed[0], truth)))
