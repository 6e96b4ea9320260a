"""The reference of tests/test_polish_e2e_gpu.py on its own, without a GPU: on
polish_e2e_cases.hard_input() the model and the oracle do meet the conditions
that keep the GPU comparison from being vacuous: a window whose POA runs out
of nodes, windows of fewer than three sequences after windows that go to the
POA, pieces dropped by the cap and by the quality filter, and a consensus that
the trimming shortens.
"""
import pytest

import polish_e2e_cases as ec
from oracle import oracle

W = 200
JUNK_WINDOW = 1  # the window of target 0 the junk reads overlap


@pytest.fixture(scope="module")
def inputs():
    return {w: ec.hard_input(w) for w in (200, 500)}


def counts_of(result):
    return [len(win["sequences"]) for win in result["slice_windows"]]


def poa_statuses(result):
    return [s for s in result["status"] if s is not None]


def assert_only_the_junk_window_fails(result):
    assert result["status"][JUNK_WINDOW] == ec.NODE_LIMIT_STATUS
    assert poa_statuses(result).count(0) == len(poa_statuses(result)) - 1 > 0
    assert result["consensus"][JUNK_WINDOW] == ""
    assert result["stats"]["backbone_by_status"] == 1


@pytest.mark.parametrize("banded, node_limit", [(False, 768), (True, 1024)])
def test_plain_run_has_a_failing_window_and_backbones_by_rule(inputs, banded, node_limit):
    r = ec.expected(inputs[W], W, banded=banded, band_width=256, cap=100)
    stats, counts = r["stats"], counts_of(r)
    assert stats["max_sequence_size"] == 256
    assert ((4 if banded else 3) * stats["max_sequence_size"] + 3) // 4 * 4 == node_limit
    # the recipe alone decides these: 11 or 16 pieces and the backbone on target 0, whose last window the
    # partial reads reach only with insertion states; then 6, 6, 2 on target 1 and two windows without a read
    assert counts == [12, 17, 12, 12, 12, 9, 6, 6, 2, 1, 1]
    assert [win["target"] for win in r["slice_windows"]] == [0] * 6 + [1] * 3 + [2] * 2
    assert_only_the_junk_window_fails(r)
    assert stats["windows"] == 11 and stats["backbone_by_rule"] == 3
    assert stats["dropped_by_cap"] == stats["dropped_by_quality"] == stats["trimmed_bases"] == 0
    # windows that go to the POA lie on both sides of a failing one, and before a backbone by rule
    first_backbone = min(i for i, n in enumerate(counts) if n < 3)
    assert JUNK_WINDOW < first_backbone and any(n >= 3 for n in counts[JUNK_WINDOW + 1:first_backbone])
    assert counts[first_backbone - 2:first_backbone + 1] == [6, 6, 2]
    # every target is the join of its windows; the one without overlaps and the empty one come back as given
    targets = inputs[W][1]
    assert r["polished"][2] == targets[2] and r["polished"][3] == "" and len(r["polished"]) == 4
    assert r["polished"][0] != targets[0] and r["polished"][1] != targets[1]
    # the junk reads share no letter with anything: every base of theirs is a new node
    junk = r["slice_windows"][JUNK_WINDOW]["sequences"][1:1 + ec.JUNK_READS]
    assert not set("".join(junk)) & set("ACGTN") and sum(len(s) for s in junk) > node_limit - W


def test_cap_of_six_keeps_the_junk_reads(inputs):
    r = ec.expected(inputs[W], W, banded=True, band_width=128, cap=6)
    assert r["stats"]["max_sequence_size"] == 256
    assert max(counts_of(r)) == 6
    assert r["stats"]["dropped_by_cap"] == 38  # 6 + 11 + 3 * 6 + 3 on target 0, none on target 1
    assert r["slice_windows"][JUNK_WINDOW]["overlap"] == [-1] + list(range(ec.JUNK_READS))
    assert_only_the_junk_window_fails(r)


def test_quality_filter_drops_the_junk_reads(inputs):
    r = ec.expected(inputs[W], W, qualities=True, threshold=10.0)
    assert r["stats"]["max_sequence_size"] == 256
    assert r["stats"]["dropped_by_quality"] == ec.JUNK_READS == 5
    assert poa_statuses(r) and all(s == 0 for s in poa_statuses(r))
    assert r["stats"]["backbone_by_status"] == 0
    # the weights are the qualities, not ones
    assert any(x != 1 for win in r["slice_windows"] for ws in win["weights"] for x in ws)
    assert r["windows"] is None


def test_threshold_zero_keeps_them(inputs):
    r = ec.expected(inputs[W], W, qualities=True, threshold=0.0)
    assert r["stats"]["max_sequence_size"] == 256
    assert r["stats"]["dropped_by_quality"] == 0
    assert_only_the_junk_window_fails(r)
    plain = ec.expected(inputs[W], W)
    assert counts_of(r) == counts_of(plain)
    assert r["consensus"] != plain["consensus"]  # the weights do change a consensus


@pytest.mark.parametrize("qualities, threshold", [(False, 10.0), (True, 10.0), (True, 0.0)])
def test_default_window_length(inputs, qualities, threshold):
    r = ec.expected(inputs[500], 500, banded=True, band_width=256, qualities=qualities, threshold=threshold)
    assert r["stats"]["max_sequence_size"] == 576
    dropped = qualities and threshold > 0
    assert counts_of(r) == ([12, 12, 9, 6, 1] if dropped else [12, 17, 9, 6, 1])
    assert r["stats"]["dropped_by_quality"] == (ec.JUNK_READS if dropped else 0)
    if dropped:
        assert all(s == 0 for s in poa_statuses(r))
    else:
        assert_only_the_junk_window_fails(r)


def test_scores_and_trim(inputs):
    scores = (4, -4, -6)
    r = ec.expected(inputs[W], W, banded=True, band_width=256, scores=scores, trim=True)
    untrimmed = ec.expected(inputs[W], W, banded=True, band_width=256, scores=scores)
    assert r["stats"]["max_sequence_size"] == 256
    assert r["stats"]["trimmed_bases"] > 0
    assert r["consensus"] == untrimmed["consensus"]  # per window as the POA gives it
    assert sum(len(t) for t in untrimmed["polished"]) - sum(len(t) for t in r["polished"]) == \
        r["stats"]["trimmed_bases"]
    # the scores do reach the consensus
    assert r["consensus"] != ec.expected(inputs[W], W, banded=True, band_width=256)["consensus"]


def test_band_width_and_mode_reach_the_consensus(inputs):
    """If banded mode, or the band's width, changed nothing on this input, the GPU test could not
    tell whether polish() passes them on.  At cap 100 they change nothing: every window of 200 bases
    lies inside a band of 128, and the junk window exceeds both node limits.  So the GPU test has two
    configurations of its own, and these are the differences they rest on."""
    full = ec.expected(inputs[W], W, banded=False)
    for band_width in (128, 256):
        banded = ec.expected(inputs[W], W, banded=True, band_width=band_width)
        assert (full["status"], full["consensus"]) == (banded["status"], banded["consensus"])
    # cap 5: the backbone and four junk reads need more than 768 nodes and fewer than 1,024
    full = ec.expected(inputs[W], W, banded=False, cap=5)
    banded = ec.expected(inputs[W], W, banded=True, band_width=128, cap=5)
    assert full["status"][JUNK_WINDOW] == ec.NODE_LIMIT_STATUS and banded["status"][JUNK_WINDOW] == 0
    assert banded["consensus"][JUNK_WINDOW] and banded["stats"]["backbone_by_status"] == 0
    # w = 500: a band of 128 gives another consensus than one of 256
    narrow = ec.expected(inputs[500], 500, banded=True, band_width=128)
    wide = ec.expected(inputs[500], 500, banded=True, band_width=256)
    assert narrow["status"] == wide["status"] and narrow["consensus"] != wide["consensus"]
    # and the gap score alone changes one at the default scores
    assert ec.expected(inputs[W], W, scores=(8, -6, -6))["consensus"] != ec.expected(inputs[W], W)["consensus"]


def test_reordered_targets_and_no_overlaps(inputs):
    inp = inputs[W]
    plain = ec.expected(inp, W)
    moved = ec.expected(ec.reordered(inp), W)
    assert moved["polished"] == [plain["polished"][i] for i in (3, 0, 2, 1)]
    assert [win["target"] for win in moved["slice_windows"]] == [1] * 6 + [2] * 2 + [3] * 3
    assert moved["status"][JUNK_WINDOW] == ec.NODE_LIMIT_STATUS
    bare = ec.expected(ec.without_overlaps(inp), W)
    assert bare["polished"] == inp[1] and bare["stats"]["backbone_by_rule"] == bare["stats"]["windows"] == 11
    assert bare["stats"]["max_sequence_size"] == 64 and bare["status"] == [None] * 11


def test_print_edit_distances(inputs):
    """Not asserted: what polishing does to each draft, through the model and the oracle."""
    truth, targets = inputs[W][0], inputs[W][1]
    r = ec.expected(inputs[W], W)
    for t in range(2):
        print("target %d, edit distance to the truth: draft %d, polished %d"
              % (t, oracle.edit_distance(targets[t], truth[t]), oracle.edit_distance(r["polished"][t], truth[t])))
