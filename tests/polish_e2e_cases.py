"""A harder input for cudapolish.polish() than polish_cases.e2e_input(), and the
result the model and the oracle give for it: four targets (two with reads, one
that no overlap names, one empty), reads that cover a part of their target,
reads that share no letter with anything (every base a new node, so their window
runs out of nodes), windows of fewer than three sequences between windows that
go to the POA, and qualities that the mean-quality filter separates.

expected() restates polish() through polish_model, polish_resident_model and the
oracle alone; nothing here touches the library under test.
"""
import random

import numpy as np

import polish_cases as pc
import polish_model as pm
import polish_resident_model as rm
from oracle import oracle

SEED = 3
JUNK_LETTERS = "BDEFHIJKLMOPQRSUVWXYZ"  # no A, C, G, T (and no N): three letters per junk read
JUNK_READS = 5
DEFAULT_SCORES = (8, -6, -8)  # polish()'s default: match, mismatch, gap
NODE_LIMIT_STATUS = 4  # node_count_exceeded_maximum_graph_size


def _random_bases(rng, n, letters="ACGT"):
    return "".join(rng.choice(letters) for _ in range(n))


def _quality(rng, n, lo, hi):
    return "".join(chr(33 + rng.randint(lo, hi)) for _ in range(n))


def hard_input(w, seed=SEED):
    """(truth, targets, queries, overlaps, query_qualities, target_qualities).

    Targets: drafts (4 % errors) of truths of 1,130 and 450 bases, 260 random bases that no overlap
    names, and the empty string.  On target 0: five junk reads of about w letters against [w, 2w),
    first in the list so that a cap of 6 keeps them; eight whole reads at 10 % errors; three reads
    of which [100, len - 150) overlaps [130, 1010).  On target 1: four reads of the truth's first
    300 bases against [0, 290) and one whole read.  A reverse read is stored reverse-complemented
    with its query range mirrored.  Qualities: 2..8 on the junk reads, 12..40 on the others, 5..30
    on the targets."""
    rng = random.Random(seed)
    truth = [_random_bases(rng, 1130), _random_bases(rng, 450)]
    targets = [pc.mutate(rng, t, 0.04) for t in truth] + [_random_bases(rng, 260), ""]
    queries, overlaps = [], []

    def add(read, target, qs, qe, ts, te, reverse):
        n = len(read)
        if reverse:
            read, qs, qe = pm.reverse_complement(read), n - qe, n - qs
        overlaps.append((len(queries), target, qs, qe, ts, te, "-" if reverse else "+"))
        queries.append(read)

    for i in range(JUNK_READS):
        n = rng.randint(w - w // 10, w + w // 10)
        add(_random_bases(rng, n, JUNK_LETTERS[3 * i:3 * i + 3]), 0, 0, n, w, 2 * w, i % 3 == 0)
    for i in range(8):
        read = pc.mutate(rng, truth[0], 0.10)
        add(read, 0, 0, len(read), 0, len(targets[0]), i % 2 == 1)
    for i in range(3):
        read = pc.mutate(rng, truth[0], 0.10)
        add(read, 0, 100, len(read) - 150, 130, 1010, i % 2 == 0)
    for i in range(4):
        read = pc.mutate(rng, truth[1][:300], 0.10)
        add(read, 1, 0, len(read), 0, 290, i % 2 == 0)
    read = pc.mutate(rng, truth[1], 0.10)
    add(read, 1, 0, len(read), 0, len(targets[1]), True)
    query_qualities = [_quality(rng, len(q), 2, 8) if i < JUNK_READS else _quality(rng, len(q), 12, 40)
                       for i, q in enumerate(queries)]
    target_qualities = [_quality(rng, len(t), 5, 30) for t in targets]
    return truth, targets, queries, overlaps, query_qualities, target_qualities


def reordered(inp, order=(3, 0, 2, 1)):
    """The same input with targets[order[j]] at position j and the overlaps renumbered: by default
    the empty target first and the one without overlaps between the two that have reads."""
    truth, targets, queries, overlaps, query_qualities, target_qualities = inp
    new_id = {old: new for new, old in enumerate(order)}
    return (truth, [targets[i] for i in order], queries, [(o[0], new_id[o[1]]) + tuple(o[2:]) for o in overlaps],
            query_qualities, [target_qualities[i] for i in order])


def without_overlaps(inp):
    truth, targets, queries, _, query_qualities, target_qualities = inp
    return truth, targets, queries, [], query_qualities, target_qualities


def max_sequence_size(windows, key):
    """polish's rule: the longest sequence of the windows that go to the POA, plus one, in steps of 64."""
    longest = max([len(s) for win in windows if len(win[key]) >= 3 for s in win["sequences"]] + [1])
    return (longest + 1 + 63) // 64 * 64


def expected(inp, w, *, banded=True, band_width=256, scores=DEFAULT_SCORES, cap=100, qualities=False,
             threshold=10.0, trim=False):
    """What polish(targets, queries, overlaps, window_length=w, ...) must return, as a dict:

    "polished", "stats" (every key polish() returns), "consensus" and "status" per window (None for
    a window of fewer than three sequences), "slice_windows" (the windows of the resident routes,
    with "slices", "sequences" and "weights") and "windows" (those of the default route; None with
    qualities, which the default route does not take), "coverage" per window and "paths"."""
    _, targets, queries, overlaps, query_qualities, target_qualities = inp
    if not qualities:
        query_qualities = target_qualities = None
    paths = pc.oracle_paths(oracle, queries, targets, overlaps)
    records = pm.window_segments(overlaps, paths, w)
    slice_windows, by_cap, by_quality = rm.build_window_slices(
        [len(t) for t in targets], [len(q) for q in queries], overlaps, records, w, cap, query_qualities,
        int(round(10 * threshold)))
    sets, quals = (targets, queries), (target_qualities, query_qualities)
    for win in slice_windows:
        win["sequences"] = [rm.slice_bases(sets, sl) for sl in win["slices"]]
        win["weights"] = [rm.slice_weights(quals, sl) for sl in win["slices"]]
    windows = None
    if not qualities:
        windows, dropped = pm.build_windows(targets, queries, overlaps, records, w, cap)
        assert dropped == by_cap and [x["sequences"] for x in windows] == [x["sequences"] for x in slice_windows]
    size = max_sequence_size(slice_windows, "slices")
    max_nodes = ((4 if banded else 3) * size + 3) // 4 * 4
    consensus, coverage, status = [], [], []
    for win in slice_windows:
        if len(win["sequences"]) < 3:
            consensus.append(None)
            coverage.append(None)
            status.append(None)
            continue
        r = oracle.poa_window(win["sequences"], weights=[np.array(x, np.int8) for x in win["weights"]],
                              match=scores[0], mismatch=scores[1], gap=scores[2], banded=banded,
                              band_width=band_width, max_nodes=max_nodes, max_consensus=2 * size, max_seqs=cap)
        consensus.append(r.consensus)
        coverage.append(r.coverage)
        status.append(r.status)
    # the join: polish_model.polish, with the trimming on the way
    trimmed = [0]

    def text_of(win):
        i = index_of[id(win)]
        text = consensus[i]
        if status[i] == 0 and trim:
            text = rm.trim_consensus(text, coverage[i], len(win["sequences"]))
            trimmed[0] += len(consensus[i]) - len(text)
        return status[i], text

    index_of = {id(win): i for i, win in enumerate(slice_windows)}
    polished, stats = pm.polish(targets, slice_windows, text_of)
    stats.update(dropped_by_cap=by_cap, dropped_by_quality=by_quality, trimmed_bases=trimmed[0],
                 max_sequence_size=size)
    return {"polished": polished, "stats": stats, "consensus": consensus, "status": status, "coverage": coverage,
            "slice_windows": slice_windows, "windows": windows, "paths": paths}
