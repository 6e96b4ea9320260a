"""Plain-Python model of cudapolish's resident route: a slice of a read as the
bytes and weights the POA batch must hold for it, the grouping of window
segments into slices with racon's mean-quality filter, and racon's coverage
trimming of a consensus.

A slice is (set, read, begin, end, flags): bases [begin, end) of read `read` of
sets[set], reverse-complemented when flags & 1.  sets is a list of read lists
(str), qualities a list of the same shape whose entries are None for a set
without qualities.
"""
from polish_model import BAD_PATH, EMPTY, NOT_ALIGNED, REVERSE, reverse_complement

SLICE_REVERSE = 1
PAD = 16  # zero bytes the batch keeps after its last base


def slice_bases(sets, sl):
    s, r, b, e, flags = sl
    text = sets[s][r][b:e]
    return reverse_complement(text) if flags & SLICE_REVERSE else text


def slice_weights(qualities, sl):
    """quality - 33 per base, turned round (not complemented) with the bases; 1 without qualities."""
    s, r, b, e, flags = sl
    if qualities[s] is None:
        return [1] * (e - b)
    w = [ord(c) - 33 for c in qualities[s][r][b:e]]
    return w[::-1] if flags & SLICE_REVERSE else w


def packed_inputs(sequences):
    """(bases, weights) of a batch: sequences is a list of (text, weights) in the
    order added, packed back to back, PAD zero bytes after the last."""
    bases = b"".join(t.encode("latin-1") for t, _ in sequences) + bytes(PAD)
    weights = bytes(x for _, w in sequences for x in w) + bytes(PAD)
    return bases, weights


def mean_quality_below(quality, begin, end, threshold_tenths):
    """racon's rule in integers: mean(quality - 33) over [begin, end) < threshold_tenths / 10."""
    return 10 * sum(ord(c) - 33 for c in quality[begin:end]) < threshold_tenths * (end - begin)


def build_window_slices(target_lengths, query_lengths, overlaps, records, w, max_sequences_per_window=100,
                        query_qualities=None, threshold_tenths=100):
    """(windows, dropped_by_cap, dropped_by_quality).  A window is a dict of
    target, window, slices (backbone first: set 0; segments: set 1), overlap,
    t_begin, t_end.  The quality filter runs after the keep rule and before the
    cap."""
    windows, first = [], []
    for r, length in enumerate(target_lengths):
        first.append(len(windows))
        for k in range((length + w - 1) // w):
            end = min((k + 1) * w, length)
            windows.append({"target": r, "window": k, "slices": [(0, r, k * w, end, 0)], "overlap": [-1],
                            "t_begin": [0], "t_end": [end - k * w]})
    by_cap = by_quality = 0
    for i, k, qb, qe, tb, te, flags, _ in records:
        if flags & (EMPTY | BAD_PATH | NOT_ALIGNED) or (qe - qb) * 50 < w:
            continue
        o = overlaps[i]
        if query_qualities is not None and mean_quality_below(query_qualities[o[0]], qb, qe, threshold_tenths):
            by_quality += 1
            continue
        win = windows[first[o[1]] + k]
        if len(win["slices"]) >= max_sequences_per_window:
            by_cap += 1
            continue
        win["slices"].append((1, o[0], qb, qe, SLICE_REVERSE if flags & REVERSE else 0))
        win["overlap"].append(i)
        win["t_begin"].append(tb - k * w)
        win["t_end"].append(te - k * w)
    return windows, by_cap, by_quality


def trim_consensus(consensus, coverage, num_sequences):
    """racon, window.cpp: from the first to the last index whose coverage reaches
    (num_sequences - 1) // 2, both included; whole when there is none or only one."""
    average = (num_sequences - 1) // 2
    good = [i for i, c in enumerate(coverage) if c >= average]
    if not good or good[0] >= good[-1]:
        return consensus
    return consensus[good[0]:good[-1] + 1]
