"""Plain-Python model of cudapolish: the cut of aligned overlaps into target
windows (racon's find_breaking_points on AlignmentState paths), the grouping
of the pieces into POA windows and the stitching of the consensus.

Path states are AlignmentState values, start -> end: 0 match and 1 mismatch
advance both sequences, 3 (deletion) advances only the query, 2 (insertion)
only the target (alignment_impl.cpp:94-103; the opposite of SAM's I / D).

An overlap is (query_id, target_id, query_start, query_end, target_start,
target_end, strand), the argument order of cudamapper.Overlap.  A record is
the tuple of the eight words of gwamd_window_segment:
(overlap, window, q_begin, q_end, t_begin, t_end, flags, 0).
"""

REVERSE, EMPTY, BAD_PATH, NOT_ALIGNED = 1, 2, 4, 8

_COMPLEMENT = {"A": "T", "T": "A", "C": "G", "G": "C"}


def window_count(ts, te, w):
    """Records overlap target[ts, te) owns: windows ts // w .. (te - 1) // w."""
    return 0 if te == ts else (te - 1) // w - ts // w + 1


def path_fits(states, query_length, target_length):
    """Whether the states are all 0..3 and advance the query by exactly
    query_length and the target by exactly target_length."""
    u = v = 0
    for s in states:
        if s not in (0, 1, 2, 3):
            return False
        u += s != 3
        v += s != 2
        if u > target_length or v > query_length:
            return False
    return u == target_length and v == query_length


def segments(index, overlap, states, w, aligned=True):
    """The records of one overlap, windows ascending."""
    _, _, qs, qe, ts, te, strand = overlap
    reverse = strand in ("-", ord("-"), b"-")
    base = REVERSE if reverse else 0
    k0 = ts // w
    count = window_count(ts, te, w)
    if not aligned:
        return [(index, k0 + j, 0, 0, 0, 0, base | EMPTY | NOT_ALIGNED, 0) for j in range(count)]
    if not path_fits(states, qe - qs, te - ts):
        return [(index, k0 + j, 0, 0, 0, 0, base | EMPTY | BAD_PATH, 0) for j in range(count)]
    seen = {}
    u = v = 0
    for s in states:
        if s in (0, 1):
            t = te - 1 - u if reverse else ts + u
            q = qs + v
            seen.setdefault(t // w, []).append((q, t))
        u += s != 3
        v += s != 2
    out = []
    for k in range(k0, k0 + count):
        if k not in seen:
            out.append((index, k, 0, 0, 0, 0, base | EMPTY, 0))
            continue
        qq = [p[0] for p in seen[k]]
        tt = [p[1] for p in seen[k]]
        out.append((index, k, min(qq), max(qq) + 1, min(tt), max(tt) + 1, base, 0))
    return out


def window_segments(overlaps, paths, w, aligned=None):
    """The records of every overlap, in input order."""
    out = []
    for i, (o, p) in enumerate(zip(overlaps, paths)):
        out += segments(i, o, p, w, True if aligned is None else aligned[i])
    return out


def reverse_complement(seq):
    """The aligner's rule: A<->T, C<->G, every other letter kept, every position complemented."""
    return "".join(_COMPLEMENT.get(c, c) for c in reversed(seq))


def build_windows(targets, queries, overlaps, records, w, max_sequences_per_window=100):
    """(windows, dropped): one window per w bases of every target, in target
    then window order, each a dict of target, window, sequences (backbone
    first) and per sequence its overlap (-1: backbone) and t_begin, t_end
    relative to the window's first base; dropped counts the pieces the cap
    left out."""
    windows, first = [], []
    for r, t in enumerate(targets):
        first.append(len(windows))
        for k in range((len(t) + w - 1) // w):
            backbone = t[k * w:min((k + 1) * w, len(t))]
            windows.append({"target": r, "window": k, "sequences": [backbone], "overlap": [-1],
                            "t_begin": [0], "t_end": [len(backbone)]})
    dropped = 0
    for rec in records:
        i, k, qb, qe, tb, te, flags, _ = rec
        if flags & (EMPTY | BAD_PATH | NOT_ALIGNED) or (qe - qb) * 50 < w:
            continue
        o = overlaps[i]
        win = windows[first[o[1]] + k]
        if len(win["sequences"]) >= max_sequences_per_window:
            dropped += 1
            continue
        piece = queries[o[0]][qb:qe]
        win["sequences"].append(reverse_complement(piece) if flags & REVERSE else piece)
        win["overlap"].append(i)
        win["t_begin"].append(tb - k * w)
        win["t_end"].append(te - k * w)
    return windows, dropped


def polish(targets, windows, consensus):
    """consensus(window) -> (status, text); windows of fewer than three
    sequences and those whose status is not 0 keep their backbone."""
    out = ["" for _ in targets]
    stats = {"windows": len(windows), "backbone_by_rule": 0, "backbone_by_status": 0}
    for win in windows:
        text = win["sequences"][0]
        if len(win["sequences"]) < 3:
            stats["backbone_by_rule"] += 1
        else:
            status, cons = consensus(win)
            if status == 0:
                text = cons
            else:
                stats["backbone_by_status"] += 1
        out[win["target"]] += text
    return out, stats
