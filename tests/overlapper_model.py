"""Plain-Python model of cudamapper's overlapper (reference
cudamapper/src/overlapper_triggered.cu and overlapper.cpp), written from the
semantics alone: every comparison is between an element and its left
neighbour, float32 quotients go through numpy.

An anchor is (query_read_id, target_read_id, query_position_in_read,
target_position_in_read); an overlap is the argument tuple of
claragenomicsanalysis_amd.cudamapper.Overlap: (query_read_id, target_read_id,
query_start, query_end, target_start, target_end, strand, num_residues,
overlap_complete)."""
import numpy as np

CHAIN_REACH = 150
FUSE_REACH = 300
CHAIN_TAIL = 3
F32 = np.float32
U32 = 0xFFFFFFFF


def _i32(v):
    v &= U32
    return v - (1 << 32) if v >> 31 else v


def _div32(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        return F32(a) / F32(b)


def same_chain(a, b):
    """a is the left neighbour of b."""
    return a[0] == b[0] and a[1] == b[1] and ((b[2] - a[2]) & U32) < CHAIN_REACH and abs(b[3] - a[3]) < CHAIN_REACH


def same_group(a, b):
    return a[0] == b[0] and a[1] == b[1] and abs(abs(a[2] - b[2]) - abs(a[3] - b[3])) < FUSE_REACH


def passes_filter(o, min_residues, min_overlap_len, min_bases_per_residue, min_overlap_fraction):
    q, t, qs, qe, ts, te, _, residues, _ = o
    tl, ql = (te - ts) & U32, (qe - qs) & U32
    ol = max(tl, ql)
    fraction = F32(min_overlap_fraction)
    return bool(residues >= min_residues and ol // residues < min_bases_per_residue and
                ql >= min_overlap_len and tl >= min_overlap_len and q != t and
                _div32(tl, ol) > fraction and _div32(ql, ol) > fraction)


def get_overlaps(anchors, min_residues=20, min_overlap_len=50, min_bases_per_residue=50, min_overlap_fraction=0.9):
    """(overlaps, counts): counts has the number of chains, kept chains, groups
    and overlaps.  ValueError for unsorted anchors or a position >= 2^31."""
    anchors = [tuple(int(x) for x in a) for a in anchors]
    for i, a in enumerate(anchors):
        if a[2] >> 31 or a[3] >> 31:
            raise ValueError("position of 2^31 or more")
        if i and anchors[i - 1] > a:
            raise ValueError("anchors are not sorted")
    n = len(anchors)
    starts = [i for i in range(n) if i == 0 or not same_chain(anchors[i - 1], anchors[i])]
    chains = [(s, (starts[c + 1] if c + 1 < len(starts) else n) - s) for c, s in enumerate(starts)]
    kept = [(s, length) for s, length in chains if length >= CHAIN_TAIL]
    groups = []  # [first anchor, past the last anchor, residues]
    for k, (s, length) in enumerate(kept):
        if k and same_group(anchors[kept[k - 1][0]], anchors[s]):
            groups[-1][1] = s + length
            groups[-1][2] += length
        else:
            groups.append([s, s + length, length])
    overlaps = []
    for first, past, residues in groups:
        s, e = anchors[first], anchors[past - 1]
        ts, te, strand = s[3], e[3], "+"
        if ts > te:
            ts, te, strand = te, ts, "-"
        o = (e[0], e[1], s[2], e[2], ts, te, strand, residues, True)
        if passes_filter(o, min_residues, min_overlap_len, min_bases_per_residue, min_overlap_fraction):
            overlaps.append(o)
    return overlaps, dict(chains=len(chains), kept=len(kept), groups=len(groups), overlaps=len(overlaps))


def mergeable(a, b):
    """Whether overlap b can be fused to its predecessor a."""
    if not (a[6] == b[6] and a[6] in ("+", "-")):
        return False
    if a[0] != b[0] or a[1] != b[1]:
        return False
    query_gap = abs(_i32(b[2] - a[3]))
    target_gap = abs(_i32(a[4] - b[5])) if a[6] == "-" else abs(_i32(b[4] - a[5]))
    if query_gap < 500 and target_gap < 500:
        return True
    # float32 quotients compared with double constants
    if float(_div32(min(query_gap, target_gap), max(query_gap, target_gap))) > 0.8:
        return True
    query_length = ((a[3] - a[2]) + (b[3] - b[2])) & U32
    target_length = ((a[5] - a[4]) + (b[5] - b[4])) & U32
    return bool(float(_div32(query_gap, query_length)) < 0.2 and float(_div32(target_gap, target_length)) < 0.2)


def post_process_overlaps(overlaps, drop_fused_overlaps=False):
    overlaps = [tuple(o) for o in overlaps]
    n = len(overlaps)
    fused = [False] * n
    added = []
    in_fuse = False
    base = span = None

    def close():
        qs, qe, ts, te, residues = span
        added.append((base[0], base[1], qs, qe, ts, te, base[6], residues & U32, base[8]))

    for i in range(1, n):
        prev, cur = overlaps[i - 1], overlaps[i]
        base = prev  # what a fusion closed now takes its other fields from
        if mergeable(prev, cur):
            fused[i] = fused[i - 1] = True
            forward = cur[6] == "+"
            if not in_fuse:
                in_fuse = True
                span = [prev[2], cur[3], prev[4] if forward else cur[4], cur[5] if forward else prev[5],
                        prev[7] + cur[7]]
            else:
                span[4] += cur[7]
                span[1] = cur[3]
                if forward:
                    span[3] = cur[5]
                else:
                    span[2] = cur[4]
        elif in_fuse:
            in_fuse = False
            close()
    if in_fuse:
        close()
    if drop_fused_overlaps:
        overlaps = [o for i, o in enumerate(overlaps) if not fused[i]]
    return overlaps + added
