"""Plain-Python model of cudamapper's overlap-end rescue, quirks included
(reference cudamapper/src/overlapper.cpp:94-109 and 254-365,
cudamapper/src/cudamapper_utils.cpp:114-170).  Sequences are bytes; overlaps
are the tuples of the other models: (query_read_id, target_read_id,
query_start, query_end, target_start, target_end, strand, num_residues,
overlap_complete).  The two float32 values, the quotient and the threshold,
are numpy float32.
"""
from collections import Counter

import numpy as np

KMER = 15            # what extend_overlap_by_sequence_similarity passes (overlapper.cpp:272, 287)
ROUNDS = 3           # max_rescue_rounds (overlapper.cpp:336)
EXTENSION = 100      # what rescue_overlap_ends passes to every round, whatever it is given
SIMILARITY = 0.9     # (overlapper.cpp:345)
COMPLEMENT = "TBGDEFCHIJKLMNOPQRSAUVWXYZ"  # complement_array (overlapper.cpp:94-99)


def as_bytes(s):
    return s.encode("latin-1") if isinstance(s, str) else bytes(s)


def split_into_kmers(s, k=KMER):
    """split_into_kmers(s, k, 1) (cudamapper_utils.cpp:114-130): substr(i, i + k)
    takes i + k as a count, so substring i is s[i : i + i + k], clipped."""
    s = as_bytes(s)
    if len(s) < k:
        return [s]
    return [s[i:i + i + k] for i in range(len(s) - k + 1)]


def shared_and_union(a, b, k=KMER):
    ka, kb = Counter(split_into_kmers(a, k)), Counter(split_into_kmers(b, k))
    shared = sum((ka & kb).values())
    return shared, sum(ka.values()) + sum(kb.values()) - shared


def similarity(a, b, k=KMER):
    """sequence_jaccard_similarity(a, b, k, 1) as a float32."""
    shared, union = shared_and_union(a, b, k)
    return np.float32(shared) / np.float32(union)


def accepted(a, b, required_similarity, k=KMER):
    return bool(similarity(a, b, k) >= np.float32(required_similarity))


def extend(qs, qe, ts, te, query, target, extension, required_similarity):
    """One round (overlapper.cpp:254-293); returns the positions and whether the head and the tail were accepted."""
    h = min(qs, ts, extension)
    head = accepted(query[qs - h:qs], target[ts - h:ts], required_similarity)
    if head:
        qs, ts = qs - h, ts - h
    t = min(extension, len(query) - qe, len(target) - te)
    tail = accepted(query[qe:qe + t], target[te:te + t], required_similarity)
    if tail:
        qe, te = qe + t, te + t
    return qs, qe, ts, te, head, tail


def extend_overlap_by_sequence_similarity(overlap, query, target, extension, required_similarity):
    q, t, qs, qe, ts, te, *rest = overlap
    qs, qe, ts, te, _, _ = extend(qs, qe, ts, te, as_bytes(query), as_bytes(target), extension, required_similarity)
    return (q, t, qs, qe, ts, te, *rest)


def reverse_complement(s):
    """reverse_complement (overlapper.cpp:101-109): the loop stops at len / 2, so
    the middle base of an odd length stays as it is; a byte outside 'A'..'Z'
    (undefined in the reference) is kept."""
    s = as_bytes(s)
    out = bytearray(reversed(s))
    for i, c in enumerate(out):
        if 65 <= c <= 90 and not (len(s) % 2 and i == len(s) // 2):
            out[i] = ord(COMPLEMENT[c - 65])
    return bytes(out)


def rescue_one(overlap, query, target, extension=EXTENSION, required_similarity=SIMILARITY, rounds=ROUNDS):
    """The overlap after the rounds, and per end the bases gained in each round."""
    q, t, qs, qe, ts, te, strand, *rest = overlap
    query, target = as_bytes(query), as_bytes(target)
    if strand == "-":
        target = reverse_complement(target)
        ts, te = len(target) - te, len(target) - ts
    head_steps, tail_steps = [], []
    for _ in range(rounds):
        before = (qs, qe)
        qs, qe, ts, te, _, _ = extend(qs, qe, ts, te, query, target, extension, required_similarity)
        head_steps.append(before[0] - qs)
        tail_steps.append(qe - before[1])
    if strand == "-":
        ts, te = len(target) - te, len(target) - ts
    return (q, t, qs, qe, ts, te, strand, *rest), head_steps, tail_steps


def rescue_overlap_ends(overlaps, query_reads, target_reads, extension=EXTENSION, required_similarity=SIMILARITY):
    """Overlapper::rescue_overlap_ends with the two numbers honoured (the reference's own
    entry point corresponds to the defaults)."""
    return [rescue_one(o, query_reads[o[0]], target_reads[o[1]], extension, required_similarity)[0]
            for o in overlaps]
