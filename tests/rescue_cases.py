"""Inputs shared by test_rescue_model.py (CPU) and test_rescue_gpu.py: the
seeded random set of overlaps on substrings of a random genome."""
import random

import rescue_model as model

BASES = b"ACGT"


def random_bases(rng, n):
    return bytes(rng.choice(BASES) for _ in range(n))


def substitute(seq, at, rng):
    return seq[:at] + bytes([rng.choice([c for c in BASES if c != seq[at]])]) + seq[at + 1:]


def plain_reverse_complement(s):
    return s[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))


def random_set(seed=20250311, count=400):
    """count overlaps, each on a query and a target read of its own that share a
    stretch of a random genome between unrelated flanks of 0 to 200 bases.  The
    overlap is that stretch trimmed inwards by up to 260 bases per end (one in
    ten is not trimmed at all); with probability 1/2 per end the query has a
    substitution within 120 bases outside the trimmed end.  Every second target
    is reverse complemented, with the overlap's target positions mirrored."""
    rng = random.Random(seed)
    genome = random_bases(rng, 60000)
    queries, targets, overlaps = [], [], []
    for i in range(count):
        length = rng.randint(700, 1500)
        start = rng.randint(0, len(genome) - length)
        core = genome[start:start + length]
        flank = [rng.choice([0, rng.randint(1, 200)]) for _ in range(4)]
        query = random_bases(rng, flank[0]) + core + random_bases(rng, flank[1])
        target = random_bases(rng, flank[2]) + core + random_bases(rng, flank[3])
        untrimmed = rng.random() < 0.1
        head_trim, tail_trim = (0, 0) if untrimmed else (rng.randint(0, 260), rng.randint(0, 260))
        qs, qe = flank[0] + head_trim, flank[0] + length - tail_trim
        ts, te = flank[2] + head_trim, flank[2] + length - tail_trim
        for end, trim in ((qs, head_trim), (qe, tail_trim)):
            distance = rng.randint(1, 120)
            if rng.random() < 0.5 and distance <= trim:
                query = substitute(query, end - distance if end == qs else end + distance - 1, rng)
        strand = "+"
        if i % 2:
            strand = "-"
            target = plain_reverse_complement(target)
            ts, te = len(target) - te, len(target) - ts
        queries.append(query)
        targets.append(target)
        overlaps.append((i, i, qs, qe, ts, te, strand, rng.randint(0, 99), rng.random() < 0.5))
    return queries, targets, overlaps


def outcomes(queries, targets, overlaps):
    """Per overlap, from the model: (bases gained at the head, at the tail, whether
    some end gained in more than one round)."""
    out = []
    for o in overlaps:
        _, head, tail = model.rescue_one(o, queries[o[0]], targets[o[1]])
        out.append((sum(head), sum(tail), max(sum(1 for s in head if s), sum(1 for s in tail if s)) > 1))
    return out
