"""Cases of cudapolish's window grouping, shared by the CPU and the GPU tests of
the grouping on the device.  The records are made by hand or from a seed: no
aligner is involved.

A case is a dict of name, target_lengths, query_lengths, overlaps ((query,
target, query_start, query_end, target_start, target_end, strand)), records
(eight-int tuples: overlap, window, q_begin, q_end, t_begin, t_end, flags, 0),
w, cap (max_sequences_per_window), qualities (one Phred + 33 string per query,
or None) and tenths (the threshold in tenths).
"""
import random

from polish_model import BAD_PATH, EMPTY, NOT_ALIGNED, REVERSE


def case(name, target_lengths, query_lengths, overlaps, records, w, cap=100, qualities=None, tenths=100):
    return {"name": name, "target_lengths": list(target_lengths), "query_lengths": list(query_lengths),
            "overlaps": list(overlaps), "records": [tuple(r) + (0,) for r in records], "w": w, "cap": cap,
            "qualities": qualities, "tenths": tenths}


def flags_case():
    """Two targets of 10 and 7 bases, three queries, w = 4: every flag kind, both strands, a
    record with q_end == 0, and a flagged record whose ranges are not zero."""
    overlaps = [(0, 0, 0, 12, 0, 10, "+"), (1, 0, 0, 9, 0, 10, "-"), (2, 1, 0, 6, 0, 7, "+"), (1, 1, 0, 9, 0, 7, "-")]
    records = [(0, 0, 0, 4, 0, 4, 0), (0, 1, 4, 8, 4, 8, 0), (0, 2, 8, 10, 8, 10, 0),
               (1, 0, 5, 9, 0, 4, REVERSE), (1, 1, 0, 0, 0, 0, REVERSE | EMPTY), (1, 2, 0, 2, 8, 10, REVERSE),
               (2, 0, 1, 3, 0, 2, BAD_PATH), (2, 1, 0, 0, 0, 0, EMPTY | BAD_PATH), (2, 1, 0, 0, 4, 4, 0),
               (3, 0, 0, 0, 0, 0, REVERSE | EMPTY | NOT_ALIGNED), (3, 1, 1, 5, 4, 7, REVERSE),
               (2, 0, 2, 6, 1, 4, NOT_ALIGNED), (2, 0, 2, 6, 1, 4, 0)]
    return case("flags", [10, 7], [12, 9, 6], overlaps, records, 4)


def two_percent_case():
    """w = 100: a query range of 1 base is left out (50 < 100), one of 2 bases kept."""
    return case("two percent", [250], [50], [(0, 0, 0, 50, 0, 250, "+")],
                [(0, 0, 5, 6, 10, 11, 0), (0, 1, 5, 7, 100, 102, 0), (0, 2, 9, 10, 249, 250, 0)], 100)


def cap_case(cap):
    """Four windows with cap - 2, cap - 1, cap and cap + 1 records that count."""
    records = []
    for k in range(4):
        for j in range(max(cap - 2 + k, 0)):
            records.append((0, k, 10 * k + j, 10 * k + j + 3, 4 * k, 4 * k + 3, 0))
    return case("cap %d" % cap, [16], [64], [(0, 0, 0, 64, 0, 16, "+")], records, 4, cap)


def interleaved_case():
    """130 records of window 1 at cap 100 (31 dropped), in the input between those of windows 0
    and 2: only a stable order by window gives the host's slices."""
    records, j = [], 0
    for step in range(130):
        for k in (0, 1, 2):
            if k == 1 or step % 3 == k // 2:
                records.append((k % 2, k, j, j + 2 + j % 3, 4 * k + j % 2, 4 * k + 3, REVERSE if k % 2 else 0))
                j += 1
    overlaps = [(0, 0, 0, 1000, 0, 12, "+"), (1, 0, 0, 1000, 0, 12, "-")]
    return case("interleaved, 130 at cap 100", [12], [1000, 1000], overlaps, records, 4, 100)


QUALITY_LENGTHS = list(range(1, 10)) + [63, 64, 65, 255, 256, 257, 5000]


def seeded_qualities(rng, lengths, low=2, high=40):
    return ["".join(chr(33 + rng.randint(low, high)) for _ in range(n)) for n in lengths]


def quality_alignment_case(tenths=200, with_qualities=True):
    """w = 1, one record per window: query ranges that begin at each of the four byte offsets
    within a word of the packed quality array, of every length in QUALITY_LENGTHS, and the
    padded edges: the first base of the first read, the last base of the last one, each read
    whole.  Qualities 2..40 against a threshold of 20: some go, some stay."""
    rng = random.Random(77)
    query_lengths = [5003, 701, 302]  # the reads begin at 0, 5003 (3 mod 4) and 5704 (0 mod 4)
    starts = [0, 5003, 5704]
    ranges = []
    for q, (start, size) in enumerate(zip(starts, query_lengths)):
        for offset in range(4):
            for length in QUALITY_LENGTHS:
                begin = (offset - start) % 4 + 4 * rng.randint(0, 2)
                if begin + length <= size:
                    ranges.append((q, begin, begin + length))
    ranges += [(0, 0, 1), (2, 301, 302), (0, 0, 5003), (1, 0, 701), (2, 0, 302), (2, 299, 302), (0, 2, 5002)]
    assert {(starts[q] + b) % 4 for q, b, _ in ranges} == {0, 1, 2, 3}
    overlaps = [(q, 0, 0, n, 0, len(ranges), "+-"[q % 2]) for q, n in enumerate(query_lengths)]
    records = [(q, k, b, e, k, k + 1, REVERSE if q % 2 else 0) for k, (q, b, e) in enumerate(ranges)]
    qualities = seeded_qualities(rng, query_lengths) if with_qualities else None
    name = "quality alignment, threshold %d" % tenths if with_qualities else "no qualities"
    return case(name, [len(ranges)], query_lengths, overlaps, records, 1, 100, qualities, tenths)


def quality_equal_case():
    """All characters '+' (10) against 10.0: kept.  The same with one character lowered: dropped."""
    qualities = ["+" * 64, "+" * 40 + "*" + "+" * 23, "+" * 5000, "+" * 4999 + "*"]
    overlaps = [(q, 0, 0, len(s), 0, 4, "+") for q, s in enumerate(qualities)]
    records = [(q, q, 0, len(s), q, q + 1, 0) for q, s in enumerate(qualities)]
    records += [(1, 1, 0, 40, 1, 2, 0), (1, 1, 41, 64, 1, 2, 0), (1, 1, 40, 41, 1, 2, 0)]
    return case("mean equal to the threshold", [4], [len(s) for s in qualities], overlaps, records, 1, 100,
                qualities, 100)


def filter_before_cap_case():
    """cap 4: the window's first three records fail the quality test and its next three pass.
    A filter applied after the cap would keep none of the three that pass."""
    qualities = ["#" * 30 + "I" * 30]  # 2 and 40
    records = [(0, 0, 5 * j, 5 * j + 5, 0, 5, 0) for j in range(3)] + \
              [(0, 0, 30 + 5 * j, 35 + 5 * j, 0, 5, 0) for j in range(3)]
    return case("filter before cap", [5], [60], [(0, 0, 0, 60, 0, 5, "+")], records, 5, 4, qualities, 100)


def size_cases():
    overlaps = [(0, 0, 0, 40, 0, 9, "+"), (0, 2, 0, 40, 0, 6, "-")]
    some = [(0, 0, 0, 3, 0, 3, 0), (1, 1, 4, 9, 4, 6, REVERSE), (0, 2, 7, 9, 8, 9, 0)]
    rng = random.Random(5)
    wide = [(0, k, k % 30, k % 30 + 4, 4 * k, 4 * k + 4, 0) for k in sorted(rng.sample(range(300), 30))]
    return [case("no segment", [9, 6], [40], overlaps[:1], [], 4),
            case("no target", [], [40], [], [], 4),
            case("no target and no query", [], [], [], [], 4),
            case("empty target between two", [9, 0, 6], [40], overlaps, some, 4),
            case("300 windows", [1200], [40], [(0, 0, 0, 40, 0, 1200, "+")], wide, 4),
            case("single segment", [9], [40], overlaps[:1], some[:1], 4)]


def seeded_case():
    """2,000 records over 3 targets and 5 queries, w = 16, cap 8, qualities 2..40, threshold 20."""
    rng = random.Random(2000)
    target_lengths, query_lengths, w = [400, 250, 333], [900, 1200, 700, 1000, 801], 16
    overlaps = []
    for _ in range(40):
        q, t = rng.randrange(5), rng.randrange(3)
        overlaps.append((q, t, 0, query_lengths[q], 0, target_lengths[t], rng.choice("+-")))
    records = []
    while len(records) < 2000:
        i = rng.randrange(len(overlaps))
        q, t = overlaps[i][0], overlaps[i][1]
        k = rng.randrange((target_lengths[t] + w - 1) // w)
        kind = rng.random()
        reverse = REVERSE if overlaps[i][6] == "-" else 0
        if kind < 0.08:
            records.append((i, k, 0, 0, 0, 0, reverse | EMPTY | rng.choice((0, BAD_PATH, NOT_ALIGNED))))
            continue
        length = rng.choice((0, 1, rng.randint(1, 24)))
        begin = rng.randint(0, query_lengths[q] - length)
        t_begin = k * w + rng.randint(0, 3)
        t_end = min(k * w + rng.randint(8, 16), target_lengths[t])
        records.append((i, k, begin, begin + length, min(t_begin, t_end), t_end, reverse))
    return case("seeded", target_lengths, query_lengths, overlaps, records, w, 8,
                seeded_qualities(rng, query_lengths), 200)


def all_cases():
    cases = [flags_case(), two_percent_case()] + [cap_case(c) for c in (1, 2, 5)] + [interleaved_case()]
    cases += [quality_alignment_case(200), quality_alignment_case(0), quality_alignment_case(200, False),
              quality_equal_case(), filter_before_cap_case()]
    cases += size_cases() + [seeded_case()]
    assert len({c["name"] for c in cases}) == len(cases)
    return cases


def model_view(c):
    """(windows, dropped_by_cap, dropped_by_quality) of the Python model."""
    import polish_resident_model as rm
    return rm.build_window_slices(c["target_lengths"], c["query_lengths"], c["overlaps"], c["records"], c["w"],
                                  c["cap"], c["qualities"], c["tenths"])


def segment_array(c):
    import numpy as np

    from claragenomicsanalysis_amd.cudapolish import SEGMENT_DTYPE
    return np.array(c["records"], dtype=SEGMENT_DTYPE)


def host_slices(cudapolish, c):
    """(windows, dropped_by_cap, dropped_by_quality) of the host's build_window_slices."""
    return cudapolish.build_window_slices(c["target_lengths"], c["query_lengths"], c["overlaps"], segment_array(c),
                                          c["w"], c["cap"], query_qualities=c["qualities"],
                                          quality_threshold=c["tenths"] / 10.0)


def query_texts(c):
    """Bases for the queries, which the grouping never reads: DeviceReads wants some."""
    return ["ACGT" * (n // 4) + "ACGT"[:n % 4] for n in c["query_lengths"]]


# What build_window_slices_device must refuse before any device call: (name, keyword changes to a
# valid call of the flags case, or a record that replaces its first one)
def refused_calls():
    base = flags_case()
    calls = [("window_length 0", {"w": 0}, None), ("window_length -4", {"w": -4}, None),
             ("cap 0", {"cap": 0}, None), ("negative threshold", {"tenths": -1}, None),
             ("overlap index", {}, (4, 0, 0, 4, 0, 4, 0, 0)),
             ("window beyond the target", {}, (0, 3, 0, 4, 0, 4, 0, 0)),
             ("query range beyond the read", {}, (0, 0, 9, 13, 0, 4, 0, 0)),
             ("query range turned round", {}, (0, 0, 5, 4, 0, 4, 0, 0))]
    out = []
    for name, changes, record in calls:
        c = dict(base, **changes)
        if record is not None:
            c["records"] = [record] + base["records"][1:]
        out.append((name, c))
    # a read id beyond the reads: the overlap names query 3 of 3
    c = dict(base)
    c["overlaps"] = [(3, 0, 0, 12, 0, 10, "+")] + base["overlaps"][1:]
    out.append(("read id", c))
    return out
