"""Hand-worked cases of the window cut, shared by the model, C ABI and GPU tests
of cudapolish.  Window length 4.  States: M = 0 match, X = 1 mismatch, I = 2
insertion (target only), D = 3 deletion (query only).

A case is (name, (query_start, query_end, target_start, target_end), path,
forward windows, reverse windows); a window is (k, q_begin, q_end, t_begin,
t_end), or (k,) for an empty one.  The Reverse mirror has the same overlap and
path with strand '-': state u sits at target position target_end - 1 - u.
"""
from polish_model import BAD_PATH, EMPTY, REVERSE

W = 4
M, X, I, D = 0, 1, 2, 3

HAND = [
    # t 0123|4567, q the same
    ("boundary inside a match run", (0, 8, 0, 8), [M] * 8,
     [(0, 0, 4, 0, 4), (1, 4, 8, 4, 8)],
     # u = 0..3 sit at t = 7..4 with q = 0..3, u = 4..7 at t = 3..0 with q = 4..7
     [(0, 4, 8, 0, 4), (1, 0, 4, 4, 8)]),
    # q 4 and 5 are deleted between t = 3 and t = 4: they belong to neither window
    ("boundary inside a deletion run", (0, 10, 0, 8), [M, M, M, X, D, D, M, M, M, M],
     [(0, 0, 4, 0, 4), (1, 6, 10, 4, 8)],
     [(0, 6, 10, 0, 4), (1, 0, 4, 4, 8)]),
    # t 3 and 4 are inserted: window 0 ends at t = 2, window 1 begins at t = 5
    ("boundary inside an insertion run", (0, 6, 0, 8), [M, M, M, I, I, M, X, M],
     [(0, 0, 3, 0, 3), (1, 3, 6, 5, 8)],
     # t = 7, 6, 5 with q = 0, 1, 2; t = 4, 3 inserted; t = 2, 1, 0 with q = 3, 4, 5
     [(0, 3, 6, 0, 3), (1, 0, 3, 5, 8)]),
    ("window covered only by insertion states", (0, 8, 0, 12), [M] * 4 + [I] * 4 + [M] * 4,
     [(0, 0, 4, 0, 4), (1,), (2, 4, 8, 8, 12)],
     [(0, 4, 8, 0, 4), (1,), (2, 0, 4, 8, 12)]),
    # D(q0) I(t0) M(t1,q1) M(t2,q2) M(t3,q3) M(t4,q4) I(t5) D(q5)
    ("path begins and ends with gaps", (0, 6, 0, 6), [D, I, M, M, M, M, I, D],
     [(0, 1, 4, 1, 4), (1, 4, 5, 4, 5)],
     # D(q0) I(t5) M(t4,q1) M(t3,q2) M(t2,q3) M(t1,q4) I(t0) D(q5)
     [(0, 2, 5, 1, 4), (1, 1, 2, 4, 5)]),
    # t = 2..8 with q = 10..16
    ("target_start not a multiple of w", (10, 17, 2, 9), [M] * 7,
     [(0, 10, 12, 2, 4), (1, 12, 16, 4, 8), (2, 16, 17, 8, 9)],
     # t = 8 with q = 10; t = 7..4 with q = 11..14; t = 3, 2 with q = 15, 16
     [(0, 15, 17, 2, 4), (1, 11, 15, 4, 8), (2, 10, 11, 8, 9)]),
    ("target_end a multiple of w", (0, 4, 4, 8), [M, X, X, M],
     [(1, 0, 4, 4, 8)],
     [(1, 0, 4, 4, 8)]),
    # M(t5,q3) D(q4) M(t6,q5)
    ("overlap inside one window", (3, 6, 5, 7), [M, D, M],
     [(1, 3, 6, 5, 7)],
     [(1, 3, 6, 5, 7)]),
]

# paths that do not fit the overlap (0, 8, 0, 8), which owns windows 0 and 1
MISFITS = [
    ("too long", [M] * 9),
    ("too short", [M] * 7),
    ("state 7", [M, M, M, 7, M, M, M, M]),
]
MISFIT_SPANS = (0, 8, 0, 8)


def overlap_of(spans, strand, query_id=0, target_id=0):
    qs, qe, ts, te = spans
    return (query_id, target_id, qs, qe, ts, te, strand)


def records_of(index, windows, reverse):
    """The expected eight-word records of one case."""
    flag = REVERSE if reverse else 0
    return [(index, w[0], 0, 0, 0, 0, flag | EMPTY, 0) if len(w) == 1 else (index,) + tuple(w) + (flag, 0)
            for w in windows]


def misfit_records(index, reverse):
    flag = (REVERSE if reverse else 0) | EMPTY | BAD_PATH
    return [(index, 0, 0, 0, 0, 0, flag, 0), (index, 1, 0, 0, 0, 0, flag, 0)]


def hand_cases():
    """(id, overlap, path, expected records for index 0), forward then Reverse mirror of each."""
    out = []
    for name, spans, path, forward, reverse in HAND:
        out.append((name, overlap_of(spans, "+"), path, records_of(0, forward, False)))
        out.append((name + ", reverse", overlap_of(spans, "-"), path, records_of(0, reverse, True)))
    for name, path in MISFITS:
        out.append((name, overlap_of(MISFIT_SPANS, "+"), path, misfit_records(0, False)))
        out.append((name + ", reverse", overlap_of(MISFIT_SPANS, "-"), path, misfit_records(0, True)))
    return out


def as_tuples(segments):
    """A SEGMENT_DTYPE array as a list of eight-int tuples."""
    return [tuple(int(x) for x in row) for row in segments.tolist()]


def random_path(rng, target_length, query_length, diagonal=None):
    """A path that fits: the gaps are spread at random among the diagonal steps."""
    if diagonal is None:
        diagonal = rng.randint(0, min(target_length, query_length))
    states = [rng.choice((0, 1)) for _ in range(diagonal)] + [2] * (target_length - diagonal) + \
        [3] * (query_length - diagonal)
    if rng.random() < 0.5:
        rng.shuffle(states)
    else:  # gaps in runs, as an aligner leaves them
        runs = [[s] for s in states[:diagonal]] + [[2] * (target_length - diagonal), [3] * (query_length - diagonal)]
        rng.shuffle(runs)
        states = [s for run in runs for s in run]
    return states


# ---- end to end: a draft and noisy reads of one truth ---------------------------------------------------

E2E_SEED = 1  # through the oracle alone: the draft 42 edits from the truth, the polished sequence 0
E2E_W = 200


def mutate(rng, seq, rate):
    """seq with `rate` errors per base: a third each substitutions, deletions and insertions."""
    out = []
    for c in seq:
        if rng.random() < rate:
            kind = rng.randrange(3)
            if kind == 0:
                out.append(rng.choice([b for b in "ACGT" if b != c]))
            elif kind == 2:
                out.append(c)
                out.append(rng.choice("ACGT"))
        else:
            out.append(c)
    return "".join(out)


def e2e_input(seed=E2E_SEED, length=1200, reads=12, draft_rate=0.04, read_rate=0.10):
    """(truth, draft, reads, overlaps): every read is the whole truth with errors, every second one
    reverse-complemented, and overlaps the whole draft."""
    import random

    from polish_model import reverse_complement
    rng = random.Random(seed)
    truth = "".join(rng.choice("ACGT") for _ in range(length))
    draft = mutate(rng, truth, draft_rate)
    queries, overlaps = [], []
    for i in range(reads):
        read = mutate(rng, truth, read_rate)
        if i % 2:
            read = reverse_complement(read)
        queries.append(read)
        overlaps.append((i, 0, 0, len(read), 0, len(draft), "-" if i % 2 else "+"))
    return truth, draft, queries, overlaps


def oracle_paths(oracle, queries, targets, overlaps):
    """oracle.align of every overlap's regions, the target's reverse-complemented for '-'."""
    from polish_model import reverse_complement
    paths = []
    for q, t, qs, qe, ts, te, strand in overlaps:
        region = targets[t][ts:te]
        paths.append(oracle.align(queries[q][qs:qe], reverse_complement(region) if strand == "-" else region))
    return paths


def build_cpp_check(tmp_path):
    """tests/polish_cpp_check.cpp compiled against the built library; returns the program's path."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "claragenomicsanalysis_amd", "lib")
    exe = str(tmp_path / "polish_cpp_check")
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-std=c++17", "-O1", "-Wall",
                           "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(root, "include"), "-I", "/opt/rocm/include",
                           "-x", "c++", os.path.join(root, "tests", "polish_cpp_check.cpp"), "-L", lib, "-lgwamd",
                           "-Wl,-rpath," + lib, "-o", exe])
    return exe


CPP_HOST = ["group_sizes", "group_sequences", "group_metadata", "window_length_refused", "no_overlaps_no_device_call"]
CPP_GPU = ["host_paths", "resident_reads"]
