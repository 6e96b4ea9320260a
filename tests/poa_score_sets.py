"""Shared by the scoring-parameter tests (test_poa_scores.py on the GPU,
test_poa_scores_cpu.py without one): the score sets, the reference's rules
restated in a few lines of Python, the windows, and the oracle's outputs
(computed once per score set and window set).

Scores are (gap, mismatch, match) throughout, the order of create_batch and the
C ABI; get_multi_batch_sizes / estimate_max_poas take (mismatch, gap, match).
"""
import functools
import random

from claragenomicsanalysis_amd import synth
from oracle import oracle

DEFAULT = (-8, -6, 8)

# name -> (gap, mismatch, match); each named by what it reaches
GENERAL = {
    "asym_a": (-4, -6, 8),        # plain asymmetric values: a swapped argument shows
    "asym_b": (-2, -4, 5),
    "sne_m1": (-8, -9, 8),        # mismatch - gap = -1: just outside fwd2_ok, the pk pass in production
    "mm_eq_gap": (-8, -8, 8),     # s_ne = 0, the byte table's lower edge; diagonal ties with vertical/horizontal
    "mm_eq_2gap": (-8, -16, 8),   # a mismatch ties with two gaps everywhere
    "gap0": (0, -6, 8),           # E domain equals H; s_ne < 0: pk
    "match0": (-8, -6, 0),
    "mismatch0": (-8, 0, 8),
    "unit": (-1, -1, 1),
    "zero": (0, 0, 0),            # every cell ties: tie order alone decides the output
}
# max_sequence_size 128 (3 * 128 = 384 graph rows).  The reference's rule gives
# lower = 128 * max(gap, mismatch) + 256 * gap: with gap -127 that is int16 only
# for mismatch >= -2, so the byte-table edge is run with mismatch -1 (upper
# 16,384 / 16,512, lower -32,640: int16) and, with mismatch -6 (lower -33,280),
# on the 32-bit rows the rule then selects.
EDGE128 = {
    "seq255": (-127, -1, 128),    # s_eq = 255: the last byte-table value, fwd2
    "seq256": (-127, -1, 129),    # s_eq = 256: first value past the table, pk
    "seq255_w": (-127, -6, 128),  # the same scores with mismatch -6: int32 by the rule
    "seq256_w": (-127, -6, 129),
}
# max_sequence_size 600: int16 by the reference's rule, yet E(j, j) = j * (match - gap) passes 32,767
EDOMAIN = {
    "edom_fwd2": (-20, -1, 40),   # upper 24,000, lower -24,600; fwd2_ok
    "edom_pk": (-15, -20, 45),    # upper 27,000, lower -27,000; s_ne = -5: pk
}
WIDE = {"x10": (-80, -60, 80)}    # the default x 10: 32-bit rows, the default's output by design
WIDE_BANDED = {"x10": (-80, -60, 80), "wide_asym": (-30, -70, 90)}
POSITIVE_GAP = {"gap_pos": (2, -6, 8)}  # banded only: the global-memory kernel
TIE_SETS = ("zero", "mm_eq_2gap", "mm_eq_gap")
SCALED = {"x10"}                  # exempt from "differs from the default's output"

ALL = {**GENERAL, **EDGE128, **EDOMAIN, **WIDE, **WIDE_BANDED, **POSITIVE_GAP}


def up4(v):
    return (v + 3) // 4 * 4


# ---- the reference's rules, restated -----------------------------------------

def ref_score_bits(max_seq, gap, mismatch, match, graph_dim=None):
    """use32bitScore (cudapoa_limits.hpp:28-37).  graph_dim: max_matrix_graph_dimension
    (the full-alignment one, also for banded batches), 3 * max_seq rounded up to 4 by default."""
    graph_dim = up4(3 * max_seq) if graph_dim is None else graph_dim
    upper = max_seq * match
    lower = max_seq * max(gap, mismatch) + (graph_dim - max_seq) * gap
    return 32 if upper > 32767 or -lower > 32768 else 16


def ref_size_bits(score_bits, max_seq, banded, max_consensus=None, graph_dim=None, graph_dim_banded=None):
    """use32bitSize (cudapoa_limits.hpp:39-53) under batch.cu:45-73: a 16-bit score implies a 16-bit size."""
    if score_bits == 16:
        return 16
    m = 2 * max_seq if max_consensus is None else max_consensus
    if banded:
        m = max(m, up4(4 * max_seq) if graph_dim_banded is None else graph_dim_banded)
    else:
        m = max(m, up4(3 * max_seq) if graph_dim is None else graph_dim)
    m = max(m, up4(max_seq))
    return 32 if m > 32767 else 16


def fwd2_ok(gap, mismatch, match):
    """poa_fwd2.hpp fwd2_ok: both substitution scores fit a byte in the E domain."""
    return 0 <= match - gap <= 255 and 0 <= mismatch - gap <= 255


def e_domain_fits(max_seq, gap, mismatch, match, graph_dim=None):
    """E[i][j] = H[i][j] - j * gap as int16 for every column j <= max_seq, H within the
    reference's own bounds ("The E domain and its bound")."""
    graph_dim = up4(3 * max_seq) if graph_dim is None else graph_dim
    upper = max_seq * match
    lower = max_seq * max(gap, mismatch) + (graph_dim - max_seq) * gap
    return upper - max_seq * min(gap, 0) <= 32767 and lower - max_seq * max(gap, 0) >= -32768


def full_kernel_variant(max_seq, scores):
    """kernel_variant() of a full-alignment batch at the tests' sizes (16-bit node
    ids): the LDS kernel (2), except 16-bit rows whose E domain does not fit (1)."""
    if ref_score_bits(max_seq, *scores) == 16 and not e_domain_fits(max_seq, *scores):
        return 1
    return 2


# ---- windows -------------------------------------------------------------------

def _bursts(rng, seq, n, k):
    """seq with n stretches of k bases rewritten at random."""
    r = bytearray(seq)
    for _ in range(n):
        p = rng.randrange(0, len(r) - k)
        r[p:p + k] = bytes(rng.choice(b"ACGT") for _ in range(k))
    return bytes(r)


@functools.lru_cache(maxsize=None)
def windows(kind):
    """kind -> (windows, max_sequence_size).  Nothing is filtered after generation."""
    if kind == "w300":    # general sets: one wave of the 16-bit LDS kernel
        return synth.poa_windows(7, 6, 300, 8, 15, 15, 15), 400
    if kind == "w580":    # two waves (the hand-over between them carries E values), E-domain cases
        return synth.poa_windows(11, 4, 580, 8, 10, 10, 10), 600
    if kind == "w580e":   # w580 and a window with reads equal to its backbone, E(j, j) = j * (match - gap)
        rng = random.Random(18)  # exactly, and reads with rewritten stretches (where -20/-1/40 aligns differently)
        bb = bytes(rng.choice(b"ACGT") for _ in range(596))
        return windows("w580")[0] + [[bb, bb, _bursts(rng, bb, 12, 7), bb[3:], _bursts(rng, bb, 12, 9)]], 600
    if kind == "w280":    # 32-bit rows at one wave
        return synth.poa_windows(13, 6, 280, 8, 15, 15, 15), 300
    if kind == "w100":    # max_sequence_size 128: reads <= 120 bases
        return synth.poa_windows(15, 6, 100, 8, 5, 5, 5), 128
    if kind == "tie":     # repeats, an empty and a one-base read: ties everywhere
        t = b"ACGTTGCA" * 30
        return [[t, b"A" * 200, b"AC" * 100, b"", b"A", t + b"T", b"CA" * 100,
                 _bursts(random.Random(9), t, 6, 7)]], 400
    if kind == "band":    # w300 and a window with a read much shorter and one much longer than the graph
        rng = random.Random(23)   # (band gradient above and below 1: where minv / Tmax comparisons are taken)
        bb = bytes(rng.choice(b"ACGT") for _ in range(390))
        near = bytearray(bb[:200])
        for _ in range(8):
            near[rng.randrange(len(near))] = rng.choice(b"ACGT")
        return windows("w300")[0] + [[bb[:200], bb[60:90], bb, bytes(near), bb[:30], bb[:200] + bb[150:330]]], 400
    raise KeyError(kind)


def max_nodes(max_seq, banded):
    return up4((4 if banded else 3) * max_seq)


@functools.lru_cache(maxsize=None)
def oracle_results(kind, scores, banded=False, bw=256, score_bits=16, msa=False, spoa=False, reads=8):
    """The oracle's WindowResult per window of windows(kind), graphs included.  Shared: do not modify."""
    wins, max_seq = windows(kind)
    gap, mismatch, match = scores
    return tuple(oracle.poa_window(w, gap=gap, mismatch=mismatch, match=match, banded=banded, band_width=bw,
                                   msa=msa, score_bits=score_bits, max_nodes=max_nodes(max_seq, banded),
                                   max_consensus=2 * max_seq, max_seqs=reads, want_graph=True, spoa_accurate=spoa)
                 for w in wins)


def observable(r):
    """What a consensus batch returns for a window, with the graph."""
    return (r.status, r.consensus, r.coverage, r.graph["bases"][:r.final_nodes],
            tuple(tuple(ins) for ins in r.graph["in"]))
