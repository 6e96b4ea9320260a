"""Shared by the error-status tests (test_poa_limits.py on the GPU,
test_poa_limits_cpu.py without one): small deterministic windows that end in
each kernel-raised status (enum Status, poa_common.hpp), every one with a near
miss one step below its limit that must succeed, and the oracle's outputs
(computed once per mode).

A batch has one set of capacities, so the windows come in groups, one batch
each: "fan" (edge limit, empty graphs), "nodes" (node limit, two errors in one
read), "cons" (consensus and MSA capacity) and, for banded batches with gap 0
only, "tb7" (the traceback's loop bound).  Within a group the capacity is
fixed and the windows differ by one node, one edge or one base, so that the
limit falls between an error window and its near miss.  The statuses written
here are what the reference's rules give; test_poa_limits_cpu.py re-derives
every one on the oracle.

No fan holds more than 49 fan reads: a kernel that missed status 5 would
write slot 49 of a 50-slot list, which is in range, and fail on the status.
"""
import collections
import functools
import random

from claragenomicsanalysis_amd import synth
from oracle import oracle

DEFAULT = (-8, -6, 8)
X10 = (-80, -60, 80)        # poa_score_sets.WIDE["x10"]: 32-bit rows where the sizes allow
X40 = (-320, -240, 320)     # the default x 40: 32-bit rows at 172 nodes too (172 * 320 > 32,767)
BAND = 128
MAX_SEQS = 64
MAX_EDGES = 50
FAN_POSITIONS = (60, 0, 1, 118, 119)

# 49 distinct printable bytes outside ACGT / acgt, and one more for single new nodes elsewhere
VARIANTS = (b"BDEFHIJKLMNOPQRSUVWXYZ" + b"bdefhijklmnopqrsuvwxyz" + b"01234")[:49]
OTHER = b"#"[0]
assert len(set(VARIANTS)) == 49 and not set(VARIANTS) & set(b"ACGTacgt#")

# name, reads, status of a consensus batch, status of an MSA batch
Case = collections.namedtuple("Case", "name reads want want_msa")
# capacities of one batch: max_sequence_size, max_nodes_per_window (and _banded), max_consensus_size
Group = collections.namedtuple("Group", "name max_seq max_nodes max_cons cases")


def _dna(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def _sub(seq, *subs):
    r = bytearray(seq)
    for p, byte in subs:
        r[p] = byte
    return bytes(r)


BACKBONE = _dna(random.Random(4201), 120)


# ---- edge fans -------------------------------------------------------------------

def byte_fan(p, n):
    """The backbone and n reads, read k with position p replaced by variant k:
    each adds one node aligned to node p, one out-edge of node p - 1 and one
    in-edge of node p + 1."""
    return [BACKBONE] + [_sub(BACKBONE, (p, VARIANTS[k])) for k in range(n)]


@functools.lru_cache(maxsize=None)
def dna_backbone():
    """A 40-base anchor ending in A, 60 bases over CGT, a 150-base tail: the
    anchor's last base matches no middle base, so a deletion behind it cannot shift."""
    rng = random.Random(4202)
    return _dna(rng, 39) + b"A" + _dna(rng, 60, b"CGT") + _dna(rng, 150)


def dna_fan(n):
    """Read k (1..n) deletes the first k middle bases: one more out-edge of the anchor's last node (39)."""
    bb = dna_backbone()
    return [bb] + [bb[:40] + bb[40 + k:] for k in range(1, n + 1)]


# ---- node limit ----------------------------------------------------------------------

def insertion_window(lengths, subs=0, inserted=0):
    """The backbone and one read per entry of lengths, read i with that many
    random bases inserted behind backbone position 10 + 20 i.  A later read may
    run part of the way through an earlier read's branch, so the node and
    column counts are not the sums of the lengths (157 nodes and 149 MSA
    columns after [20, 20]; test_poa_limits_cpu.py asserts them).  The last
    read tops them up exactly: `subs` bytes no base matches, three positions
    apart from 60 on (one new aligned node each, no new column) or `inserted`
    such bytes behind position 80 (one new node and one new column each)."""
    rng = random.Random(4203)
    ins = [_dna(rng, 20) for _ in range(5)]
    w = [BACKBONE] + [BACKBONE[:10 + 20 * i] + ins[i][:n] + BACKBONE[10 + 20 * i:] for i, n in enumerate(lengths)]
    if subs:
        w.append(_sub(BACKBONE, *[(60 + 3 * i, OTHER) for i in range(subs)]))
    if inserted:
        w.append(BACKBONE[:80] + bytes([OTHER]) * inserted + BACKBONE[80:])
    return w


def two_error_fan(fillers):
    """The 48-variant fan at 60 and `fillers` reads with one new byte each
    elsewhere: N = 168 + fillers nodes, 49 out-edges at node 59 and 49 in-edges at node 61."""
    return byte_fan(60, 48) + [_sub(BACKBONE, (30 + 5 * i, OTHER)) for i in range(fillers)]


READ_A = _sub(BACKBONE, (20, OTHER), (60, VARIANTS[48]))   # a new node at 20, then the 49th variant at 60
READ_B = _sub(BACKBONE, (60, VARIANTS[48]), (100, OTHER))  # the 49th variant at 60, then a new node at 100
READ_1 = _sub(BACKBONE, (20, OTHER))                       # near misses: one and two new nodes, no fan edge
READ_2 = _sub(BACKBONE, (20, OTHER), (100, OTHER))


def _ordinary(seed, n, backbone_len, edits):
    return [Case("ordinary%d" % i, w, 0, 0)
            for i, w in enumerate(synth.poa_windows(seed, n, backbone_len, 8, edits, edits, edits))]


def _interleave(cases, ordinary):
    """Ordinary windows spread between the others, in a fixed order."""
    out = list(cases)
    step = max(1, len(out) // (len(ordinary) + 1))
    for i, o in enumerate(ordinary):
        out.insert((i + 1) * step + i, o)
    return out


@functools.lru_cache(maxsize=None)
def group(name):
    """name -> Group.  An error window is followed by its near miss."""
    if name == "fan":
        # default capacities at max_sequence_size 256 (768 nodes, 1,024 banded, consensus 512)
        cases = []
        for p in FAN_POSITIONS:
            cases += [Case("fan49_p%d" % p, byte_fan(p, 49), 5, 5), Case("fan48_p%d" % p, byte_fan(p, 48), 0, 0)]
        cases += [Case("fan48_repeat", byte_fan(60, 48) + [byte_fan(60, 1)[1]], 0, 0),  # the edge exists: no error
                  Case("dna49", dna_fan(49), 5, 5), Case("dna48", dna_fan(48), 0, 0),
                  Case("empty1", [b""], 7, 0), Case("empty2", [b"", b""], 7, 0),
                  Case("empty_then_read", [b"", BACKBONE], 0, 0)]
        return Group(name, 256, 768, 512, tuple(_interleave(cases, _ordinary(4210, 3, 240, 10))))
    if name == "nodes":
        # 172 nodes (a multiple of 4: the host rounds node capacities up to one), full and banded
        M = 172
        rng = random.Random(4204)
        bb172 = _dna(rng, M)
        cases = [
            # N = M - 2: the node limit comes first in read A, the edge limit in read B
            Case("two_A", two_error_fan(2) + [READ_A], 4, 4), Case("two_B", two_error_fan(2) + [READ_B], 5, 5),
            Case("two_near", two_error_fan(2) + [READ_1], 0, 0),
            # N = M - 1: the first new node of either read is one too many
            Case("two_A_m1", two_error_fan(3) + [READ_A], 4, 4), Case("two_B_m1", two_error_fan(3) + [READ_B], 4, 4),
            # N = M - 3: both reads reach the fan first
            Case("two_A_m3", two_error_fan(1) + [READ_A], 5, 5), Case("two_B_m3", two_error_fan(1) + [READ_B], 5, 5),
            Case("two_near_m3", two_error_fan(1) + [READ_2], 0, 0),
            # 157 nodes after two reads, 177 after three: the limit falls in the middle of the third
            Case("ins_mid", insertion_window([20] * 5), 4, 4),
            # the last node that fits, the first that does not
            Case("ins_172", insertion_window([20, 20], subs=15), 4, 4),
            Case("ins_171", insertion_window([20, 20], subs=14), 0, 0),
            # the check before a read: the backbone alone fills the graph
            Case("backbone_172", [bb172, bb172], 4, 4), Case("backbone_171", [bb172[:-1], bb172[:-1]], 0, 0),
        ]
        return Group(name, M, M, 2 * M, tuple(_interleave(cases, _ordinary(4220, 2, 100, 4))))
    if name == "cons":
        # max_consensus_size 161 = max_sequence_size: C = L, C = L + 1, and the MSA's 161 and 160 columns
        C = 161
        rng = random.Random(4205)
        r161 = _dna(rng, C)
        cases = [
            Case("cons_L161", [r161] * 3, 2, 2), Case("cons_L160", [r161[:-1]] * 3, 0, 0),
            Case("cols_161", insertion_window([20, 20], inserted=12), 0, 2),
            Case("cols_160", insertion_window([20, 20], inserted=11), 0, 0),
            Case("empty1", [b""], 7, 0),
        ]
        return Group(name, C, 484, C, tuple(_interleave(cases, _ordinary(4230, 2, 120, 5))))
    if name == "tb7":
        # Status 7 from the banded traceback (found by the bounded search of
        # test_poa_limits_cpu.py, not by hand): a 2-node graph and a read so long
        # that its last column lies outside the last row's band.  The end cell
        # then holds min_score_value, and with gap 0 the horizontal step
        # "matches" for ever; the loop bound ends it.  188 bases still end inside
        # the band.  Banded batches with GAP0 only: the full alignment and the
        # default scores give status 0 for both windows.
        r = _dna(random.Random(4206), 200)
        cases = [Case("tb7_L200", [r[:2], r], 7, 7), Case("tb7_L188", [r[:2], r[:188]], 0, 0)]
        return Group(name, 256, 1024, 512, tuple(cases + _ordinary(4240, 1, 240, 10)))
    raise KeyError(name)


GROUPS = ("fan", "nodes", "cons")
GAP0 = (0, -6, 8)           # poa_score_sets.GENERAL["gap0"]: the scores of group "tb7"
GAP0_WIDE = (0, -768, 1024) # the same x 128: 32-bit rows (256 * 1,024 > 32,767; gap 0 leaves the lower bound at 0)


@functools.lru_cache(maxsize=None)
def oracle_results(name, banded=False, msa=False, score_bits=16, scores=DEFAULT, spoa=False):
    """The oracle's WindowResult per window of group(name), graphs included.  Shared: do not modify."""
    g = group(name)
    gap, mismatch, match = scores
    return tuple(oracle.poa_window(c.reads, gap=gap, mismatch=mismatch, match=match, banded=banded, band_width=BAND,
                                   msa=msa, score_bits=score_bits, max_nodes=g.max_nodes, max_consensus=g.max_cons,
                                   max_seqs=MAX_SEQS, want_graph=True, spoa_accurate=spoa)
                 for c in g.cases)


def run_oracle(reads, banded=False, msa=False, score_bits=16, scores=DEFAULT, max_nodes=768, max_cons=512,
               want_graph=True):
    gap, mismatch, match = scores
    return oracle.poa_window(reads, gap=gap, mismatch=mismatch, match=match, banded=banded, band_width=BAND,
                             msa=msa, score_bits=score_bits, max_nodes=max_nodes, max_consensus=max_cons,
                             max_seqs=MAX_SEQS, want_graph=want_graph)


def degrees(r):
    """(in-degree, out-degree) per node of a WindowResult's graph."""
    ins = [len(e) for e in r.graph["in"]]
    outs = [0] * len(ins)
    for e in r.graph["in"]:
        for src, _ in e:
            outs[src] += 1
    return ins, outs
