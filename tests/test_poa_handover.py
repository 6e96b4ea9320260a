"""The block hand-over of row carries between the waves of the 16-bit LDS
forward pass (fwd2_rows, poa_fwd2.hpp; arithmetic in poa_handover.hpp).

Every case compares status, consensus, coverage and the final graph with the
oracle, on a persistent grid of three workgroups with two generates, so the
control region (head, tail, channel slots) is reused by later windows and by
the second launch.  The shapes 8,2 (default), 8,3, 8,4 and 4,4 make the middle
waves both take and post carries; a span is 64 * CPL read columns.

The graph lengths V of a window's first alignment sit around the block sizes
B = 8 and 16 and the channel depth 64: B-1, B, B+1, 63, 64, 65, 64+B-1, 64+B+1
and 3*64+1 (the channel wraps three times), each against reads long enough to
reach the second (and at 4,4 the third) wave.  The other cases: a long graph
with a read of exactly one span (no feed) and of one span plus one column; a
read just over NW spans (second sweep: the channels restart and wave 0 takes
its carries from HBM); bubbles whose branches part exactly at the second
wave's first column (ring predecessors at distance 2 .. 7: the boundary value
comes from the carry register); and marked rows there (a non-ACGT base, a
predecessor farther back than the ring).
"""
import random

import pytest

from claragenomicsanalysis_amd.cudapoa import CudaPoaBatch
from oracle import oracle

MEM = 8 << 30
MAX_SEQ = 1100
MAX_SEQS = 6
BLOCKS = (8, 16)
V_FIRST = sorted({v for B in BLOCKS for v in (B - 1, B, B + 1, 64 + B - 1, 64 + B + 1)} | {63, 64, 65, 3 * 64 + 1})


def _seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def _noisy(rng, s, sub=0.03):
    r = [rng.choice("ACGT") if rng.random() < sub else c for c in s]
    for _ in range(len(r) // 150):
        r.insert(rng.randrange(len(r)), rng.choice("ACGT"))
        del r[rng.randrange(len(r))]
    return "".join(r)


def _other(c, k=1):
    return "ACGT"[("ACGT".index(c) + k) % 4]


def _windows(cpl, nw):
    span = 64 * cpl
    rng = random.Random(100 * cpl + nw)
    wins = []
    # short graphs against reads that reach the later waves
    long_reads = [span + 44, min(2 * span + 88, MAX_SEQ - 8)]
    for v in V_FIRST:
        tmpl = _seq(rng, max(long_reads) + 8)
        bb = tmpl[:v]
        wins.append([bb] + [_noisy(rng, tmpl[:n]) for n in long_reads] + [_noisy(rng, tmpl[:span + 1])])
    # long graph; reads of exactly one span (no feed) and one span plus a column
    tmpl = _seq(rng, span + 120)
    wins.append([tmpl[:span + 100], _noisy(rng, tmpl[:span]), _noisy(rng, tmpl[:span + 1]), tmpl[:span]])
    # just over NW spans: a second sweep, where the shape's sweep fits a 16-bit batch
    if nw * span + 9 <= MAX_SEQ - 8:
        n = nw * span
        tmpl = _seq(rng, n + 40)
        wins.append([tmpl[:n + 9], _noisy(rng, tmpl[:n + 1]), _noisy(rng, tmpl[:n + 7]), tmpl[:n + 30]])
    # bubbles that part at column span + 1: an insertion of k bases after
    # column span puts the next node's predecessor k + 1 rows back; a
    # substitution at column span + 1 two rows back
    for k in (1, 2, 3, 5, 6):
        bb = _seq(rng, span + 70)
        ins = "".join(_other(bb[span], 1 + i % 3) for i in range(k))
        wins.append([bb, bb[:span] + ins + bb[span:], bb, bb[:span] + ins + bb[span:], bb[:span + 60]])
    bb = _seq(rng, span + 70)
    alt = bb[:span] + _other(bb[span]) + bb[span + 1:]
    wins.append([bb, alt, bb, alt, bb[:span] + _other(bb[span], 2) + bb[span + 1:], bb])
    # marked rows at that column: a base that is not A/C/G/T, and a
    # predecessor farther back than the 8 ring rows (an insertion of 12)
    bb = _seq(rng, span + 70)
    wins.append([bb[:span] + "N" + bb[span + 1:], bb, bb[:span] + "N" + bb[span + 1:], bb])
    ins = "".join(_other(bb[span], 1 + i % 3) for i in range(12))
    wins.append([bb, bb[:span] + ins + bb[span:], bb, bb[:span] + ins + bb[span:]])
    return [[r.encode() for r in w] for w in wins]


def _snapshot(b):
    graphs, _ = b.get_graphs()
    gs = [({e: g.weight(*e) for e in g.edges}, {v: g.label(v) for v in g.nodes}) for g in graphs]
    cons, cov, st = b.get_consensus()
    return [(st[i], cons[i], cov[i], gs[i]) for i in range(len(st))]


def _expect(wins):
    out = []
    for w in wins:
        r = oracle.poa_window(w, max_nodes=3 * MAX_SEQ, max_consensus=2 * MAX_SEQ, max_seqs=MAX_SEQS, want_graph=True)
        g = ({}, {})
        if r.status == 0:
            edges = {(src, v): wt for v, ins in enumerate(r.graph["in"]) for (src, wt) in ins}
            g = (edges, {v: r.graph["bases"][v] for v in sorted({x for e in edges for x in e})})
        out.append((r.status, r.consensus, r.coverage, g))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["8,2", "8,3", "8,4", "4,4"])
def test_block_handover(shape, monkeypatch):
    cpl, nw = (int(x) for x in shape.split(","))
    monkeypatch.delenv("GWAMD_POA_KERNEL", raising=False)
    monkeypatch.delenv("GWAMD_POA_ADD", raising=False)
    monkeypatch.delenv("GWAMD_POA_FWD", raising=False)
    monkeypatch.setenv("GWAMD_DIAG", "1")
    monkeypatch.setenv("GWAMD_POA_LDS_SHAPE", shape)
    monkeypatch.setenv("GWAMD_POA_SLOTS", "3")
    wins = _windows(cpl, nw)
    assert max(len(r) for w in wins for r in w) <= MAX_SEQ and max(len(w) for w in wins) <= MAX_SEQS
    expect = _expect(wins)
    assert sum(e[0] == 0 for e in expect) >= len(expect) - 2
    b = CudaPoaBatch(MAX_SEQS, MAX_SEQ, MEM, alignment_band_width=256)
    for w in wins:
        st, _ = b.add_poa_group(list(w))
        assert st == 0
    for rep in range(2):
        b.generate_poa()
        assert b.kernel_variant() == 2 and b.get_types()[0] == 16 and b.get_grid()[0] == 3
        for i, (g, e) in enumerate(zip(_snapshot(b), expect)):
            assert g == e, (shape, rep, i)
