"""The row loop of the 16-bit LDS forward pass (fwd2_rows, poa_fwd2.hpp): an
outer loop per hand-over block, the rows inside it, the previous row carried
as a register tuple, column 0 of the first span, the HBM carries of a later
sweep stored once per block, spill rows stored behind one test per row.

Every case compares status, consensus, coverage and the final graph with the
oracle, on a persistent grid of three workgroups with two generates.  Shapes:
8,2 (the default), 8,1 (one wave: every span but the last keeps its carries in
HBM) and 4,4 (four cells per lane, middle waves that take and post).  A span
is 64 * CPL read columns.

Windows (at most 6 reads each):
 * graph lengths V of the first alignment around the row loop's block of 16
   and the carry register's 64 lanes: 1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64,
   65, 129.  The graph is a chain, so its sink is row V: the last row of a
   block at V = 15, 31, 63, the first row of one at V = 16, 32, 64;
 * column 0 on the first span.  Every bubble parts after the first base, so
   the cell at read column 1 of the row that closes it takes column 0 of a
   predecessor k + 1 rows back: insertions of 1 .. 6 bases (ring rows 2 .. 7
   back) and of 7, 14, 15, 16 and 62 bases (8, 15, 16, 17 and 63 back, beyond
   the ring: spill rows); deletions of 12, 20, 64 and 70 bases in one read
   (far predecessors across one and several block edges, 64 and more rows
   back); a second source node; a non-ACGT first base; and a substitution at
   the second base, after which the third node's two predecessors tie at
   column 0 (the code keeps the first maximising slot), with reads that lack
   the first bases so the walk runs up column 0;
 * inactive lanes: reads of 1, 7, 8, 9, span - 1, span and span + 1 bases, and
   one just over NW spans (a second sweep, fed by the HBM carries);
 * spill rows: after a read with a long deletion the far edge stays in the
   graph, so every later read of the window takes a predecessor from a spill
   row written earlier in the same pass, one or more blocks before.
"""
import random

import pytest

from claragenomicsanalysis_amd.cudapoa import CudaPoaBatch
from oracle import oracle

MEM = 8 << 30
MAX_SEQ = 1100
MAX_SEQS = 6
V_FIRST = (1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129)
INSERTIONS = (1, 2, 3, 4, 5, 6, 7, 14, 15, 16, 62)
DELETIONS = (12, 20, 64, 70)
SHAPES = ("8,2", "8,1", "4,4")


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
    rng = random.Random(1000 * cpl + nw)
    wins = []
    # chains of V nodes against a short read and one that reaches the next span
    for v in V_FIRST:
        tmpl = _seq(rng, span + 60)
        wins.append([tmpl[:v], _noisy(rng, tmpl[:v + 3]), _noisy(rng, tmpl[:span + 44]), tmpl[:max(v, 9)]])
    # bubbles that part after the first base: insertions of k bases
    for k in INSERTIONS:
        bb = _seq(rng, 150)
        ins = "".join(_other(bb[1], 1 + i % 3) for i in range(k))
        alt = bb[:1] + ins + bb[1:]
        wins.append([bb, alt, bb, alt, bb[:120]])
    # ... and deletions of d bases in one read; the later reads meet the far edge
    for d in DELETIONS:
        bb = _seq(rng, 190)
        cut = bb[:1] + bb[1 + d:]
        wins.append([bb, cut, bb, cut, _noisy(rng, bb), bb[:1] + bb[1 + d:150]])
    # a second source node, a non-ACGT first base
    bb = _seq(rng, 140)
    wins.append([bb, _other(bb[0]) + bb[1:], bb, _other(bb[0], 2) + bb[1:], bb[1:]])
    wins.append([bb, "N" + bb[1:], bb, "N" + bb[1:], bb[:100]])
    # a substitution at the second base: the third node's predecessors tie at
    # column 0; reads without the first bases walk up column 0
    alt = bb[:1] + _other(bb[1]) + bb[2:]
    wins.append([bb, alt, bb[3:], alt, bb[2:], bb[4:90]])
    # short and span-sized reads against a graph longer than a block
    tmpl = _seq(rng, span + 40)
    wins.append([tmpl[:70], tmpl[:1], tmpl[:7], tmpl[:8], tmpl[:9], tmpl[:70]])
    wins.append([tmpl[:span + 20], tmpl[:span - 1], tmpl[:span], tmpl[:span + 1], _noisy(rng, tmpl[:span])])
    # just over NW spans: a second sweep
    n = nw * span
    assert n + 30 <= MAX_SEQ - 8
    tmpl = _seq(rng, n + 40)
    wins.append([tmpl[:n + 9], _noisy(rng, tmpl[:n + 1]), _noisy(rng, tmpl[:n + 7]), tmpl[:n + 30]])
    return [[r.encode() for r in w] for w in wins]


def _snapshot(b):
    graphs, _ = b.get_graphs()
    gs = [({e: g.weight(*e) for e in g.edges}, {v: g.label(v) for v in g.nodes}) for g in graphs]
    cons, cov, st = b.get_consensus()
    return [(st[i], cons[i], cov[i], gs[i]) for i in range(len(st))]


_EXPECT = {}


def _expect(shape, wins):
    # computed once per shape and shared by the checks below; never changed
    if shape not in _EXPECT:
        out = []
        for w in wins:
            r = oracle.poa_window(w, max_nodes=3 * MAX_SEQ, max_consensus=2 * MAX_SEQ, max_seqs=MAX_SEQS,
                                  want_graph=True)
            g = ({}, {})
            if r.status == 0:
                edges = {(src, v): wt for v, ins in enumerate(r.graph["in"]) for (src, wt) in ins}
                g = (edges, {v: r.graph["bases"][v] for v in sorted({x for e in edges for x in e})})
            out.append((r.status, r.consensus, r.coverage, g))
        _EXPECT[shape] = out
    return _EXPECT[shape]


@pytest.mark.parametrize("shape", SHAPES)
def test_fwd_rows_windows_valid(shape):
    """CPU: every window is one the oracle accepts, so the GPU comparison below covers every case"""
    cpl, nw = (int(x) for x in shape.split(","))
    wins = _windows(cpl, nw)
    assert max(len(r) for w in wins for r in w) <= MAX_SEQ and max(len(w) for w in wins) <= MAX_SEQS
    bad = [i for i, e in enumerate(_expect(shape, wins)) if e[0] != 0]
    assert not bad, (shape, bad)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_fwd_rows(shape, monkeypatch):
    cpl, nw = (int(x) for x in shape.split(","))
    monkeypatch.delenv("GWAMD_POA_KERNEL", raising=False)
    monkeypatch.delenv("GWAMD_POA_ADD", raising=False)
    monkeypatch.delenv("GWAMD_POA_FWD", raising=False)
    monkeypatch.setenv("GWAMD_DIAG", "1")
    monkeypatch.setenv("GWAMD_POA_LDS_SHAPE", shape)
    monkeypatch.setenv("GWAMD_POA_SLOTS", "3")
    wins = _windows(cpl, nw)
    expect = _expect(shape, wins)
    assert all(e[0] == 0 for e in expect)
    b = CudaPoaBatch(MAX_SEQS, MAX_SEQ, MEM, alignment_band_width=256)
    for w in wins:
        st, _ = b.add_poa_group(list(w))
        assert st == 0
    for rep in range(2):
        b.generate_poa()
        assert b.kernel_variant() == 2 and b.get_types()[0] == 16 and b.get_grid()[0] == 3
        for i, (g, e) in enumerate(zip(_snapshot(b), expect)):
            assert g == e, (shape, rep, i)
