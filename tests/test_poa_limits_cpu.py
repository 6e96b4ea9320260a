"""The error statuses on the oracle alone (no GPU): every window of
poa_limit_windows.py ends in the status stated there, in every mode the GPU
tests run; every near miss succeeds with an output; the fans fill the slots
they are planned to fill; and the reference's firing rules, restated here in
a few lines each, agree with the oracle on both sides of every limit.  So
test_poa_limits.py cannot pass vacuously: its expectations hold every status
in {0, 2, 4, 5, 7}.
"""
import random

import pytest

import poa_limit_windows as W
import poa_score_sets as S
from claragenomicsanalysis_amd import cudapoa
from oracle import oracle

# (banded, msa, score bits, scores): full 16-bit, full 32-bit, MSA, banded 128, banded 128 with MSA and 32-bit scores
MODES = [(False, False, 16, W.DEFAULT), (False, False, 32, W.X10), (False, True, 16, W.DEFAULT),
         (True, False, 16, W.DEFAULT), (True, True, 32, W.X10)]
TB7_MODES = [(True, False, 16, W.GAP0), (True, True, 16, W.GAP0), (True, False, 32, W.GAP0_WIDE)]


# ---- the reference's firing rules, restated ------------------------------------------

def edge_rule(out_count, in_count):
    """cudapoa_add_alignment.cuh:245, after the new edge is written at slots out_count / in_count."""
    return out_count + 1 >= W.MAX_EDGES or in_count + 1 >= W.MAX_EDGES


def node_rule(node_count_after_increment, max_nodes):
    """cudapoa_add_alignment.cuh:114 and :170; the same comparison before a read, cudapoa_kernels.cuh:222-225."""
    return node_count_after_increment >= max_nodes


def consensus_rule(count, max_cons):
    """cudapoa_generate_consensus.cuh:264; count is the consensus length - 1 (the walk's steps)."""
    return count >= max_cons - 1


def msa_rule(msa_len, max_cons):
    """cudapoa_generate_msa.cuh:200."""
    return msa_len >= max_cons


def loop_rule(loops, n):
    """cudapoa_generate_consensus.cuh:228 (n nodes; also fires for an empty graph, 0 >= 0) and the
    tracebacks' bound, cudapoa_nw_banded.cuh:390 and :476, cudapoa_nw.cuh:362 and :454 (n = read length +
    graph rows + 2)."""
    return loops >= n


def _want(c, msa):
    return c.want_msa if msa else c.want


def _has_output(r, msa):
    return bool(r.msa) and any(r.msa) if msa else bool(r.consensus) and len(r.coverage) == len(r.consensus)


# ---- every window, every mode ------------------------------------------------------------

@pytest.mark.parametrize("name", W.GROUPS + ("tb7",))
def test_every_window_has_its_stated_status(name):
    g = W.group(name)
    for banded, msa, sbits, scores in (TB7_MODES if name == "tb7" else MODES):
        if name == "nodes" and sbits == 32:
            scores = W.X40
        for c, r in zip(g.cases, W.oracle_results(name, banded, msa, sbits, scores)):
            assert r.status == _want(c, msa), (c.name, banded, msa, sbits)
            if r.status == 0 and c.reads != [b""] and c.reads != [b"", b""]:
                assert _has_output(r, msa), (c.name, banded, msa, sbits)
            if r.status != 0:
                assert r.consensus == "" and r.coverage == [] and r.msa is None
        # the scaled scores are there for the row width alone: the default's statuses and outputs
        if sbits == 32 and name != "tb7":
            base = W.oracle_results(name, banded, msa, 16, W.DEFAULT)
            got = W.oracle_results(name, banded, msa, sbits, scores)
            assert [(r.status, r.consensus, r.msa) for r in got] == [(r.status, r.consensus, r.msa) for r in base]


def test_statuses_reached_are_exactly_the_kernel_raised_ones():
    seen = set()
    near = 0
    for name in W.GROUPS + ("tb7",):
        g = W.group(name)
        for banded, msa, sbits, scores in (TB7_MODES if name == "tb7" else MODES):
            if name == "nodes" and sbits == 32:
                scores = W.X40
            rs = W.oracle_results(name, banded, msa, sbits, scores)
            seen |= {r.status for r in rs}
            # every error window is followed (ordinary windows apart) by a window that succeeds
            plain = [(c, r) for c, r in zip(g.cases, rs) if not c.name.startswith("ordinary")]
            for (c, r), (c2, r2) in zip(plain, plain[1:]):
                if r.status != 0 and r2.status == 0:
                    near += 1
    assert seen == {0, 2, 4, 5, 7}
    assert near >= 40
    # status 6 cannot come from a kernel: BatchSize refuses max_nodes_per_window < max_sequence_size
    with pytest.raises(ValueError):
        cudapoa.BatchSize.make_full(256, 512, 252, 1024, 128, 8)
    with pytest.raises(ValueError):
        cudapoa.BatchSize.make_full(256, 512, 768, 252, 128, 8)
    # ... and rounds node capacities up to a multiple of 4
    bs = cudapoa.BatchSize.make_full(172, 344, 169, 170, 128, 8)
    assert (bs.max_nodes_per_window, bs.max_nodes_per_window_banded) == (172, 172)


# ---- edge fans ----------------------------------------------------------------------------

@pytest.mark.parametrize("banded,msa,sbits,scores", MODES)
@pytest.mark.parametrize("p", W.FAN_POSITIONS)
def test_byte_fan_slots(p, banded, msa, sbits, scores):
    """48 variants leave the fanned lists at 49 entries (the rule's last
    success: 48 + 1 >= 50 is false), the 49th writes slot 49 and fires."""
    kw = dict(banded=banded, msa=msa, score_bits=sbits, scores=scores)
    r48, r49 = W.run_oracle(W.byte_fan(p, 48), **kw), W.run_oracle(W.byte_fan(p, 49), **kw)
    assert (r48.status, r49.status) == (0, 5) and (r48.final_nodes, r49.final_nodes) == (168, 169)
    for r, n in ((r48, 48), (r49, 49)):
        ins, outs = W.degrees(r)
        if p > 0:      # out-edges of node p - 1: the backbone's and one per variant
            assert outs[p - 1] == n + 1
            assert edge_rule(outs[p - 1] - 1, 0) == (n == 49)
        if p < 119:    # in-edges of node p + 1; the 49th read stops at its out-edge first, one position earlier
            assert ins[p + 1] == (n + 1 if p == 0 or n == 48 else n)
        if p == 0:
            assert edge_rule(0, ins[1] - 1) == (n == 49)
        assert max(ins) <= W.MAX_EDGES and max(outs) <= W.MAX_EDGES
    # a repeat of variant 0: its edges exist, so nothing is written and nothing fires
    rep = W.run_oracle(W.byte_fan(p, 48) + [W.byte_fan(p, 1)[1]], **kw)
    assert rep.status == 0 and W.degrees(rep) == W.degrees(r48) and rep.final_nodes == 168


@pytest.mark.parametrize("banded", [False, True])
def test_dna_fan_slots(banded):
    for msa in (False, True):
        r48 = W.run_oracle(W.dna_fan(48), banded=banded, msa=msa)
        r49 = W.run_oracle(W.dna_fan(49), banded=banded, msa=msa)
        assert (r48.status, r49.status) == (0, 5)
        # no new node: every read is a path through the backbone's nodes
        assert r48.final_nodes == r49.final_nodes == 250
        assert W.degrees(r48)[1][39] == 49 and W.degrees(r49)[1][39] == 50
        assert max(W.degrees(r49)[0]) == 2
    # without the anchor's A (here: an anchor ending in a middle base) the fan does not form
    bb = bytearray(W.dna_backbone())
    bb[39] = bb[40]
    plain = [bytes(bb)] + [bytes(bb[:40] + bb[40 + k:]) for k in range(1, 50)]
    assert max(W.degrees(W.run_oracle(plain, banded=banded))[1]) < 49


# ---- two errors in one read -------------------------------------------------------------

@pytest.mark.parametrize("banded,msa", [(False, False), (False, True), (True, False)])
def test_first_error_in_read_order_wins(banded, msa):
    for fillers in (0, 2):
        fan = W.two_error_fan(fillers)
        N = W.run_oracle(fan, banded=banded, msa=msa).final_nodes
        assert N == 168 + fillers
        for cap, want_a, want_b in ((N + 1, 4, 4), (N + 2, 4, 5), (N + 3, 5, 5)):
            a = W.run_oracle(fan + [W.READ_A], banded=banded, msa=msa, max_nodes=cap)
            b = W.run_oracle(fan + [W.READ_B], banded=banded, msa=msa, max_nodes=cap)
            assert (a.status, b.status) == (want_a, want_b), (fillers, cap)
            # read A's first new node is N + 1 nodes, its second N + 2; read B reaches the fan with N + 1
            assert want_a == (4 if node_rule(N + 1, cap) or node_rule(N + 2, cap) else 5)
            assert want_b == (4 if node_rule(N + 1, cap) else 5)
    assert (168 + 2 + 2) % 4 == 0 and W.group("nodes").max_nodes == 168 + 2 + 2


# ---- node limit -------------------------------------------------------------------------

@pytest.mark.parametrize("banded", [False, True])
def test_node_limit_at_every_capacity(banded):
    w = W.insertion_window([20] * 5)
    total = W.run_oracle(w, banded=banded).final_nodes
    assert total == 211  # (a later read runs part of the way through an earlier read's branch)
    for cap in range(121, total + 2):
        r = W.run_oracle(w, banded=banded, max_nodes=cap, want_graph=False)
        assert r.status == (4 if node_rule(total, cap) else 0), cap
    # the counts the batch's windows rely on
    assert W.run_oracle(W.insertion_window([20, 20]), banded=banded).final_nodes == 157
    assert W.run_oracle(W.insertion_window([20, 20, 20]), banded=banded).final_nodes == 177
    for subs, want in ((14, 0), (15, 4)):
        r = W.run_oracle(W.insertion_window([20, 20], subs=subs), banded=banded, max_nodes=172)
        assert r.status == want and node_rule(157 + subs, 172) == (want == 4)
    # before a read: the backbone alone reaches the capacity
    rng = random.Random(1)
    bb = bytes(rng.choice(b"ACGT") for _ in range(172))
    for n, want in ((172, 4), (171, 0)):
        r = W.run_oracle([bb[:n], bb[:n]], banded=banded, max_nodes=172)
        assert r.status == want and node_rule(n, 172) == (want == 4)


# ---- consensus and MSA capacity -----------------------------------------------------------

@pytest.mark.parametrize("banded,msa", [(False, False), (False, True), (True, False)])
def test_consensus_capacity(banded, msa):
    rng = random.Random(2)
    read = bytes(rng.choice(b"ACGT") for _ in range(161))
    for L, C, want in ((120, 120, 2), (120, 121, 0), (161, 161, 2), (160, 161, 0)):
        r = W.run_oracle([read[:L]] * 3, banded=banded, msa=msa, max_cons=C)
        assert r.status == want, (L, C)
        assert (msa_rule(L, C) if msa else consensus_rule(L - 1, C)) == (want == 2)
        if want == 0:
            assert (r.msa == [read[:L].decode()] * 3) if msa else (r.consensus == read[:L].decode())


@pytest.mark.parametrize("banded", [False, True])
def test_msa_columns(banded):
    for inserted, cols in ((12, 161), (11, 160)):
        w = W.insertion_window([20, 20], inserted=inserted)
        big = W.run_oracle(w, banded=banded, msa=True)
        assert big.status == 0 and {len(row) for row in big.msa} == {cols}
        first_ok = min(C for C in range(cols - 3, cols + 4)
                       if W.run_oracle(w, banded=banded, msa=True, max_cons=C, want_graph=False).status == 0)
        assert first_ok == cols + 1
        for C in (cols, cols + 1):
            r = W.run_oracle(w, banded=banded, msa=True, max_cons=C, want_graph=False)
            assert r.status == (2 if msa_rule(cols, C) else 0)
        # the consensus of the same window is far from its limit
        assert W.run_oracle(w, banded=banded, max_cons=161).status == 0


# ---- empty graphs, the loop bounds ------------------------------------------------------------

@pytest.mark.parametrize("banded", [False, True])
def test_empty_graph(banded):
    for reads in ([b""], [b"", b""]):
        assert loop_rule(0, 0)
        assert W.run_oracle(reads, banded=banded).status == 7
        m = W.run_oracle(reads, banded=banded, msa=True)
        assert m.status == 0 and m.msa == [""] * len(reads)
    r = W.run_oracle([b"", W.BACKBONE], banded=banded)
    assert r.status == 0 and r.consensus == W.BACKBONE.decode()


def test_traceback_loop_bound():
    g = W.group("tb7")
    long_read, near = g.cases[0].reads[1], g.cases[1].reads[1]
    assert (len(long_read), len(near)) == (200, 188)
    for sbits, scores in ((16, W.GAP0), (32, W.GAP0_WIDE)):
        assert S.ref_score_bits(g.max_seq, *scores, graph_dim=g.max_nodes) == sbits
        kw = dict(banded=True, score_bits=sbits, scores=scores, max_nodes=g.max_nodes)
        assert W.run_oracle([long_read[:2], long_read], **kw).status == 7
        r = W.run_oracle([long_read[:2], near], **kw)
        assert r.status == 0 and r.consensus
    # the full alignment, and the default scores in the band, end both windows normally
    for kw in (dict(banded=False, scores=W.GAP0), dict(banded=True, scores=W.DEFAULT)):
        assert [W.run_oracle(c.reads, max_nodes=g.max_nodes, **kw).status for c in g.cases[:2]] == [0, 0]


def test_traceback_status_7_search():
    """A bounded search for other windows whose traceback runs into its loop
    bound: length-skewed windows (prefixes, suffixes, unrelated reads, a doubled
    backbone, long deletions, in a random order, so that a short read may be
    the backbone) under every score set of poa_score_sets.py, banded 128 and
    256 and the full alignment.  What it finds is one family: a graph of one or
    two nodes under a read whose end lies outside the band, with gap 0 or match
    0 (group "tb7" is its plainest member).  Anything else is a new case for
    test_poa_limits.py."""
    sets = sorted(S.ALL.items())
    found = []
    runs = 0
    for seed in range(300):
        rng = random.Random(seed)
        blen = rng.choice((120, 180, 250))
        bb = bytes(rng.choice(b"ACGT") for _ in range(blen))
        reads = [bb]
        for _ in range(rng.randrange(2, 8)):
            kind = rng.randrange(5)
            if kind == 0:
                r = bb[:rng.randrange(1, 40)]
            elif kind == 1:
                r = bb[rng.randrange(blen - 40, blen - 1):]
            elif kind == 2:
                r = bytes(rng.choice(b"ACGT") for _ in range(rng.randrange(1, 250)))
            elif kind == 3:
                r = (bb + bb)[:250]
            else:
                a = rng.randrange(0, blen // 2)
                r = bb[:a] + bb[a + rng.randrange(20, blen // 2):]
            reads.append(r)
        rng.shuffle(reads)
        for name, (gap, mismatch, match) in (sets[seed % len(sets)], sets[(seed // len(sets) + 7 * seed) % len(sets)]):
            for banded, bw in ((True, 128), (True, 256), (False, 256)):
                if not banded and gap > 0:
                    continue
                r = oracle.poa_window(reads, gap=gap, mismatch=mismatch, match=match, banded=banded, band_width=bw,
                                      max_nodes=1024, max_consensus=512, max_seqs=64)
                runs += 1
                assert r.status in (0, 7), (seed, name, banded, bw)
                if r.status == 7:
                    found.append((seed, name, banded, bw, len(reads[0]), gap, match))
    assert runs > 1500 and found  # (the search can find what it looks for)
    for seed, name, banded, bw, len0, gap, match in found:
        assert banded and len0 <= 2 and (gap == 0 or match == 0), (seed, name, bw)
