"""The full-alignment LDS kernel's row order between two reads: the previous
order with the read's new nodes spliced in (order_splice, poa_order.hpp)
instead of a Kahn sort after every read.

* The routine alone (gwamd_internal_order_splice): random DAGs with an old
  topological order and a path through them; the host checks the new order.
* Whole windows: status, consensus, coverage (or MSA rows) and the final graph
  bit for bit against the oracle, under the default and under
  GWAMD_POA_ORDER=kahn (a sort after every read), which must agree too.
* Every test meant to cover the splice asserts through the per-window counters
  (CudaPoaBatch.get_order_stats) that every window spliced at least one read;
  the tie and fallback tests assert their own counters.
"""
import ctypes as C
import random

import numpy as np
import pytest

from claragenomicsanalysis_amd import load_library, synth
from claragenomicsanalysis_amd.cudapoa import CudaPoaBatch
from oracle import oracle

MEM = 8 << 30
ST = {name: i for i, name in enumerate(CudaPoaBatch.ORDER_STATS)}
# one of these is counted for every read after the first: it was spliced, or sorted for that cause
PER_READ = [i for name, i in ST.items() if name == "spliced" or name.startswith("sort_")]


# ---------------------------------------------------------------------------
# the routine alone

def _splice(V, n, sorted_old, curr, kind, threads):
    L = load_library()
    L.gwamd_internal_order_splice.restype = C.c_int
    L.gwamd_internal_order_splice.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                              C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.c_int]
    so = np.full(n, -1, np.int32)
    so[:V] = sorted_old
    po = np.full(n, -1, np.int32)
    cu = np.asarray(curr, np.int32)
    ki = np.asarray(kind, np.uint8)
    p32 = C.POINTER(C.c_int32)
    rc = L.gwamd_internal_order_splice(V, n, len(cu), so.ctypes.data_as(p32), po.ctypes.data_as(p32),
                                       cu.ctypes.data_as(p32), ki.ctypes.data_as(C.POINTER(C.c_uint8)), threads)
    return rc, so, po


def _case(rng, V, L, layout, cap=10 ** 6):
    """A random DAG on V old nodes with a random topological order, and a path of
    L read positions over it.  layout: which positions are new nodes (at most cap)."""
    order = list(range(V))
    rng.shuffle(order)
    rank = {v: r for r, v in enumerate(order)}
    edges = set()
    for r in range(1, V):  # every old node but the first gets 1-3 predecessors of lower rank
        for _ in range(rng.randrange(1, 4)):
            edges.add((order[rng.randrange(max(0, r - 12), r)], order[r]))
    if layout == "none":
        new = [False] * L
    elif layout == "all":
        new = [True] * L
    elif layout == "front":
        k = min(cap, max(1, L // 3))
        new = [i < k for i in range(L)]
    elif layout == "end":
        k = min(cap, max(1, L // 3))
        new = [i >= L - k for i in range(L)]
    elif layout == "middle":
        k = min(cap, max(1, L // 3))
        new = [L // 3 <= i < L // 3 + k for i in range(L)]
    else:  # mixed: runs of random lengths, new nodes at both ends
        new, i = [], 0
        while len(new) < L:
            new += [i % 2 == 0] * rng.randrange(1, 6)
            i += 1
        new = new[:L]
        new[-1] = True
        inner = [i for i in range(1, L - 1) if new[i]]
        rng.shuffle(inner)
        for i in inner[:max(0, new.count(True) - cap)]:
            new[i] = False
    n_old = new.count(False)
    assert n_old <= V
    old_ranks = sorted(rng.sample(range(V), n_old))
    curr, kind, nxt, oi = [], [], V, 0
    for i in range(L):
        if new[i]:
            curr.append(nxt)
            kind.append(rng.choice((2, 3, 2 | 4)))
            nxt += 1
        else:
            curr.append(order[old_ranks[oi]])
            kind.append(rng.choice((0, 1, 4, 5)))
            oi += 1
    for a, b in zip(curr, curr[1:]):
        edges.add((a, b))
    return order, rank, edges, curr, kind, nxt


def _check_spliced(V, n, order, edges, curr, kind, so, po):
    assert sorted(so.tolist()) == list(range(n)), "not a permutation"
    assert all(po[so[r]] == r for r in range(n)), "pos is not the inverse of sorted"
    for a, b in edges:
        assert po[a] < po[b], ("edge goes down", a, b)
    kept = [v for v in so.tolist() if v < V]
    assert kept == list(order), "old nodes changed their relative order"
    # every run directly behind its anchor; a leading run directly in front of the first old path node
    isnew = [(k & 3) >= 2 for k in kind]
    i, L = 0, len(curr)
    while i < L:
        if not isnew[i]:
            i += 1
            continue
        j = i
        while j < L and isnew[j]:
            j += 1
        if i > 0:
            base = po[curr[i - 1]] + 1
        else:
            base = po[curr[j]] - (j - i)
        assert [po[curr[t]] for t in range(i, j)] == list(range(base, base + j - i)), ("run placement", i, j)
        i = j


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 63, 64, 65, 127, 128, 129, 257])
def test_routine_path_lengths(L):
    rng = random.Random(100 + L)
    for layout in ("mixed", "front", "middle", "end", "none"):
        for threads in (64, 128, 256):
            V = rng.randrange(max(L, 2), 281) if L < 257 else 290  # n = V + new nodes <= 300
            order, rank, edges, curr, kind, n = _case(rng, V, L, layout, cap=300 - V)
            assert n <= 300
            rc, so, po = _splice(V, n, order, curr, kind, threads)
            if n - V == L:  # (L = 1: the one position is a new node, with no old node to anchor to)
                assert rc == 2 and so[:V].tolist() == list(order), (layout, threads, rc)
                continue
            assert rc == 0, (layout, threads, rc)
            if n == V:
                assert so.tolist() == list(order)
            _check_spliced(V, n, order, edges, curr, kind, so, po)


@pytest.mark.gpu
def test_routine_no_new_node_and_every_node_new():
    rng = random.Random(5)
    # no new node: the order stands, nothing is written
    order, rank, edges, curr, kind, n = _case(rng, 200, 150, "none")
    rc, so, po = _splice(200, n, order, curr, kind, 128)
    assert rc == 0 and n == 200 and so.tolist() == list(order)
    # every node new: no old node to anchor to, declined, nothing written
    order, rank, edges, curr, kind, n = _case(rng, 50, 70, "all")  # (n = 120)
    rc, so, po = _splice(50, n, order, curr, kind, 128)
    assert rc == 2
    assert so[:50].tolist() == list(order) and (so[50:] == -1).all()
    assert all(po[v] == rank[v] for v in range(50)) and (po[50:] == -1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("L", [65, 200])
def test_routine_out_of_order_sibling_declines(L):
    rng = random.Random(9 + L)
    order, rank, edges, curr, kind, n = _case(rng, 250, L, "mixed", cap=50)
    olds = [i for i, k in enumerate(kind) if (k & 3) < 2]
    # one old position lands on a node ranked below the old node before it
    i = olds[len(olds) // 2]
    prev = rank[curr[olds[len(olds) // 2 - 1]]]
    on_path = set(curr)
    lower = [order[r] for r in range(prev) if order[r] not in on_path]
    curr[i], kind[i] = lower[-1], 1
    rc, so, po = _splice(250, n, order, curr, kind, 128)
    assert rc == 1
    assert so[:250].tolist() == list(order) and (so[250:] == -1).all()
    assert all(po[v] == rank[v] for v in range(250)) and (po[250:] == -1).all()


# ---------------------------------------------------------------------------
# whole windows against the oracle

def _mutate(rng, seq, length, sub=0.04, alphabet="ACGT"):
    off = rng.randrange(0, len(seq) - length + 1)
    r = list(seq[off:off + length])
    for i in range(len(r)):
        if rng.random() < sub:
            r[i] = rng.choice(alphabet)
    for _ in range(length // 60):
        r.insert(rng.randrange(len(r)), rng.choice(alphabet))
        del r[rng.randrange(len(r))]
    return "".join(r).encode()


def _snapshot(b, msa):
    graphs, gst = b.get_graphs()
    gs = [({e: g.weight(*e) for e in g.edges}, {v: g.label(v) for v in g.nodes}) for g in graphs]
    if msa:
        rows, st = b.get_msa()
        return [(st[i], rows[i], gs[i]) for i in range(len(st))]
    cons, cov, st = b.get_consensus()
    return [(st[i], cons[i], cov[i], gs[i]) for i in range(len(st))]


def _expect(wins, max_seq, max_seqs, msa=False, score_bits=16, wts=None, max_nodes=None):
    mn = (3 * max_seq + 3) // 4 * 4 if max_nodes is None else max_nodes
    out = []
    for i, w in enumerate(wins):
        ww = None
        if wts is not None:
            ww = [np.ones(len(r), np.int8) if x is None else x for x, r in zip(wts[i], w)]
        r = oracle.poa_window(w, weights=ww, msa=msa, score_bits=score_bits, max_nodes=mn, max_consensus=2 * max_seq,
                              max_seqs=max_seqs, want_graph=True)
        g = ({}, {})
        if r.status == 0:
            edges = {(src, v): wt for v, ins in enumerate(r.graph["in"]) for (src, wt) in ins}
            g = (edges, {v: r.graph["bases"][v] for v in sorted({x for e in edges for x in e})})
        out.append((r.status, r.msa, g) if msa else (r.status, r.consensus, r.coverage, g))
    return out


def _env(monkeypatch, shape, kahn, slots=None, keep_add=False):
    monkeypatch.delenv("GWAMD_POA_KERNEL", raising=False)
    if not keep_add:
        monkeypatch.delenv("GWAMD_POA_ADD", raising=False)
    monkeypatch.delenv("GWAMD_TOPSORT", raising=False)
    monkeypatch.setenv("GWAMD_DIAG", "1")
    if shape is None:
        monkeypatch.delenv("GWAMD_POA_LDS_SHAPE", raising=False)
    else:
        monkeypatch.setenv("GWAMD_POA_LDS_SHAPE", shape)
    if kahn:
        monkeypatch.setenv("GWAMD_POA_ORDER", "kahn")
    else:
        monkeypatch.delenv("GWAMD_POA_ORDER", raising=False)
    if slots is None:
        monkeypatch.delenv("GWAMD_POA_SLOTS", raising=False)
    else:
        monkeypatch.setenv("GWAMD_POA_SLOTS", str(slots))


def _both_orders(monkeypatch, shape, wins, max_seq, max_seqs, score_bits=16, out="consensus", wts=None, slots=None,
                 generates=1, keep_add=False, **kw):
    """The windows under the spliced order and under a sort per read: both equal
    the oracle (and so each other).  Returns the spliced run's counters."""
    expect = _expect(wins, max_seq, max_seqs, msa=out == "msa", score_bits=score_bits, wts=wts,
                     max_nodes=kw.get("max_nodes_per_window"))
    stats = None
    for kahn in (False, True):
        _env(monkeypatch, shape, kahn, slots, keep_add)
        b = CudaPoaBatch(max_seqs, max_seq, MEM, output_type=out, alignment_band_width=256 if max_seq >= 256 else 128,
                         **kw)
        for i, w in enumerate(wins):
            st, _ = b.add_poa_group(list(w), weights=None if wts is None else wts[i])
            assert st == 0
        for rep in range(generates):
            b.generate_poa()
            assert b.kernel_variant() == 2 and b.get_types()[0] == score_bits
            for i, (g, e) in enumerate(zip(_snapshot(b, out == "msa"), expect)):
                assert g == e, (shape, "kahn" if kahn else "splice", rep, i)
            s = b.get_order_stats()
            if kahn:
                assert not s.any(), "GWAMD_POA_ORDER=kahn sorts after every read and counts nothing"
            else:
                stats = s
    return stats, expect


def _windows(seed, count, lo=60, hi=300, reads=(6, 12)):
    rng = random.Random(seed)
    wins = []
    for _ in range(count):
        n = rng.randrange(lo, hi + 1)
        bb = "".join(rng.choice("ACGT") for _ in range(n + 10))
        wins.append([bb[:n].encode()] + [_mutate(rng, bb, rng.randrange(max(lo, n - 40), n + 1), sub=0.06)
                                         for _ in range(rng.randrange(reads[0] - 1, reads[1]))])
    return wins


@pytest.mark.gpu
@pytest.mark.parametrize("shape,score_bits,max_seq", [("8,2", 16, 320), ("8,1", 16, 320), ("8,4", 16, 320),
                                                      ("8,2", 32, 1500)])
def test_windows_match_oracle(shape, score_bits, max_seq, monkeypatch):
    wins = _windows(40 + score_bits + int(shape[-1]), 5)
    stats, _ = _both_orders(monkeypatch, shape, wins, max_seq, 12, score_bits=score_bits)
    assert (stats[:, ST["spliced"]] >= 1).all(), stats
    # every read but the last is spliced or sorted for a counted cause; the last one sorts
    causes = stats[:, PER_READ].sum(axis=1)
    assert causes.tolist() == [len(w) - 1 for w in wins], stats
    assert (stats[:, ST["sort_last_read"]] == 1).all(), stats


@pytest.mark.gpu
def test_persistent_grid_two_generates(monkeypatch):
    wins = _windows(77, 8, lo=60, hi=120, reads=(6, 8))
    stats, _ = _both_orders(monkeypatch, "8,2", wins, 130, 8, slots=3, generates=2)
    assert (stats[:, ST["spliced"]] >= 1).all(), stats


@pytest.mark.gpu
@pytest.mark.parametrize("out", ["consensus", "msa"])
def test_weights_and_msa(out, monkeypatch):
    wins = _windows(91, 4, lo=100, hi=300, reads=(6, 8))
    wrng = np.random.default_rng(3)
    wts = [[None if j % 4 == 3 else wrng.integers(0, 61, size=len(r), dtype=np.int8) for j, r in enumerate(w)]
           for w in wins]
    stats, _ = _both_orders(monkeypatch, "8,2", wins, 320, 8, out=out, wts=wts)
    assert (stats[:, ST["spliced"]] >= 1).all(), stats


@pytest.mark.gpu
def test_edge_windows(monkeypatch):
    """Single-read windows, one-base and empty reads, the node limit."""
    rng = random.Random(7)
    bb = "".join(rng.choice("ACGT") for _ in range(100))
    ok = [bb.encode()] + [_mutate(rng, bb, 90 + k) for k in range(5)]
    wins = [[ok[0]], [ok[0], b"", ok[1], ok[2]], [ok[0], ok[3], b"G", ok[4], b"", ok[1]], ok, [ok[2], ok[0], b"A"]]
    wins += synth.poa_windows(61, 3, 100, 8, 20, 20, 20)
    stats, expect = _both_orders(monkeypatch, "8,2", wins, 130, 8, max_nodes_per_window=140)
    assert any(e[0] == 4 for e in expect) and any(e[0] == 0 for e in expect)
    assert not stats[0].any()  # one read: no sort at all
    assert stats[2, ST["sort_empty_read"]] == 1 and stats[2, ST["spliced"]] >= 1, stats
    assert stats[3, ST["spliced"]] >= 1, stats


@pytest.mark.gpu
def test_sink_ties(monkeypatch):
    """Reads that end in different last bases and in trailing insertions leave
    several sinks; a later read that matches none of the ends scores the same on
    them, and the reference's choice among them is the Kahn order's."""
    rng = random.Random(21)
    wins = []
    for k in range(6):
        n = 80 + 7 * k
        core = "".join(rng.choice("ACGT") for _ in range(n))
        ends = ["A", "C", "G", "CA", "GAC", "T"]
        rng.shuffle(ends)
        reads = [(core + "A").encode()]
        for e in ends[:4]:
            reads.append((_mutate(rng, core + "A", n + 1, sub=0.03).decode()[:n] + e).encode())
        # matches none of the ends: the core only, then the core with another tail
        reads.append(core.encode())
        reads.append((core[:n - 1] + "T" + "TT").encode())
        reads.append(_mutate(rng, core + "A", n, sub=0.03))
        wins.append(reads)
    stats, _ = _both_orders(monkeypatch, "8,2", wins, 130, 10)
    assert (stats[:, ST["spliced"]] >= 1).all(), stats
    # ends that share their one predecessor are told apart by its out-list, the others by a Kahn sort,
    # after which the window sorts per read while the tie lasts
    assert stats[:, ST["tie_sorts"]].sum() >= 1 and stats[:, ST["tie_quick"]].sum() >= 1, stats
    assert stats[:, ST["sort_after_tie"]].sum() >= 1, stats
    stats_w, _ = _both_orders(monkeypatch, "8,2", wins[:2], 1500, 10, score_bits=32)
    assert (stats_w[:, ST["spliced"]] >= 1).all(), stats_w
    # the round-3 packed pass (nw_forward_lds_pk): its spilled sink rows feed the same tie check
    monkeypatch.setenv("GWAMD_POA_FWD", "v1")
    stats_p, _ = _both_orders(monkeypatch, "8,2", wins, 130, 10)
    monkeypatch.delenv("GWAMD_POA_FWD")
    assert (stats_p == stats).all(), (stats_p, stats)
    # more sinks than the tie check holds (GWAMD_POA_SINK_CAP=2 instead of 64): the window sorts once
    # under the spliced order and stops splicing
    monkeypatch.setenv("GWAMD_POA_SINK_CAP", "2")
    stats_c, _ = _both_orders(monkeypatch, "8,2", wins, 130, 10)
    monkeypatch.delenv("GWAMD_POA_SINK_CAP")
    assert (stats_c[:, ST["spliced"]] >= 1).all() and (stats_c[:, ST["sort_sink_cap"]] <= 1).all(), stats_c
    assert stats_c[:, ST["sort_sink_cap"]].sum() >= 1, stats_c


@pytest.mark.gpu
def test_fallback_sequential_add(monkeypatch):
    """The dense two-letter windows of test_poa_add_waves.py.  A read whose graph
    update ran sequentially is sorted, not spliced.

    Measured with these counters: the every-wave update's conflict return is
    not taken by this set (0 of 144 reads), nor by any of 54 variations of it
    (alphabets AC, AAAC, ACG; 15-45 % substitutions; 0-10 indel pairs; 9 and 20
    reads per window: 0 of 12,528 reads), so the sequential update is forced
    here with GWAMD_POA_ADD=serial and =wave0."""
    rng = random.Random(11)
    wins = []
    for k in range(16):
        n = 60 + 4 * k
        bb = "".join(rng.choice("AC") for _ in range(n + 10))
        wins.append([bb[:n].encode()] + [_mutate(rng, bb, rng.randrange(60, n + 1), sub=0.28, alphabet="AC")
                                         for _ in range(9)])
    reads = [len(w) - 1 for w in wins]
    stats, _ = _both_orders(monkeypatch, "8,2", wins, 130, 10)
    assert stats[:, PER_READ].sum(axis=1).tolist() == reads, stats
    assert (stats[:, ST["spliced"]] >= 1).all(), stats
    for mode in ("serial", "wave0"):
        monkeypatch.setenv("GWAMD_POA_ADD", mode)
        stats, _ = _both_orders(monkeypatch, "8,2", wins, 130, 10, keep_add=True)
        assert stats[:, ST["sort_seq_add"]].tolist() == reads and not stats[:, ST["spliced"]].any(), (mode, stats)
    monkeypatch.delenv("GWAMD_POA_ADD")


@pytest.mark.gpu
def test_fallback_order_check(monkeypatch):
    """A read base that lands on an aligned sibling ranked below the path's
    previous old node: the order check declines and the read is sorted.

    Read 1 substitutes G for the backbone's A and then inserts bases, so that
    G (a new node, aligned to A) and the insertion are spliced in behind A's
    predecessor while A's successors keep their ranks; read 2 makes more such
    siblings; the later reads walk backbone -> sibling -> backbone."""
    rng = random.Random(31)
    wins = []
    for k in range(10):
        n = 70 + 5 * k
        bb = [rng.choice("ACGT") for _ in range(n)]
        reads = ["".join(bb)]
        for _ in range(3):
            r = list(bb)
            for p in rng.sample(range(5, n - 5), 6):
                r[p] = rng.choice([c for c in "ACGT" if c != bb[p]])
            ins = rng.randrange(10, n - 10)
            r[ins:ins] = [rng.choice("ACGT") for _ in range(rng.randrange(1, 4))]
            reads.append("".join(r))
        for _ in range(5):
            # recombine the earlier reads base by base: paths that hop between siblings
            r = list(bb)
            for p in range(n):
                src = rng.choice(reads[1:4])
                if len(src) > p and rng.random() < 0.5:
                    r[p] = src[p]
            reads.append("".join(r))
        wins.append([x.encode() for x in reads])
    stats, _ = _both_orders(monkeypatch, "8,2", wins, 130, 10)
    assert (stats[:, ST["spliced"]] >= 1).all(), stats
    assert stats[:, ST["sort_order_check"]].sum() >= 1, stats


# ---------------------------------------------------------------------------
# the row program on every wave against the one-wave build

def _row_programs(n, base, in_lists, order, xl_cap, ring_rows, threads):
    """(records, lists + sink words) of the one-wave build and of the every-wave build."""
    L = load_library()
    p32, pu8, pu16 = C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_uint16)
    L.gwamd_internal_row_program.restype = C.c_int
    L.gwamd_internal_row_program.argtypes = [C.c_int, pu8, pu16, pu16, p32, p32, C.c_int, C.c_int, C.c_int,
                                             C.POINTER(C.c_uint32), pu16]
    in_cnt = np.array([len(x) for x in in_lists], np.uint16)
    out_cnt = np.zeros(n, np.uint16)
    in_e = np.zeros((n, 50), np.int32)
    for v, preds in enumerate(in_lists):
        for k, p in enumerate(preds):
            in_e[v, k] = p
            out_cnt[p] += 1
    b = np.asarray(base, np.uint8)
    so = np.asarray(order, np.int32)
    rec = np.zeros((2, n + 2), np.uint32)
    xl = np.zeros((2, xl_cap + 72), np.uint16)
    rc = L.gwamd_internal_row_program(n, b.ctypes.data_as(pu8), in_cnt.ctypes.data_as(pu16),
                                      out_cnt.ctypes.data_as(pu16), in_e.ctypes.data_as(p32), so.ctypes.data_as(p32),
                                      xl_cap, ring_rows, threads, rec.ctypes.data_as(C.POINTER(C.c_uint32)),
                                      xl.ctypes.data_as(pu16))
    assert rc == 0, rc
    return rec, xl, int((out_cnt == 0).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("n,xl_cap,threads", [(200, 1024, 128), (256, 1024, 128), (257, 1024, 128), (700, 1024, 128),
                                              (700, 1024, 64), (1300, 4096, 256), (1300, 512, 128), (2300, 4096, 128),
                                              (2300, 4096, 512)])
def test_row_program_every_wave_equals_one_wave(n, xl_cap, threads):
    """Records, predecessor lists, the 0x80 and bit-15 marks, the escaped lists (a
    list region too small for the graph) and the sink list: byte for byte."""
    rng = random.Random(n + xl_cap + threads)
    order = list(range(n))
    rng.shuffle(order)
    in_lists = [[] for _ in range(n)]
    for r in range(1, n):
        v = order[r]
        if rng.random() < 0.02:
            continue  # a source
        k = 1 if rng.random() < 0.7 else rng.randrange(2, 7)
        lo = 0 if rng.random() < 0.1 else max(0, r - 6)  # some predecessors beyond an 8-row ring
        in_lists[v] = list(dict.fromkeys(order[rng.randrange(lo, r)] for _ in range(k)))
    base = [rng.choice(b"ACGT") if rng.random() < 0.95 else rng.choice([ord("N"), 0x7f, 0x80, 0xff, ord("a")])
            for _ in range(n)]
    rec, xl, nsinks = _row_programs(n, base, in_lists, order, xl_cap, 8, threads)
    assert rec[0].any() and xl[0, :xl_cap].any()
    assert (rec[0] == rec[1]).all(), np.nonzero(rec[0] != rec[1])[0][:8]
    assert (xl[0] == xl[1]).all(), np.nonzero(xl[0] != xl[1])[0][:8]
    # what the cases are meant to reach: sinks listed and counted, spilled rows, general-path rows, escapes
    assert xl[0, xl_cap + 64] == nsinks and nsinks >= 2
    assert (rec[0] >> 15 & 1).any() and (rec[0] & 0x80).any()
    escaped = ((rec[0] >> 8) & 63) == 63
    assert escaped.any() == (xl_cap == 512)
