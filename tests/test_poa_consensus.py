"""Parity tests of the wave-wide, LDS-resident consensus (consensus_lds in
csrc/poa_consensus.hpp) against the lane-0 HBM path it replaces
(consensus_raw, csrc/poa_device.hpp) and the CPU restatement of the reference
(oracle/poa_oracle.cpp consensus_raw, oracle.poa_window):

1. the reference's generate-consensus known answers (tests/golden/poa_kat.json,
   from Test_CudapoaGenerateConsensus.cu) through the C-ABI test hook;
2. 300 random DAGs through the hook (most take weight ties, a third enter
   branch completion; both counts are recomputed here and required);
3. the edges of the rule: one node, chains across the 64-lane groups of the
   emit step, the consensus-length limit, and the LDS fit limit by one byte
   and by one edge;
4. whole windows on the LDS kernel and the banded kernel against
   oracle.poa_window, with the default path, with GWAMD_CONSENSUS=hbm and with
   GWAMD_CONSENSUS_LDS_BYTES pushing the larger graphs of a batch to HBM;
5. (no GPU) the fit function against the layout's byte count.

Expected values come from the oracle only."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

from claragenomicsanalysis_amd import load_library, synth
from claragenomicsanalysis_amd.cudapoa import CudaPoaBatch
from oracle import oracle

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "poa_kat.json")))
MAX_EDGES = 50
MEM = 8 << 30
gpu = pytest.mark.gpu


# ---------------------------------------------------------------------------
# graphs as the reference's fixed-slot arrays
class SlotGraph:
    def __init__(self, n):
        self.n = n
        self.base = np.zeros(n, np.uint8)
        self.sorted = np.zeros(n, np.int32)
        self.pos = np.zeros(n, np.int32)
        self.in_cnt = np.zeros(n, np.uint16)
        self.in_e = np.zeros(n * MAX_EDGES, np.int32)
        self.in_w = np.zeros(n * MAX_EDGES, np.uint16)
        self.out_cnt = np.zeros(n, np.uint16)
        self.out_e = np.zeros(n * MAX_EDGES, np.int32)
        self.aln_cnt = np.zeros(n, np.uint16)
        self.aln = np.zeros(n * MAX_EDGES, np.int32)
        self.cov = np.zeros(n, np.uint16)

    def set_order(self, order):
        self.sorted[:] = order
        for p, v in enumerate(order):
            self.pos[v] = p

    def add_edge(self, u, v, w):
        self.in_e[v * MAX_EDGES + int(self.in_cnt[v])] = u
        self.in_w[v * MAX_EDGES + int(self.in_cnt[v])] = w
        self.in_cnt[v] += 1
        self.out_e[u * MAX_EDGES + int(self.out_cnt[u])] = v
        self.out_cnt[u] += 1

    @property
    def m(self):
        return int(self.in_cnt.sum())

    def arrays(self):
        return (self.base, self.sorted, self.pos, self.in_cnt, self.in_e, self.in_w, self.out_cnt, self.out_e,
                self.aln_cnt, self.aln, self.cov)


def kat_graph(case):
    """Input construction of the reference test, as oracle.consensus_raw does
    (Test_CudapoaGenerateConsensus.cu:30-75: the weight of edge i->o sits at
    slot index i of node o)."""
    n = len(case["nodes"])
    g = SlotGraph(n)
    g.in_cnt, g.in_e, g.out_cnt, g.out_e = oracle.edges_from_lists(case["outgoing"], n)
    for i, outs in enumerate(case["outgoing"]):
        for j, o in enumerate(outs):
            g.in_w[o * MAX_EDGES + i] = case["weights"][i][j]
    g.base[:] = np.frombuffer(case["nodes"].encode(), np.uint8)
    g.set_order(case["sorted"])
    for i, al in enumerate(case["aligned"]):
        for j, x in enumerate(al):
            g.aln[i * MAX_EDGES + j] = x
            g.aln_cnt[i] += 1
    g.cov[:] = case["coverage"]
    return g


def random_graph(seed):
    """Rank r >= 1 takes predecessor r-1 with probability 0.9 and r-d, d = 2..6,
    with probability 0.15 each; the candidates are shuffled, at most 8 kept,
    weights from {1, 2, 3}; node ids are a random permutation of the ranks."""
    rs = np.random.RandomState(seed)
    n = int(rs.randint(1, 301))
    g = SlotGraph(n)
    order = rs.permutation(n)
    g.set_order(order)
    g.base[:] = np.frombuffer(b"ACGT", np.uint8)[rs.randint(0, 4, n)]
    for r in range(1, n):
        cand = [r - 1] if rs.rand() < 0.9 else []
        for d in range(2, 7):
            if rs.rand() < 0.15 and r - d >= 0:
                cand.append(r - d)
        rs.shuffle(cand)
        for p in cand[:8]:
            g.add_edge(int(order[p]), int(order[r]), int(rs.randint(1, 4)))
    g.cov[:] = rs.randint(0, 60000, n)  # (sums over aligned nodes wrap in uint16)
    for v in range(n):
        if n > 4 and rs.rand() < 0.2:
            k = int(rs.randint(1, 4))
            others = rs.choice(n, k, replace=False)
            g.aln[v * MAX_EDGES:v * MAX_EDGES + k] = others
            g.aln_cnt[v] = k
    return g


def chain_graph(n, extra_edge=False):
    g = SlotGraph(n)
    g.set_order(np.arange(n))
    g.base[:] = np.frombuffer(b"ACGT", np.uint8)[np.arange(n) % 4]
    g.cov[:] = 1 + np.arange(n) % 7
    for v in range(1, n):
        g.add_edge(v - 1, v, 2)
    if extra_edge:
        g.add_edge(0, n - 1, 1)
    return g


def restate(g):
    """The scoring rule in Python (cudapoa_generate_consensus.cuh:279-347), to
    classify a case: (entered branch completion, took a weight tie)."""
    score = [-1] * g.n
    pred = [-1] * g.n
    tie = False
    max_id, max_score = 0, -1
    for r in range(g.n):
        v = int(g.sorted[r])
        s = -1
        for e in range(int(g.in_cnt[v])):
            w, b = int(g.in_w[v * MAX_EDGES + e]), int(g.in_e[v * MAX_EDGES + e])
            if s == w:
                tie = True
            if s < w or (s == w and score[pred[v]] <= score[b]):
                s, pred[v] = w, b
        if pred[v] != -1:
            s += score[pred[v]]
        if max_score <= s:
            max_id, max_score = v, s
        score[v] = s
    return int(g.out_cnt[max_id]) != 0, tie


# ---------------------------------------------------------------------------
# the device hook and the oracle on the same arrays
def _hook():
    L = load_library()
    f = L.gwamd_internal_consensus
    f.restype = C.c_int
    f.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 11 + [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 4
    return f


def device_consensus(g, max_cons=2048, force_hbm=False, scratch=64 << 10, size_bits=16):
    """(path, status, consensus bytes, coverage list): path 1 = LDS, 0 = HBM."""
    st = np.zeros(1, np.int32)
    ln = np.zeros(1, np.int32)
    cons = np.zeros(max_cons, np.uint8)
    cov = np.zeros(max_cons, np.uint16)
    path = _hook()(size_bits, g.n, *[a.ctypes.data for a in g.arrays()], max_cons, int(force_hbm), scratch,
                   st.ctypes.data, ln.ctypes.data, cons.ctypes.data, cov.ctypes.data)
    assert path in (0, 1), path
    n = int(ln[0])
    return path, int(st[0]), bytes(cons[:n]), cov[:n].tolist()


def oracle_consensus(g, max_cons=2048):
    """(status, consensus bytes, coverage list) in host order; empty on an error."""
    cons = np.zeros(max_cons + 1, np.uint8)
    cov = np.zeros(max_cons + 1, np.uint16)
    st = oracle.lib().oracle_consensus_raw(g.n, *[oracle._p(a) for a in g.arrays()], max_cons, oracle._p(cons),
                                           oracle._p(cov))
    if st != 0:
        return st, b"", []
    raw = bytes(cons).split(b"\0", 1)[0]
    return st, raw[::-1], cov[:len(raw)][::-1].tolist()


def check_both_paths(g, max_cons=2048, size_bits=16, tag=None):
    want = oracle_consensus(g, max_cons)
    lds = device_consensus(g, max_cons, size_bits=size_bits)
    hbm = device_consensus(g, max_cons, force_hbm=True, size_bits=size_bits)
    assert lds[0] == 1 and hbm[0] == 0, tag
    assert lds[1:] == want, tag
    assert hbm[1:] == want, tag
    return want


# ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("size_bits", [16, 32])
@pytest.mark.parametrize("case", GOLD["consensus"], ids=lambda c: c["answer"])
def test_consensus_kat(case, size_bits):
    # Test_CudapoaGenerateConsensus.cu:77-156; the golden answer is the raw
    # (backwards) kernel string
    g = kat_graph(case)
    st, cons, _ = check_both_paths(g, size_bits=size_bits)
    assert st == 0
    assert cons.decode() == case["answer"][::-1]


@gpu
def test_consensus_random_dags():
    entered = ties = 0
    for seed in range(300):
        g = random_graph(seed)
        bc, tie = restate(g)
        entered += bc
        ties += tie
        check_both_paths(g, size_bits=32 if seed % 10 == 0 else 16, tag=seed)
    # the generator must keep producing the hard cases
    assert entered >= 75, entered
    assert ties >= 270, ties


@gpu
@pytest.mark.parametrize("n", [1, 64, 65, 129])
def test_consensus_chains(n):
    # one node; chains ending on and just past the 64-position groups of the emit step
    st, cons, cov = check_both_paths(chain_graph(n))
    assert st == 0 and len(cons) == n and len(cov) == n


@gpu
@pytest.mark.parametrize("slack", [2, 1, 0])
def test_consensus_length_limit(slack):
    # a consensus exactly max_cons - 2, max_cons - 1 and max_cons long: the
    # last is kExceededMaxSeqSize (count >= max_cons - 1)
    n = 70
    st, cons, _ = check_both_paths(chain_graph(n), max_cons=n + slack)
    assert (st, len(cons)) == ((0, n) if slack else (2, 0))


@gpu
def test_consensus_fit_limit():
    L = load_library()
    L.gwamd_internal_consensus_lds_bytes.restype = C.c_longlong
    g = chain_graph(40)
    need = L.gwamd_internal_consensus_lds_bytes(g.n, g.m)
    want = oracle_consensus(g)
    # fits exactly / misses by one byte: the path flips, the answer does not
    fit = device_consensus(g, scratch=need)
    miss = device_consensus(g, scratch=need - 1)
    assert (fit[0], miss[0]) == (1, 0)
    assert fit[1:] == want and miss[1:] == want
    # one more edge under the same cap misses by one entry
    g2 = chain_graph(40, extra_edge=True)
    assert L.gwamd_internal_consensus_lds_bytes(g2.n, g2.m) == need + 4
    miss2 = device_consensus(g2, scratch=need)
    fit2 = device_consensus(g2, scratch=need + 4)
    assert (miss2[0], fit2[0]) == (0, 1)
    assert miss2[1:] == oracle_consensus(g2) and fit2[1:] == miss2[1:]
    # no scratch at all (the global-memory kernel's case)
    assert device_consensus(g, scratch=0)[0] == 0


# ---------------------------------------------------------------------------
# whole windows
MAX_SEQ, MAX_SEQS = 320, 8


@functools.lru_cache(maxsize=None)
def _windows():
    # (built on first use: nothing at import time loads the library)
    wins = []
    for k in (2, 3, 4):  # few reads: nearly every junction is a weight tie
        wins += synth.poa_windows(700 + k, 1, 300, k, 30, 30, 30)
    bb = bytes(synth.poa_windows(711, 1, 300, 2, 0, 0, 0)[0][0])
    # later reads are prefixes and suffixes of the backbone: the heaviest path
    # ends before a sink / starts after a source
    wins.append([bb, bb[:150], bb[:220], bb[:150]])
    wins.append([bb, bb[100:], bb[40:], bb[:260], bb[100:]])
    mut = [bytes(r) for r in synth.poa_windows(712, 1, 300, 5, 25, 25, 25)[0]]
    wins.append([mut[0], mut[1][:180], mut[2][60:], mut[3][:240], mut[4]])
    wins.append([bb])    # one read
    wins.append([b""])   # an empty window
    return [[bytes(r) for r in w] for w in wins]


def _weights(wins, seed):
    rng = np.random.default_rng(seed)
    return [[rng.integers(0, 61, size=len(r), dtype=np.int8) for r in w] for w in wins]


def _max_nodes(banded):
    return ((4 if banded else 3) * MAX_SEQ + 3) // 4 * 4


@functools.lru_cache(maxsize=None)
def _expected(banded, msa, sbits, weighted):
    wts = _weights(_windows(), 5) if weighted else [None] * len(_windows())
    return [oracle.poa_window(w, weights=ww, banded=banded, band_width=256, msa=msa, score_bits=sbits,
                              max_nodes=_max_nodes(banded), max_consensus=2 * MAX_SEQ, max_seqs=MAX_SEQS)
            for w, ww in zip(_windows(), wts)]


def _run(wins, banded, out="consensus", wts=None):
    b = CudaPoaBatch(MAX_SEQS, MAX_SEQ, MEM, output_type=out, cuda_banded_alignment=banded,
                     alignment_band_width=256)
    for i, w in enumerate(wins):
        st, _ = b.add_poa_group(list(w), weights=None if wts is None else wts[i])
        assert st == 0
    b.generate_poa()
    assert b.kernel_variant() in ((3, 4) if banded else (2,))
    return b


def _check_consensus(b, banded, weighted=False, tag=None):
    cons, cov, st = b.get_consensus()
    want = _expected(banded, False, b.get_types()[0], weighted)
    for i, r in enumerate(want):
        assert (st[i], cons[i], cov[i]) == (r.status, r.consensus, r.coverage), (tag, i)


def _set_path(monkeypatch, path):
    monkeypatch.delenv("GWAMD_CONSENSUS", raising=False)
    monkeypatch.delenv("GWAMD_CONSENSUS_LDS_BYTES", raising=False)
    if path == "hbm":
        monkeypatch.setenv("GWAMD_CONSENSUS", "hbm")
    elif path == "cap":
        # the one-read window (300 nodes, 299 edges: 4,196 bytes) still fits,
        # the windows with more reads do not
        monkeypatch.setenv("GWAMD_CONSENSUS_LDS_BYTES", "4200")


@gpu
@pytest.mark.parametrize("path", ["lds", "hbm", "cap"])
@pytest.mark.parametrize("kernel", ["lds", "band"])
def test_consensus_windows(kernel, path, monkeypatch):
    _set_path(monkeypatch, path)
    banded = kernel == "band"
    _check_consensus(_run(_windows(), banded), banded, tag=(kernel, path))


@gpu
@pytest.mark.parametrize("path", ["lds", "hbm"])
@pytest.mark.parametrize("kernel", ["lds", "band"])
def test_consensus_weighted_windows(kernel, path, monkeypatch):
    _set_path(monkeypatch, path)
    banded = kernel == "band"
    b = _run(_windows(), banded, wts=_weights(_windows(), 5))
    _check_consensus(b, banded, weighted=True, tag=(kernel, path))


@gpu
@pytest.mark.parametrize("kernel", ["lds", "band"])
def test_consensus_slot_reuse(kernel, monkeypatch):
    # 8 windows on 3 scratch slots, two generates: the LDS image that held a
    # consensus is reused by the workgroup's next window
    _set_path(monkeypatch, "lds")
    monkeypatch.setenv("GWAMD_POA_SLOTS", "3")
    banded = kernel == "band"
    assert len(_windows()) == 8
    b = _run(_windows(), banded)
    assert b.get_grid()[0] < len(_windows())
    for rep in range(2):
        if rep:
            b.generate_poa()
        _check_consensus(b, banded, tag=(kernel, rep))


@gpu
@pytest.mark.parametrize("kernel", ["lds", "band"])
def test_consensus_with_msa(kernel, monkeypatch):
    # an MSA batch that also emits the consensus: the consensus runs first in
    # the LDS the racon sort then takes
    _set_path(monkeypatch, "lds")
    banded = kernel == "band"
    b = _run(_windows(), banded, out="both")
    _check_consensus(b, banded, tag=kernel)
    rows, st = b.get_msa()
    want = _expected(banded, True, b.get_types()[0], False)
    for i, r in enumerate(want):
        assert (st[i], rows[i] if r.status == 0 else None) == (r.status, r.msa if r.status == 0 else None), i


# ---------------------------------------------------------------------------
def test_consensus_fit_function():
    # the layout: rec u32[n] | score i32[n] | edge u32[m] | pred u16[n]
    L = load_library()
    L.gwamd_internal_consensus_lds_bytes.restype = C.c_longlong
    for n, m in [(1, 0), (2, 1), (40, 39), (300, 812), (2051, 3598), (65535, 65535)]:
        need = 4 * n + 4 * n + 4 * m + 2 * n
        assert L.gwamd_internal_consensus_lds_bytes(n, m) == need
        assert L.gwamd_internal_consensus_lds_fits(n, m, need) == 1
        assert L.gwamd_internal_consensus_lds_fits(n, m, need - 1) == 0
    # the largest config-B window seen (2,051 nodes, 3,598 in-edges) leaves
    # headroom in the 40,560 bytes config B offers
    assert L.gwamd_internal_consensus_lds_bytes(2051, 3598) <= 40560 - 4096
    # ranks and edge offsets are 16-bit fields
    assert L.gwamd_internal_consensus_lds_fits(65536, 10, 1 << 30) == 0
    assert L.gwamd_internal_consensus_lds_fits(10, 65536, 1 << 30) == 0
    assert L.gwamd_internal_consensus_lds_fits(0, 0, 1 << 30) == 0
