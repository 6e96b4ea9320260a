"""GPU parity over the error statuses: every POA kernel route against the
oracle on the windows of poa_limit_windows.py, bit-exact, window by window:
status; consensus and coverage, or MSA rows; for a window that succeeds the
final graph (edges, weights, labels, node count); for an error window an
empty consensus, an empty coverage, no MSA rows and no graph.

Each test is one batch (per output type) of error windows next to their near
misses and two or three ordinary windows, so every workgroup of the persistent
grid takes good windows after windows that left early.  The statuses a batch
must hold are asserted per test, so no route passes on status 0 alone; that
the expectations hold every status in {0, 2, 4, 5, 7} is asserted on the
oracle in test_poa_limits_cpu.py.

Where status 5 is raised: the sequential update (poa_device.hpp, the
global-memory kernel and GWAMD_POA_ADD=serial), the one-wave update
(add_alignment_parallel, GWAMD_POA_ADD=wave0) and the batched update of the
LDS kernel's every-wave form and of the banded kernel
(add_alignment_parallel_batched).  Status 2 comes from the wave-wide consensus
in LDS, from lane 0's in HBM (GWAMD_CONSENSUS=hbm, the global-memory kernel)
and from the MSA's column count; status 7 from both consensus builders on an
empty graph and from the banded tracebacks (group "tb7").
"""
import ctypes as C

import numpy as np
import pytest

import poa_limit_windows as W
import poa_score_sets as S
from claragenomicsanalysis_amd import load_library
from claragenomicsanalysis_amd.cudapoa import CudaPoaBatch, CudaPoaMultiBatch
from oracle import oracle
from test_poa_multibatch import mem_for
from test_poa_scores import BAND_VARIANT, _band_env, _full_env

pytestmark = pytest.mark.gpu

MEM = 1 << 30
STATUSES = {"fan": {0, 5, 7}, "nodes": {0, 4, 5}, "cons": {0, 2, 7}, "tb7": {0, 7}}
STATUSES_MSA = {"fan": {0, 5}, "nodes": {0, 4, 5}, "cons": {0, 2}, "tb7": {0, 7}}


def wide_scores(name):
    """The default scores scaled until the reference's rule selects 32-bit rows at the group's sizes."""
    return W.X40 if name == "nodes" else W.X10


def make_batch(g, out, scores, banded, spoa=None):
    gap, mismatch, match = scores
    b = CudaPoaBatch(W.MAX_SEQS, g.max_seq, MEM, output_type=out, gap_score=gap, mismatch_score=mismatch,
                     match_score=match, cuda_banded_alignment=banded, alignment_band_width=W.BAND,
                     max_consensus_size=g.max_cons, max_nodes_per_window=g.max_nodes,
                     max_nodes_per_window_banded=g.max_nodes, spoa_accurate=spoa)
    # the capacities the batch reports are the ones the oracle is given (node capacities are rounded up to 4)
    bs = b.batch_size
    assert (bs.max_sequence_size, bs.max_consensus_size, bs.max_nodes_per_window, bs.max_nodes_per_window_banded,
            bs.alignment_band_width, bs.max_sequences_per_poa) == (g.max_seq, g.max_cons, g.max_nodes, g.max_nodes,
                                                                   W.BAND, W.MAX_SEQS)
    return b


def add_all(b, cases):
    for c in cases:
        st, seq_st = b.add_poa_group(list(c.reads))
        assert st == 0 and all(s == 0 for s in seq_st), c.name


def compare(b, cases, want, msa):
    """The batch's outputs against the oracle's WindowResults, window by window."""
    graphs, gst = b.get_graphs()
    _, fnodes = b.get_stats()
    if msa:
        rows, st = b.get_msa()
    else:
        cons, cov, st = b.get_consensus()
    assert len(st) == len(want) == len(cases)
    for i, (c, r) in enumerate(zip(cases, want)):
        assert st[i] == r.status, (c.name, st[i], r.status)
        if msa:
            assert rows[i] == (r.msa if r.status == 0 else []), c.name
        else:
            assert (cons[i], cov[i]) == (r.consensus, r.coverage), c.name
            if r.status != 0:
                assert (cons[i], cov[i]) == ("", []), c.name
        g = graphs[i]
        if r.status == 0:
            expect = {(src, v): wt for v, ins in enumerate(r.graph["in"]) for (src, wt) in ins}
            assert gst[i] == 0 and {(u, v): g.weight(u, v) for (u, v) in g.edges} == expect, c.name
            assert "".join(g.label(v) for v in g.nodes) == "".join(r.graph["bases"][v] for v in g.nodes), c.name
            assert fnodes[i] == r.final_nodes, c.name
        else:
            assert gst[i] == r.status and g.number_of_nodes() == 0, c.name


def check(name, banded=False, out="consensus", scores=W.DEFAULT, spoa=False, variant=None, generates=1):
    """One batch of group `name` against the oracle; returns the batch."""
    g = W.group(name)
    msa = out == "msa"
    b = make_batch(g, out, scores, banded, spoa=spoa)
    add_all(b, g.cases)
    sbits, zbits = b.get_types()
    assert (sbits, zbits) == (S.ref_score_bits(g.max_seq, *scores, graph_dim=g.max_nodes), 16)
    want = W.oracle_results(name, banded, msa, sbits, scores, spoa)
    assert {r.status for r in want} == (STATUSES_MSA if msa else STATUSES)[name]
    for _ in range(generates):
        b.generate_poa()
        compare(b, g.cases, want, msa)
    if variant is not None:
        assert b.kernel_variant() == variant
    return b


# ---- routes ------------------------------------------------------------------------------

# LDS kernel: forward-pass shape, and the packed pass (GWAMD_POA_FWD=v1) or the row-program pass (the
# default scores fit its byte table)
LDS_ROUTES = {"lds81": ("8,1", None), "lds81_pk": ("8,1", "v1"), "lds82": ("8,2", None), "lds82_pk": ("8,2", "v1")}


def _route_env(monkeypatch, route):
    """Sets the route's environment; returns (banded, 32-bit scores, kernel_variant)."""
    for k in ("GWAMD_POA_ADD", "GWAMD_CONSENSUS", "GWAMD_CONSENSUS_LDS_BYTES", "GWAMD_POA_SLOTS", "GWAMD_POA_ORDER"):
        monkeypatch.delenv(k, raising=False)
    if route in LDS_ROUTES:
        shape, fwd = LDS_ROUTES[route]
        _full_env(monkeypatch, "lds")
        monkeypatch.setenv("GWAMD_POA_LDS_SHAPE", shape)
        if fwd is not None:
            monkeypatch.setenv("GWAMD_POA_FWD", fwd)
        return False, False, 2
    if route == "wide":
        _full_env(monkeypatch, "lds")
        return False, True, 2
    if route == "v1":
        _full_env(monkeypatch, "v1")
        return False, False, 1
    fwd = route.split("_")[1]
    monkeypatch.delenv("GWAMD_POA_LDS_SHAPE", raising=False)
    monkeypatch.delenv("GWAMD_POA_FWD", raising=False)
    _band_env(monkeypatch, fwd)
    return True, route.endswith("_wide"), BAND_VARIANT[fwd]


FULL = sorted(LDS_ROUTES) + ["wide", "v1"]
BANDED = ["band_row", "band_ad", "band_v1", "band_row_wide", "band_ad_wide"]


@pytest.mark.parametrize("out", ["consensus", "msa"])
@pytest.mark.parametrize("name", W.GROUPS)
@pytest.mark.parametrize("route", FULL + BANDED)
def test_error_windows_on_every_route(route, name, out, monkeypatch):
    banded, wide, variant = _route_env(monkeypatch, route)
    scores = wide_scores(name) if wide else W.DEFAULT
    b = check(name, banded=banded, out=out, scores=scores, variant=variant)
    assert b.get_types()[0] == (32 if wide else 16)
    if route in LDS_ROUTES:
        assert S.fwd2_ok(*scores)  # the row-program pass unless GWAMD_POA_FWD=v1 asks for the packed one


@pytest.mark.parametrize("out", ["consensus", "msa"])
@pytest.mark.parametrize("route", ["band_row", "band_ad", "band_v1", "band_row_wide"])
def test_traceback_loop_bound(route, out, monkeypatch):
    # a read whose end lies outside the last row's band, gap 0: the traceback
    # runs into its loop bound (status 7); 188 bases end inside the band
    banded, wide, variant = _route_env(monkeypatch, route)
    scores = W.GAP0_WIDE if wide else W.GAP0
    b = check("tb7", banded=True, out=out, scores=scores, variant=variant)
    assert b.get_types()[0] == (32 if wide else 16)


@pytest.mark.parametrize("name", W.GROUPS)
@pytest.mark.parametrize("banded", [False, True])
def test_spoa_accurate(banded, name, monkeypatch):
    # the racon order after every read: the error exits sit in front of it
    _route_env(monkeypatch, "band_row" if banded else "lds81")
    monkeypatch.delenv("GWAMD_POA_LDS_SHAPE", raising=False)
    for out in ("consensus", "msa"):
        check(name, banded=banded, out=out, spoa=True, variant=3 if banded else 2)


# ---- the three forms of the graph update ------------------------------------------------------

def _add_plan(max_seq, max_nodes, score_bits):
    L = load_library()
    L.gwamd_internal_poa_lds_add_plan.restype = C.c_int32
    L.gwamd_internal_poa_lds_add_plan.argtypes = [C.c_int32] * 3 + [C.POINTER(C.c_int32)] * 3
    ring, waves, lds = C.c_int32(), C.c_int32(), C.c_int32()
    return L.gwamd_internal_poa_lds_add_plan(max_seq, max_nodes, score_bits, C.byref(ring), C.byref(waves),
                                             C.byref(lds)), waves.value


@pytest.mark.parametrize("out", ["consensus", "msa"])
@pytest.mark.parametrize("name", ["fan", "nodes"])
@pytest.mark.parametrize("mode", [None, "wave0", "serial"])
@pytest.mark.parametrize("route", ["lds81", "lds82", "band_row", "band_ad"])
def test_graph_update_forms(route, mode, name, out, monkeypatch):
    """Status 5 and the first-error order from each form of the update: the
    every-wave form (the default), wave 0 with one read position per lane, and
    the sequential restatement.  The banded kernel has one form (the batched
    update) whatever GWAMD_POA_ADD says; it runs here under all three values."""
    banded, _, variant = _route_env(monkeypatch, route)
    if mode is not None:
        monkeypatch.setenv("GWAMD_POA_ADD", mode)
    g = W.group(name)
    if not banded:
        fits, waves = _add_plan(g.max_seq, g.max_nodes, 16)
        assert fits == 1 and waves == int(LDS_ROUTES[route][0].split(",")[1])
    b = check(name, banded=banded, out=out, variant=variant)
    if banded:
        return
    # the row-order counters tell which form wrote the graph: a read the
    # sequential update took counts as sort_seq_add; every read of a window
    # that succeeds is counted once
    stats = b.get_order_stats()
    want = W.oracle_results(name, False, out == "msa", 16, W.DEFAULT)
    seq_add = CudaPoaBatch.ORDER_STATS.index("sort_seq_add")
    sink_cap = CudaPoaBatch.ORDER_STATS.index("sort_sink_cap")
    per_read = [i for i, n in enumerate(CudaPoaBatch.ORDER_STATS)
                if n == "spliced" or (n.startswith("sort_") and n != "sort_sink_cap")]
    took = 0
    for i, (c, r) in enumerate(zip(g.cases, want)):
        if r.status == 0:
            reads_ok = len(c.reads) - 1
        elif c.name.startswith(("fan49", "dna49", "two_")):
            reads_ok = len(c.reads) - 2  # the error is in the last read, which is not counted
        else:
            continue
        if c.name.startswith(("ordinary", "empty")) or stats[i, sink_cap]:
            continue
        assert int(stats[i, per_read].sum()) == reads_ok, c.name
        # the fan, filler and insertion reads hold no two positions that claim one node: no conflict, no fallback
        assert int(stats[i, seq_add]) == (0 if mode is None else reads_ok), (c.name, mode)
        took += reads_ok
    assert took >= 48 * 5


# ---- consensus builders ------------------------------------------------------------------------

@pytest.mark.parametrize("builder", ["lds", "hbm"])
@pytest.mark.parametrize("route", ["lds81", "lds82", "band_row", "band_ad"])
def test_consensus_builders(route, builder, monkeypatch):
    # C = L (status 2), C = L + 1 (status 0) and the empty window (status 7) from the wave-wide
    # consensus in LDS and from lane 0 in HBM
    banded, _, variant = _route_env(monkeypatch, route)
    if builder == "hbm":
        monkeypatch.setenv("GWAMD_CONSENSUS", "hbm")
    g = W.group("cons")
    names = [c.name for c in g.cases]
    assert {"cons_L161", "cons_L160", "empty1"} <= set(names)
    check("cons", banded=banded, variant=variant)
    check("fan", banded=banded, variant=variant)  # (two more empty windows)


# ---- slot reuse ----------------------------------------------------------------------------------

@pytest.mark.parametrize("out", ["consensus", "msa"])
@pytest.mark.parametrize("name", W.GROUPS)
@pytest.mark.parametrize("route", ["lds81", "lds82", "wide", "band_row", "band_ad"])
def test_slot_reuse_after_errors(route, name, out, monkeypatch):
    """Two workgroups take the whole batch, so each dequeues good windows into
    the slot an error window just left; a second generate_poa gives the same;
    after reset() a batch of the good windows alone shows nothing of the errors."""
    banded, wide, variant = _route_env(monkeypatch, route)
    monkeypatch.setenv("GWAMD_POA_SLOTS", "2")
    scores = wide_scores(name) if wide else W.DEFAULT
    msa = out == "msa"
    b = check(name, banded=banded, out=out, scores=scores, variant=variant, generates=2)
    assert b.get_grid()[0] == 2
    g = W.group(name)
    want = W.oracle_results(name, banded, msa, b.get_types()[0], scores)
    good = [i for i, r in enumerate(want) if r.status == 0]
    assert 2 < len(good) < len(want)
    b.reset()
    assert b.total_poas == 0
    add_all(b, [g.cases[i] for i in good])
    b.generate_poa()
    compare(b, [g.cases[i] for i in good], [want[i] for i in good], msa)
    # the raw output arrays: no status, length or byte of the earlier run's windows
    if not msa:
        status, lens, cbase, vbase, stride = b.get_consensus_raw()
        assert not status.any() and lens.tolist() == [len(want[i].consensus) for i in good]
        for k, i in enumerate(good):
            row = np.ctypeslib.as_array((C.c_uint8 * stride).from_address(cbase + k * stride))
            assert bytes(row[:lens[k]]) == want[i].consensus.encode()


@pytest.mark.parametrize("route", ["lds81", "v1", "band_row"])
def test_msa_rows_of_empty_reads_after_reuse(route, monkeypatch):
    """An empty read writes no begin node.  The first run leaves begin nodes
    120.. in the windows' slots (reads that start on a new node); after reset()
    the same slots hold windows with empty reads, whose MSA rows must start at
    node 0 as in a fresh batch, and an empty window's rows must be empty."""
    banded, _, variant = _route_env(monkeypatch, route)
    g = W.group("fan")
    first = [W.byte_fan(0, 3)] * 4
    second = [[W.BACKBONE, b"", b"", W.READ_1], [b"", b""], [b"", W.BACKBONE, b""], [W.BACKBONE, W.READ_2, b""]]
    b = make_batch(g, "msa", W.DEFAULT, banded)
    for wins in (first, second):
        b.reset()
        for w in wins:
            assert b.add_poa_group(list(w))[0] == 0
        b.generate_poa()
        rows, st = b.get_msa()
        want = [W.run_oracle(w, banded=banded, msa=True, max_nodes=g.max_nodes, max_cons=g.max_cons) for w in wins]
        assert [r.status for r in want] == [0] * 4
        for i, r in enumerate(want):
            assert (st[i], rows[i]) == (0, r.msa), i
    assert b.kernel_variant() == variant
    assert want[0].msa[1] == want[0].msa[2] == W.BACKBONE[:1].decode() + "-" * 119 and want[1].msa == ["", ""]


# ---- through the multi-batch driver ----------------------------------------------------------------

@pytest.mark.parametrize("banded", [False, True])
def test_multibatch_stream_with_error_windows(banded, monkeypatch):
    _route_env(monkeypatch, "band_row" if banded else "lds81")
    monkeypatch.delenv("GWAMD_POA_LDS_SHAPE", raising=False)
    fan = W.group("fan")
    r256 = (W.dna_backbone() + W.BACKBONE)[:256]
    wins = [c.reads for c in fan.cases if not c.name.startswith("empty")]
    wins.insert(3, [r256] * 3)          # C = L = 256: status 2
    wins.insert(9, [r256[:255]] * 3)    # C = L + 1: status 0
    mb = CudaPoaMultiBatch(W.MAX_SEQS, 256, num_batches=2, mem_per_batch=mem_for(256, W.MAX_SEQS, 6),
                           cuda_banded_alignment=banded, alignment_band_width=W.BAND, max_consensus_size=256)
    flat = [r for w in wins for r in w]
    status, clen, cons_a, cov_a = mb.process_packed(np.frombuffer(b"".join(flat), np.uint8),
                                                    np.array([len(r) for r in flat], np.int32),
                                                    [len(w) for w in wins])
    assert mb.skipped() == 0 and mb.info()[2] >= 3
    want = [oracle.poa_window(w, banded=banded, band_width=W.BAND, max_nodes=1024 if banded else 768,
                              max_consensus=256, max_seqs=W.MAX_SEQS) for w in wins]
    assert {r.status for r in want} == {0, 2, 5}
    assert want[3].status == 2 and want[9].status == 0 and len(want[9].consensus) == 255
    for i, r in enumerate(want):
        assert (int(status[i]), int(clen[i])) == (r.status, len(r.consensus)), i
        assert cons_a[i, :clen[i]].tobytes().decode() == r.consensus and cov_a[i, :clen[i]].tolist() == r.coverage, i
