"""The LDS full-alignment kernel's graph update on every wave of the workgroup
(add_alignment_waves, poa_wave.hpp): the batched add with kAU = 4 read
positions per lane, so one pass of NW waves covers P = NW * 4 * 64 positions.

Every GPU test compares status, consensus and coverage (or MSA rows) and the
final graph (edges, weights, bases) bit for bit with the oracle, and the three
forms of the update with each other: the default (every wave), GWAMD_POA_ADD=
wave0 (one wave, one position per lane) and GWAMD_POA_ADD=serial (the
sequential restatement on lane 0 for every read).  Small windows would pick a
one-wave shape by themselves; GWAMD_POA_LDS_SHAPE forces the multi-wave ones.
A test that returns at all has passed the barrier check of its paths: every
wave of the workgroup must meet the same barriers on each of them.
"""
import ctypes as C
import random

import numpy as np
import pytest

from claragenomicsanalysis_amd import load_library, synth
from claragenomicsanalysis_amd.cudapoa import CudaPoaBatch
from oracle import oracle

MEM = 8 << 30
MODES = (None, "wave0", "serial")  # None: the default, the every-wave update


def _lib():
    L = load_library()
    L.gwamd_internal_poa_lds_add_bytes.restype = C.c_longlong
    L.gwamd_internal_poa_lds_add_bytes.argtypes = [C.c_int32, C.c_int32]
    L.gwamd_internal_poa_lds_add_fits.restype = C.c_int32
    L.gwamd_internal_poa_lds_add_fits.argtypes = [C.c_int32] * 3
    L.gwamd_internal_poa_lds_add_plan.restype = C.c_int32
    L.gwamd_internal_poa_lds_add_plan.argtypes = [C.c_int32] * 3 + [C.POINTER(C.c_int32)] * 3
    return L


def _plan(max_seq, max_nodes, score_bits):
    """(the fit rule on the planned ring region, its bytes, waves, LDS bytes) of the host plan."""
    ring, waves, lds = C.c_int32(), C.c_int32(), C.c_int32()
    r = _lib().gwamd_internal_poa_lds_add_plan(max_seq, max_nodes, score_bits, C.byref(ring), C.byref(waves),
                                               C.byref(lds))
    return r, ring.value, waves.value, lds.value


def _mutate(rng, seq, length, sub=0.04, alphabet="ACGT"):
    """A read of exactly `length` bases from a random place of seq: substitutions
    and a few insertion / deletion pairs."""
    off = rng.randrange(0, len(seq) - length + 1)
    r = list(seq[off:off + length])
    for i in range(len(r)):
        if rng.random() < sub:
            r[i] = rng.choice(alphabet)
    for _ in range(length // 100):
        r.insert(rng.randrange(len(r)), rng.choice(alphabet))
        del r[rng.randrange(len(r))]
    return "".join(r).encode()


def _snapshot(b, msa):
    graphs, gst = b.get_graphs()
    # (a DiGraph holds the nodes that have an edge, and their bases)
    gs = [({e: g.weight(*e) for e in g.edges}, {v: g.label(v) for v in g.nodes}) for g in graphs]
    if msa:
        rows, st = b.get_msa()
        return [(st[i], rows[i], gs[i]) for i in range(len(st))]
    cons, cov, st = b.get_consensus()
    return [(st[i], cons[i], cov[i], gs[i]) for i in range(len(st))]


def _run(wins, max_seq, max_seqs, out="consensus", wts=None, generates=1, **kw):
    b = CudaPoaBatch(max_seqs, max_seq, MEM, output_type=out, alignment_band_width=256 if max_seq >= 256 else 128, **kw)
    for i, w in enumerate(wins):
        st, _ = b.add_poa_group(list(w), weights=None if wts is None else wts[i])
        assert st == 0
    snaps = []
    for _ in range(generates):
        b.generate_poa()
        snaps.append(_snapshot(b, out == "msa"))
    return b, snaps


def _expect(wins, max_seq, max_seqs, msa=False, score_bits=16, wts=None, max_nodes=None, max_consensus=None):
    mn = (3 * max_seq + 3) // 4 * 4 if max_nodes is None else max_nodes
    out = []
    for i, w in enumerate(wins):
        ww = None
        if wts is not None:
            ww = [np.ones(len(r), np.int8) if x is None else x for x, r in zip(wts[i], w)]
        r = oracle.poa_window(w, weights=ww, msa=msa, score_bits=score_bits, max_nodes=mn,
                              max_consensus=2 * max_seq if max_consensus is None else max_consensus,
                              max_seqs=max_seqs, want_graph=True)
        g = ({}, {})
        if r.status == 0:
            edges = {(src, v): wt for v, ins in enumerate(r.graph["in"]) for (src, wt) in ins}
            g = (edges, {v: r.graph["bases"][v] for v in sorted({x for e in edges for x in e})})
        out.append((r.status, r.msa, g) if msa else (r.status, r.consensus, r.coverage, g))
    return out


def _set_mode(monkeypatch, mode, shape=None):
    monkeypatch.delenv("GWAMD_POA_KERNEL", raising=False)
    monkeypatch.setenv("GWAMD_DIAG", "1")
    if shape is None:
        monkeypatch.delenv("GWAMD_POA_LDS_SHAPE", raising=False)
    else:
        monkeypatch.setenv("GWAMD_POA_LDS_SHAPE", shape)
    if mode is None:
        monkeypatch.delenv("GWAMD_POA_ADD", raising=False)
    else:
        monkeypatch.setenv("GWAMD_POA_ADD", mode)


def _all_modes(monkeypatch, shape, wins, max_seq, max_seqs, score_bits=16, out="consensus", wts=None, **kw):
    """The windows under the three forms of the update; every form must equal
    the oracle (and so each other)."""
    expect = _expect(wins, max_seq, max_seqs, msa=out == "msa", score_bits=score_bits, wts=wts,
                     max_nodes=kw.get("max_nodes_per_window"), max_consensus=kw.get("max_consensus_size"))
    got = {}
    for mode in MODES:
        _set_mode(monkeypatch, mode, shape)
        if mode is None:  # the every-wave update is what the plan selects, on the forced shape
            mn = kw.get("max_nodes_per_window", 3 * max_seq)
            fits, _, waves, _ = _plan(max_seq, mn, score_bits)
            assert fits == 1 and waves == int(shape.split(",")[1]), (shape, fits, waves)
        b, snaps = _run(wins, max_seq, max_seqs, out=out, wts=wts, **kw)
        assert b.kernel_variant() == 2 and b.get_types()[0] == score_bits
        got[mode] = snaps[0]
        for i, (g, e) in enumerate(zip(snaps[0], expect)):
            assert g == e, (shape, mode, i)
    assert got[None] == got["wave0"] == got["serial"]
    return expect


# 1 and 3a. Read lengths around the pass size P = NW * 4 * 64: below P the upper
# waves have no positions at all in a pass; P - 1, P, P + 1 end a pass one short
# of, at and one past its last lane; one read longer than 2 P where the batch's
# maximum read length allows.  16-bit kernel at two and four waves, the 32-bit
# one (max_sequence_size >= 1,490 selects it) at two and eight.
@pytest.mark.gpu
@pytest.mark.parametrize("shape,score_bits,max_seq", [("8,2", 16, 1100), ("8,4", 16, 1100), ("4,4", 16, 1100),
                                                      ("8,2", 32, 1600), ("8,8", 32, 2200)])
def test_pass_boundaries(shape, score_bits, max_seq, monkeypatch):
    nw = int(shape.split(",")[1])
    P = nw * 4 * 64
    rng = random.Random(1000 * nw + score_bits)
    long_len = 2 * P + 6 if 2 * P + 6 <= max_seq else None
    groups = [[1, 63, 64, 65, P - 1], [255, 256, 257, P, P + 1], [long_len or P, 65, 1, P + 1]]
    wins = []
    for lens in groups:
        bb = "".join(rng.choice("ACGT") for _ in range(max(lens) + 8))
        wins.append([bb.encode()] + [_mutate(rng, bb, n) for n in lens])
    assert max(len(r) for w in wins for r in w) <= max_seq
    _all_modes(monkeypatch, shape, wins, max_seq, 6, score_bits=score_bits)


# 2. Error and early-exit paths on two and four waves, on a persistent grid of
# three workgroups with two generates, so slots and LDS images are reused after
# an error window: the node limit (max_nodes_per_window just above the
# backbone), a second read that is empty or one base long, a single read.
@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["8,2", "8,4"])
def test_error_and_early_exit_paths(shape, monkeypatch):
    _set_mode(monkeypatch, None, shape)
    monkeypatch.setenv("GWAMD_POA_SLOTS", "3")
    wins = synth.poa_windows(61, 3, 100, 8, 20, 20, 20)
    rng = random.Random(7)
    bb = "".join(rng.choice("ACGT") for _ in range(100))
    ok = [bb.encode()] + [_mutate(rng, bb, 90 + k) for k in range(4)]
    wins = [wins[0], [ok[0], b"", ok[1], ok[2]], wins[1], [ok[0], b"G", ok[3], b"", ok[1]], [ok[0]], wins[2], ok,
            [ok[2], ok[0]]]
    fits, _, waves, _ = _plan(130, 140, 16)
    assert fits == 1 and waves == int(shape.split(",")[1])
    b, snaps = _run(wins, 130, 8, generates=2, max_nodes_per_window=140)
    assert b.kernel_variant() == 2 and b.get_grid()[0] == 3
    expect = _expect(wins, 130, 8, max_nodes=140, max_consensus=260)
    assert any(e[0] == 4 for e in expect) and any(e[0] == 0 for e in expect)
    for rep, snap in enumerate(snaps):
        for i, (g, e) in enumerate(zip(snap, expect)):
            assert g == e, (shape, rep, i)


# 3b. Dense aligned-node groups: short, high-error reads over a two-letter
# alphabet make positions of one read claim the same node or group, which is
# the conflict return and the sequential restatement behind it.
@pytest.mark.gpu
def test_fallback_path_low_complexity(monkeypatch):
    rng = random.Random(11)
    wins = []
    for k in range(16):
        n = 60 + 4 * k
        bb = "".join(rng.choice("AC") for _ in range(n + 10))
        wins.append([bb[:n].encode()] + [_mutate(rng, bb, rng.randrange(60, n + 1), sub=0.28, alphabet="AC")
                                         for _ in range(9)])
    _all_modes(monkeypatch, "8,2", wins, 130, 10)


# 4. Caller-supplied weights (the edge weights the update adds) and the MSA
# (the update writes the edges' read lists) at config B's shape of two waves.
@pytest.mark.gpu
@pytest.mark.parametrize("out", ["consensus", "msa"])
def test_weights_and_msa(out, monkeypatch):
    wins = synth.poa_windows(2101, 3, 560, 8, 30, 30, 30)
    wins.append([b"ACGTACGTTA", b"", b"A", b"ACGTTCGTTA", b"ACGAACGTTA"])
    wrng = np.random.default_rng(3)
    wts = [[None if j % 4 == 3 else wrng.integers(0, 61, size=len(r), dtype=np.int8) for j, r in enumerate(w)]
           for w in wins]
    _all_modes(monkeypatch, "8,2", wins, 700, 8, out=out, wts=wts)


# 6. The fit rule (lds_add_fits, one constexpr function for the host's plan and
# the kernel) against the layout the host plans, without a device.
def test_fit_function_matches_plan(monkeypatch):
    monkeypatch.setenv("GWAMD_DIAG", "1")
    monkeypatch.delenv("GWAMD_POA_KERNEL", raising=False)
    monkeypatch.delenv("GWAMD_POA_LDS_SHAPE", raising=False)
    monkeypatch.delenv("GWAMD_POA_LDS_PAD", raising=False)
    L = _lib()

    def need(msl, mn):  # the layout written out: gid, curr, kind, owner | hit, ohit, control words
        ms = (msl + 16) & ~15
        return ((5 * ms + 2 * (mn + msl) + 15) & ~15) + 2 * ms + 64

    # config B: BatchSize(1100, 32), 3,300 nodes; two waves, four workgroups per
    # CU (40 KB each), 8 ring rows of 1,152 int16 = 18,432 bytes
    fits, ring, waves, lds = _plan(1100, 3300, 16)
    assert (fits, ring, waves) == (1, 18432, 2) and lds + 16 <= 40960
    assert L.gwamd_internal_poa_lds_add_bytes(1100, 3300) == need(1100, 3300) == 16592
    # the rule itself, at its edge
    for msl, mn in [(1100, 3300), (130, 140), (2200, 6600), (700, 2100)]:
        n = need(msl, mn)
        assert L.gwamd_internal_poa_lds_add_bytes(msl, mn) == n
        assert L.gwamd_internal_poa_lds_add_fits(msl, mn, n) == 1
        assert L.gwamd_internal_poa_lds_add_fits(msl, mn, n - 1) == 0
    assert L.gwamd_internal_poa_lds_add_fits(0, 100, 1 << 20) == 0
    assert L.gwamd_internal_poa_lds_add_fits(30000, 40000, 1 << 20) == 0  # 16-bit node and position fields
    # the plan's flag is the rule applied to the plan's own ring region, where
    # it accepts and where it must decline (a node capacity whose owner array
    # outgrows a ring region sized by the rows, the tile and the one-wave update)
    seen = set()
    for msl, mn, bits in [(1100, 3300, 16), (1100, 4400, 16), (1100, 5200, 16), (600, 1800, 16), (130, 140, 16),
                          (1600, 4800, 32), (2200, 6600, 32), (1100, 8000, 16)]:
        fits, ring, waves, lds = _plan(msl, mn, bits)
        if fits < 0:
            continue
        assert fits == L.gwamd_internal_poa_lds_add_fits(msl, mn, ring), (msl, mn, bits)
        assert fits == (1 if need(msl, mn) <= ring else 0), (msl, mn, bits)
        seen.add(fits)
    assert seen == {0, 1}
    assert _plan(1100, 5200, 16)[0] == 0
