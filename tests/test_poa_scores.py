"""GPU parity over the scoring parameters: every POA kernel against the oracle
(oracle.poa_window) with the same gap / mismatch / match scores, bit-exact:
status, consensus, coverage, the final graph (edges and weights: the
alignments decide them) and MSA rows.  The score sets (tests/poa_score_sets.py)
are chosen by the code they reach: the 16-bit LDS kernel's row-program pass
(fwd2) and its packed pass (nw_forward_lds_pk, taken when a substitution score
leaves the byte table), the byte table's edges, the int16 / int32 choice, the
E-domain bound, the banded kernel's minv / Tmax / truncation and real-value
bounds, and the traceback tie order.  Each test restates which route its
scores take and asserts what a batch shows of it (get_types, kernel_variant).

That every set's expected output differs from the default scores' is asserted
on the oracle alone in test_poa_scores_cpu.py.
"""
import pytest

import poa_score_sets as S
from claragenomicsanalysis_amd.cudapoa import CudaPoaBatch

pytestmark = pytest.mark.gpu

MEM = 1 << 30


def run_gpu(kind, scores, banded=False, bw=256, output_type="consensus", spoa=None):
    wins, max_seq = S.windows(kind)
    gap, mismatch, match = scores
    b = CudaPoaBatch(8, max_seq, MEM, output_type=output_type, gap_score=gap, mismatch_score=mismatch,
                     match_score=match, cuda_banded_alignment=banded, alignment_band_width=bw, spoa_accurate=spoa)
    for w in wins:
        st, seq_st = b.add_poa_group(list(w))
        assert st == 0 and all(s == 0 for s in seq_st)
    b.generate_poa()
    return b


def check(kind, scores, banded=False, bw=256, msa=False, spoa=False, variant=None):
    """One consensus batch (and one MSA batch) against the oracle; returns the batch."""
    max_seq = S.windows(kind)[1]
    b = run_gpu(kind, scores, banded, bw, spoa=spoa)
    sbits, zbits = b.get_types()
    assert (sbits, zbits) == (S.ref_score_bits(max_seq, *scores), 16)
    want = S.oracle_results(kind, scores, banded, bw, sbits, False, spoa)
    assert all(r.status == 0 for r in want)
    cons, cov, st = b.get_consensus()
    graphs, gst = b.get_graphs()
    for i, r in enumerate(want):
        assert (st[i], cons[i], cov[i]) == (r.status, r.consensus, r.coverage), i
        g = graphs[i]
        expect = {(src, v): wt for v, ins in enumerate(r.graph["in"]) for (src, wt) in ins}
        assert gst[i] == 0 and {(u, v): g.weight(u, v) for (u, v) in g.edges} == expect, i
        assert "".join(g.label(v) for v in range(r.final_nodes)) == r.graph["bases"], i
    if variant is not None:
        assert b.kernel_variant() == variant
    if msa:
        m = run_gpu(kind, scores, banded, bw, output_type="msa", spoa=spoa)
        rows, mst = m.get_msa()
        wantm = S.oracle_results(kind, scores, banded, bw, sbits, True, spoa)
        for i, r in enumerate(wantm):
            assert (mst[i], rows[i]) == (r.status, r.msa), i
    return b


def _full_env(monkeypatch, kernel):
    monkeypatch.delenv("GWAMD_POA_FWD", raising=False)
    monkeypatch.delenv("GWAMD_POA_LDS_SHAPE", raising=False)
    if kernel == "v1":
        monkeypatch.setenv("GWAMD_POA_KERNEL", "v1")
    else:
        monkeypatch.delenv("GWAMD_POA_KERNEL", raising=False)


def _band_env(monkeypatch, fwd):
    if fwd == "v1":
        monkeypatch.setenv("GWAMD_POA_KERNEL", "v1")
        monkeypatch.delenv("GWAMD_BAND_FWD", raising=False)
    else:
        monkeypatch.delenv("GWAMD_POA_KERNEL", raising=False)
        monkeypatch.setenv("GWAMD_BAND_FWD", fwd)


BAND_VARIANT = {"row": 3, "ad": 4, "v1": 1}
# general sets whose substitution scores both fit the byte table (0 <= score - gap <= 255):
# the row-program pass; the others have mismatch < gap and take the packed pass
FWD2_SETS = {"mm_eq_gap", "match0", "mismatch0", "unit", "zero"}


# ---- full alignment --------------------------------------------------------------

@pytest.mark.parametrize("kernel", ["lds", "v1"])
@pytest.mark.parametrize("kind", ["w300", "w580"])
@pytest.mark.parametrize("name", sorted(S.GENERAL))
def test_full_general_sets(name, kind, kernel, monkeypatch):
    # 16-bit scores by the reference's rule at both sizes; on the LDS kernel one
    # wave (max_sequence_size 400) and two (600), row-program pass when both
    # substitution scores fit the byte table, else the packed pass; MSA rows on
    # the one-wave LDS route
    _full_env(monkeypatch, kernel)
    scores = S.GENERAL[name]
    max_seq = S.windows(kind)[1]
    assert S.ref_score_bits(max_seq, *scores) == 16 and S.e_domain_fits(max_seq, *scores)
    assert S.fwd2_ok(*scores) == (name in FWD2_SETS)
    check(kind, scores, msa=(kernel == "lds" and kind == "w300"), variant=1 if kernel == "v1" else 2)


@pytest.mark.parametrize("kernel", ["lds", "v1"])
@pytest.mark.parametrize("name", sorted(S.EDGE128))
def test_full_byte_table_edge(name, kernel, monkeypatch):
    # match - gap = 255 is the last value of fwd2's byte table, 256 the first
    # past it (then 128 * 256 also passes the E-domain bound).  With mismatch
    # -6 the reference's rule selects int32 at this size, so those run the
    # 32-bit rows
    _full_env(monkeypatch, kernel)
    scores = S.EDGE128[name]
    gap, mismatch, match = scores
    assert match - gap == (255 if "255" in name else 256) and S.fwd2_ok(*scores) == ("255" in name)
    wide = name.endswith("_w")
    assert S.ref_score_bits(128, *scores) == (32 if wide else 16)
    assert max(len(r) for w in S.windows("w100")[0] for r in w) <= 120
    b = check("w100", scores, bw=128, msa=(kernel == "lds"),
              variant=1 if kernel == "v1" else S.full_kernel_variant(128, scores))
    assert b.get_types()[0] == (32 if wide else 16)


@pytest.mark.parametrize("kernel", ["lds", "v1"])
@pytest.mark.parametrize("name", sorted(S.EDOMAIN))
def test_full_e_domain_bound(name, kernel, monkeypatch):
    """int16 by the reference's rule, but the LDS kernel's E domain, E[i][j] =
    H[i][j] - j * gap, passes 32,767 on a read that matches its graph.  Such a
    batch must not run the packed 16-bit rows: it runs the global-memory kernel
    and reports the reference's types."""
    _full_env(monkeypatch, kernel)
    scores = S.EDOMAIN[name]
    gap, mismatch, match = scores
    wins, max_seq = S.windows("w580e")
    assert S.ref_score_bits(max_seq, *scores) == 16
    assert S.fwd2_ok(*scores) == (name == "edom_fwd2")
    assert max(len(r) for w in wins for r in w) * (match - gap) > 32767
    assert not S.e_domain_fits(max_seq, *scores)
    b = check("w580e", scores, msa=(kernel == "lds"), variant=1)
    assert b.get_types()[0] == 16


@pytest.mark.parametrize("kernel", ["lds", "v1"])
@pytest.mark.parametrize("kind", ["w280", "w580"])
def test_full_wide_rows_other_scores(kind, kernel, monkeypatch):
    # 32-bit rows (nw_forward_lds_w) at one wave (max_sequence_size 300) and two (600)
    _full_env(monkeypatch, kernel)
    scores = S.WIDE["x10"]
    assert S.ref_score_bits(S.windows(kind)[1], *scores) == 32
    check(kind, scores, msa=(kernel == "lds"), variant=1 if kernel == "v1" else 2)


# ---- banded ------------------------------------------------------------------------

@pytest.mark.parametrize("fwd", ["row", "ad", "v1"])
@pytest.mark.parametrize("bw", [128, 256])
@pytest.mark.parametrize("name", sorted(S.GENERAL) + sorted(S.EDOMAIN))
def test_banded_sets(name, bw, fwd, monkeypatch):
    # band_min_value / Tmax / trunc_score (row-parallel pass) and the real-value
    # bound lo / hi / store_all (anti-diagonal pass) take the scores; the windows
    # hold a read much shorter and one much longer than the graph
    _band_env(monkeypatch, fwd)
    scores = S.ALL[name]
    assert S.ref_score_bits(400, *scores) == 16
    check("band", scores, banded=True, bw=bw, msa=(fwd == "row" and bw == 256), variant=BAND_VARIANT[fwd])


@pytest.mark.parametrize("fwd", ["row", "ad", "v1"])
@pytest.mark.parametrize("bw", [128, 256])
@pytest.mark.parametrize("name", sorted(S.WIDE_BANDED))
def test_banded_wide_scores(name, bw, fwd, monkeypatch):
    _band_env(monkeypatch, fwd)
    scores = S.WIDE_BANDED[name]
    assert S.ref_score_bits(400, *scores) == 32
    check("band", scores, banded=True, bw=bw, msa=(fwd == "ad" and bw == 128), variant=BAND_VARIANT[fwd])


@pytest.mark.parametrize("bw", [128, 256])
def test_banded_positive_gap(bw, monkeypatch):
    # gap > 0: no banded LDS kernel (plan_band_kernel), the global-memory kernel, still equal to the oracle
    monkeypatch.delenv("GWAMD_POA_KERNEL", raising=False)
    monkeypatch.delenv("GWAMD_BAND_FWD", raising=False)
    check("band", S.POSITIVE_GAP["gap_pos"], banded=True, bw=bw, msa=(bw == 256), variant=1)


# ---- ties, SPOA_ACCURATE ---------------------------------------------------------------

@pytest.mark.parametrize("route", ["lds", "v1", "band_row", "band_ad", "band_v1"])
@pytest.mark.parametrize("name", S.TIE_SETS)
def test_tie_window(name, route, monkeypatch):
    # repeats, an empty and a one-base read under scores that tie everywhere:
    # the traceback's tie order (cudapoa_nw.cuh:361-443) decides the graph
    banded = route.startswith("band")
    if banded:
        _band_env(monkeypatch, route[5:])
    else:
        _full_env(monkeypatch, route)
    check("tie", S.GENERAL[name], banded=banded, msa=route in ("lds", "band_row"),
          variant=BAND_VARIANT[route[5:]] if banded else (1 if route == "v1" else 2))


@pytest.mark.parametrize("banded", [False, True])
@pytest.mark.parametrize("name", ["asym_a", "mm_eq_2gap"])
def test_spoa_accurate_with_scores(name, banded, monkeypatch):
    monkeypatch.delenv("GWAMD_POA_KERNEL", raising=False)
    monkeypatch.setenv("GWAMD_BAND_FWD", "row")
    check("band" if banded else "w300", S.GENERAL[name], banded=banded, msa=True, spoa=True,
          variant=3 if banded else 2)
