"""Scoring parameters, host side (no GPU): the score / size widths the plan
returns against the reference's rule restated in Python (poa_score_sets.py,
from cudapoa_limits.hpp:28-53 and batch.cu:45-73), the capacity estimate's
(mismatch, gap, match) argument order, and that the oracle's output really
depends on every score set the GPU tests run (so those cannot pass vacuously).
"""
import pytest

import poa_score_sets as S
import test_poa_plan as P
from claragenomicsanalysis_amd import cudapoa


def _widths(L, max_seq, scores, banded):
    got = P.plan(L, {}, P._args(max_seq, banded=banded, scores=scores))
    assert "error" not in got, got
    return got["score_bits"], got["size_bits"]


def _bounds(max_seq, gap, mismatch, match):
    g = S.up4(3 * max_seq)
    return max_seq * match, -(max_seq * max(gap, mismatch) + (g - max_seq) * gap)


def width_grid():
    """(max_sequence_size, (gap, mismatch, match)): the tests' score sets at the
    tests' sizes, and every point of a score grid that lies on a boundary of
    the rule: upper in {32767, 32768}, -lower in {32768, 32769}."""
    pts = [(ms, sc) for ms in (128, 300, 400, 600, 1100, 1489, 1490, 4400, 10600)
           for sc in sorted(set(S.ALL.values()) | {S.DEFAULT})]
    edge = {"upper": set(), "lower": set()}
    for ms in (128, 151, 217, 256, 512, 1024, 1057, 2048, 4096, 10923):
        for match in range(0, 260):
            up, _ = _bounds(ms, -1, -1, match)
            if up in (32767, 32768):
                pts.append((ms, (-1, -1, match)))
                edge["upper"].add(up)
    for target in (32768, 32769):
        found = 0
        for ms in range(128, 1400):
            for gap in range(-130, 0):
                # -lower = ms * -max(gap, mismatch) + (graph rows - ms) * -gap, with mismatch >= gap
                rest = target + (S.up4(3 * ms) - ms) * gap
                if found < 24 and rest >= 0 and rest % ms == 0 and rest // ms <= -gap:
                    sc = (gap, -(rest // ms), 1)
                    assert _bounds(ms, *sc)[1] == target
                    pts.append((ms, sc))
                    edge["lower"].add(target)
                    found += 1
    assert edge == {"upper": {32767, 32768}, "lower": {32768, 32769}}
    return pts


@pytest.mark.parametrize("banded", [0, 1])
def test_score_and_size_width_follow_the_reference_rule(banded, monkeypatch):
    for k in P.ENV_NAMES:
        monkeypatch.setenv(k, "")
    L = P._lib()
    seen = set()
    bad = []
    for ms, sc in width_grid():
        sb = S.ref_score_bits(ms, *sc)
        zb = S.ref_size_bits(sb, ms, bool(banded))
        seen.add((sb, zb))
        got = _widths(L, ms, sc, banded)
        if got != (sb, zb):
            bad.append((ms, sc, got, (sb, zb)))
    assert not bad, bad[:8]
    # both widths occur, and so do 32-bit sizes (10,600 bases, banded: 42,400 rows)
    assert seen == ({(16, 16), (32, 16), (32, 32)} if banded else {(16, 16), (32, 16)})
    # a 16-bit score implies a 16-bit size, whatever the dimensions
    for ms in (8192, 10000, 10900):
        assert S.ref_score_bits(ms, -1, -1, 1) == 16 and 4 * ms > 32767
        assert _widths(L, ms, (-1, -1, 1), banded) == (16, 16)
        assert _widths(L, ms, S.DEFAULT, banded) == (32, 32 if banded or 3 * ms > 32767 else 16)


def test_boundary_values_of_the_rule():
    # the rule's two comparisons, at the last value that keeps int16 and the first that does not
    assert _bounds(256, -1, -1, 128) == (32768, 768)
    assert S.ref_score_bits(256, -1, -1, 128) == 32 and S.ref_score_bits(1057, -1, -1, 31) == 16
    assert _bounds(1024, -11, -10, 1)[1] == 32768 and S.ref_score_bits(1024, -11, -10, 1) == 16
    assert _bounds(331, -49, -1, 1)[1] == 32916 and S.ref_score_bits(331, -49, -1, 1) == 32
    # the tests' sets: what each is there for
    assert S.ref_score_bits(128, -127, -1, 128) == 16 and _bounds(128, -127, -1, 128) == (16384, 32640)
    assert S.ref_score_bits(128, -127, -6, 128) == 32 and _bounds(128, -127, -6, 128) == (16384, 33280)
    assert _bounds(600, -20, -1, 40) == (24000, 24600) and _bounds(600, -15, -20, 45) == (27000, 27000)
    for name in S.EDOMAIN:
        assert S.ref_score_bits(600, *S.EDOMAIN[name]) == 16 and not S.e_domain_fits(600, *S.EDOMAIN[name])
    # the default scores fit the E domain at every size that selects int16
    assert S.ref_score_bits(1489, *S.DEFAULT) == 16 and S.ref_score_bits(1490, *S.DEFAULT) == 32
    assert all(S.e_domain_fits(ms, *S.DEFAULT) for ms in range(1, 1490))


def test_full_plan_keeps_packed_rows_inside_the_e_domain(monkeypatch):
    # the 16-bit LDS kernel (lds_kernel 1 with 16-bit scores) is planned exactly
    # when E[i][j] = H[i][j] - j * gap fits int16 over the batch's columns
    for k in P.ENV_NAMES:
        monkeypatch.setenv(k, "")
    L = P._lib()
    n16 = 0
    for ms, sc in width_grid():
        if ms > 1500 or S.ref_score_bits(ms, *sc) != 16:
            continue
        got = P.plan(L, {}, P._args(ms, scores=sc))
        assert got["lds_kernel"] == (1 if S.e_domain_fits(ms, *sc) else 0), (ms, sc)
        assert got["kernel"] == 1
        n16 += 1
    assert n16 > 50


@pytest.mark.parametrize("kind,names", [
    ("w300", sorted(S.GENERAL)), ("w580", sorted(S.GENERAL)), ("w580e", sorted(S.EDOMAIN)),
    ("w100", sorted(S.EDGE128)), ("tie", list(S.TIE_SETS)),
    ("band", sorted(S.GENERAL) + sorted(S.EDOMAIN) + ["wide_asym", "gap_pos"])])
def test_oracle_output_differs_from_default_scores(kind, names):
    # every window succeeds under every set, and every set changes the output of
    # at least one window (the x k scaled set is exempt: the default's output by design)
    for banded, bw in ((False, 256), (True, 128), (True, 256)):
        if kind == "band" and not banded:
            continue
        if kind in ("w580", "w580e", "w100") and banded:
            continue
        base = [S.observable(r) for r in S.oracle_results(kind, S.DEFAULT, banded, bw)]
        assert all(o[0] == 0 for o in base)
        for name in names:
            if name == "gap_pos" and not banded:
                continue
            sbits = S.ref_score_bits(S.windows(kind)[1], *S.ALL[name])
            out = [S.observable(r) for r in S.oracle_results(kind, S.ALL[name], banded, bw, sbits)]
            assert all(o[0] == 0 for o in out), (name, banded, bw)
            assert sum(a != b for a, b in zip(out, base)) >= 1, (name, banded, bw)


def test_scaled_scores_give_the_default_output():
    for kind in ("w280", "w580"):
        base = [S.observable(r) for r in S.oracle_results(kind, S.DEFAULT)]
        assert [S.observable(r) for r in S.oracle_results(kind, S.WIDE["x10"], score_bits=32)] == base


# ---- (mismatch, gap, match): the capacity overloads' order ---------------------------

FREE = 8 << 30
MS = 1000  # lower = 1000 * max(gap, mismatch) + 2000 * gap: gap -14 / mismatch -6 gives -34,000, swapped -18,000


def _cap(mismatch, gap, match=8, banded=True, msa=False):
    return cudapoa.estimate_max_poas(MS, 8, 256, banded, msa, FREE, 0.9, mismatch=mismatch, gap=gap, match=match)


@pytest.mark.parametrize("banded,msa", [(True, False), (False, False), (True, True)])
def test_capacity_takes_mismatch_before_gap(banded, msa):
    # a swap of gap and mismatch changes the width at this length; scores with
    # gap == mismatch are the same either way, so they give each width's capacity
    assert S.ref_score_bits(MS, -14, -6, 8) == 32 and S.ref_score_bits(MS, -6, -14, 8) == 16
    assert S.ref_score_bits(MS, -14, -14, 8) == 32 and S.ref_score_bits(MS, -6, -6, 8) == 16
    cap32, cap16 = _cap(-14, -14, banded=banded, msa=msa), _cap(-6, -6, banded=banded, msa=msa)
    assert 0 < cap32 < cap16
    assert _cap(mismatch=-6, gap=-14, banded=banded, msa=msa) == cap32
    assert _cap(mismatch=-14, gap=-6, banded=banded, msa=msa) == cap16
    # the score matrix is what differs: band (or read) columns x graph rows x the score's bytes
    cols = 256 + 8 if banded else MS
    rows = S.up4((4 if banded else 3) * MS)
    per16, per32 = int(0.9 * FREE) // cap16, int(0.9 * FREE) // cap32
    assert abs((per32 - per16) - 2 * cols * rows) <= max(per32 // cap32, per16 // cap16) + 2


def test_multi_batch_sizes_take_mismatch_before_gap():
    # groups around the length where the swap flips the width: binning with
    # (mismatch -6, gap -14) equals binning with the 32-bit capacity, the
    # swapped call the 16-bit one, and the two differ
    groups = [["A" * n] + ["C" * 10] * 7 for n in range(968, 1088, 4)]
    bins = [13, 19, 1 << 19]  # between the capacities of the two widths at these lengths
    free = 96 << 20

    def sizes(mismatch, gap):
        res = cudapoa.get_multi_batch_sizes(groups, bins_capacity=bins, free_device_memory=free,
                                            mismatch_score=mismatch, gap_score=gap, match_score=8)
        assert sorted(g for b in res[1] for g in b) == list(range(len(groups)))
        return res

    def binning(mismatch, gap):
        caps = [cudapoa.estimate_max_poas(len(g[0]), len(g), 256, True, False, free, 0.9, mismatch=mismatch,
                                          gap=gap, match=8) for g in groups]
        return [min(j for j in range(3) if c <= bins[j] or j == 2) for c in caps]

    for n in range(968, 1088, 4):  # the rule at each group's length
        assert S.ref_score_bits(n, -14, -6, 8) == 32 and S.ref_score_bits(n, -14, -14, 8) == 32
        assert S.ref_score_bits(n, -6, -14, 8) == 16 and S.ref_score_bits(n, -6, -6, 8) == 16
    assert sizes(mismatch=-6, gap=-14) == sizes(mismatch=-14, gap=-14)
    assert sizes(mismatch=-14, gap=-6) == sizes(mismatch=-6, gap=-6)
    assert binning(mismatch=-6, gap=-14) != binning(mismatch=-14, gap=-6)
    assert sizes(mismatch=-6, gap=-14) != sizes(mismatch=-14, gap=-6)
