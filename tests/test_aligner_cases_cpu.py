"""The aligner case families, host side (no GPU): every oracle path of every
family is an optimal alignment by a checker that does not use the oracle, and
every family really has the property it is there for (paths that depend on
the tie rules, band classes, band rows, results that change with
max_query_length, a letter rule that changes the distance), so that the GPU
tests of test_aligner_ties.py cannot pass vacuously.
"""
import pytest

import aligner_cases as A
from oracle import oracle

BATCHES = A.batches()


def _check_batch(pairs):
    mq_all = max([1] + [len(q) for q, _ in pairs])
    for name, oalgo, rule in A.ALGORITHMS:
        for q, t in pairs:
            st = A.oracle_states(q, t, oalgo, mq_all)
            A.check_alignment(q, t, st, rule, band_limited=name == "ukkonen")


@pytest.mark.parametrize("batch", sorted(BATCHES))
def test_oracle_paths_are_optimal(batch):
    _check_batch(BATCHES[batch])


def test_oracle_paths_are_optimal_long_pairs():
    # the pairs that have GPU tests of their own
    for d in A.UKKONEN_WIDE_DIFFS:
        _check_batch(A.ukkonen_wide(d))
    for q, t in A.seams_8k():
        A.check_alignment(q, t, A.oracle_states(q, t, oracle.ALIGN_MYERS, len(q)), "myers")


def test_multi_chunk_diagonal_bands_are_not_exact():
    # bands of 58 and 258 words that are not the whole query: the reference's
    # chunk hand-over in the diagonal phase (check_alignment, exact) costs 12
    # and 1 edits more than the distance here; the other aligners are exact on
    # the same pairs
    over = []
    for q, t in A.banded()["multi_chunk"]:
        st, bw, _ = oracle.myers_banded(q, t)
        assert 32 * 32 < bw < len(q)
        assert st == A.oracle_states(q, t, oracle.ALIGN_MYERS_BANDED, len(q))
        over.append(A.check_alignment(q, t, st, "myers", exact=False) - A.edit_distance(q, t, "myers"))
        A.check_alignment(q, t, A.oracle_states(q, t, oracle.ALIGN_MYERS, len(q)), "myers")
    assert over == [12, 1]
    q, t = A.banded()["multi_chunk"][0]
    A.check_alignment(q, t, A.oracle_states(q, t, oracle.ALIGN_HM, len(q)), "myers")
    A.check_alignment(q, t, A.oracle_states(q, t, oracle.ALIGN_UKKONEN, len(q)), "raw", band_limited=True)


def test_checker_rejects_wrong_paths():
    q, t = "ACGGGT", "ACGNNT"
    assert A.edit_distance(q, t, "myers") == 0 and A.edit_distance(q, t, "raw") == 2
    A.check_alignment(q, t, [0] * 6, "myers")
    A.check_alignment(q, t, [0, 0, 0, 1, 1, 0], "raw")
    with pytest.raises(AssertionError):  # one base of the target not consumed
        A.check_alignment(q, t, [0] * 5 + [3], "myers")
    with pytest.raises(AssertionError):  # a complete path that costs 2 more than the distance
        A.check_alignment(q, t, [2] + [0] * 5 + [3], "myers")
    with pytest.raises(AssertionError):  # ACGT only: a mismatch labelled as a match
        A.check_alignment("ACGT", "ACTT", [0, 0, 0, 0], "raw")
    assert A.edit_distance("", "ACG", "raw") == 3 and A.edit_distance("ACG", "", "myers") == 3
    assert A.edit_distance("kitten", "sitting", "raw") == 3
    # against the oracle's own distance (Myers rule) on a pair of the alphabet family
    q, t = A.alphabet()[1]
    assert A.edit_distance(q, t, "myers") == oracle.edit_distance(q, t)


@pytest.mark.parametrize("family", A.TIE_FAMILIES)
def test_tie_families_depend_on_the_tie_rules(family):
    # Hirschberg-Myers and full Myers differ only through their tie rules
    pairs = A.tie_family(family)
    mq = max(len(q) for q, _ in pairs)
    differ = sum(1 for q, t in pairs
                 if A.oracle_states(q, t, oracle.ALIGN_HM, mq) != A.oracle_states(q, t, oracle.ALIGN_MYERS, mq))
    assert differ >= 3, differ


def _first_band(q, t):
    lo, d = min(len(q), len(t)), abs(len(q) - len(t))
    return min(1 + 2 * (lo // 40) + d, len(q))


def test_banded_classes_are_reached():
    C = A.banded()
    got = {k: [oracle.myers_banded(q, t)[1:] for q, t in v] for k, v in C.items()}
    first = {k: [_first_band(q, t) for q, t in v] for k, v in C.items()}
    assert all(bw % 32 == 0 and tries == 1 for bw, tries in got["bw_mod32_0"]), got["bw_mod32_0"]
    assert all(f % 32 == 1 for f in first["bw_mod32_1"])
    assert all(bw == f + 2 and tries == 1 for (bw, tries), f in zip(got["bw_mod32_1"], first["bw_mod32_1"]))
    assert all(bw == len(q) for (bw, _), (q, _) in zip(got["bw_is_query"], C["bw_is_query"]))
    assert got["bw_is_query"][0][1] == 1 and got["bw_is_query"][2][1] > 1  # at once, and by doubling
    assert all(tries == 1 for _, tries in got["tries_1"])
    assert all(tries == 2 for _, tries in got["tries_2"])
    assert all(tries >= 4 for _, tries in got["tries_4"])
    assert all(bw < len(q) for k in ("tries_1", "tries_2") for (bw, _), (q, _) in zip(got[k], C[k]))
    assert got["multi_chunk"][0][0] > 32 * 32      # more than one 32-word chunk
    assert got["multi_chunk"][1][0] > 256 * 32     # more band words than a 4 KiB tile holds
    # the classes are the oracle's: the same path as oracle.align
    for v in C.values():
        for q, t in v[:1]:
            assert oracle.myers_banded(q, t)[0] == A.oracle_states(q, t, oracle.ALIGN_MYERS_BANDED, len(q))


def test_max_query_length_changes_the_result():
    pairs = A.max_query()
    assert sorted((len(q), len(t)) for q, t in pairs) == [(40, 600), (40, 2000), (60, 600), (60, 2000)]
    longest = max(len(q) for q, _ in pairs)
    for q, t in pairs:
        cigars = set()
        for mq in A.MAX_QUERY_VALUES + (longest,):
            st = A.oracle_states(q, t, oracle.ALIGN_HM, mq)
            A.check_alignment(q, t, st, "myers")
            cigars.add(oracle.cigar(st))
        assert len(cigars) >= A.max_query_regimes((q, t)), (len(q), len(t), len(cigars))
        same = [oracle.cigar(A.oracle_states(q, t, oracle.ALIGN_HM, mq)) for mq in (400, 5000)]
        assert same[0] == same[1]
    assert [A.max_query_regimes(p) for p in pairs] == [2, 2, 3, 3]


def test_ukkonen_band_rows_and_ten_percent_rule():
    def rows(diff):  # ukkonen_band_rows
        return (diff + 202) // 2

    want = {54: 128, 56: 129, 182: 192, 184: 193, 310: 256, 312: 257, 438: 320, 440: 321, 822: 512, 824: 513}
    lists = [(A.ukkonen_rows(), A.UKKONEN_ROWS_MAX_TARGET)]
    lists += [(A.ukkonen_wide(d), A.UKKONEN_WIDE_MAX_TARGET) for d in A.UKKONEN_WIDE_DIFFS]
    seen = set()
    for pairs, max_t in lists:
        orient = set()
        for q, t in pairs:
            d = abs(len(q) - len(t))
            assert rows(d) == want[d] == A.ukkonen_band_rows(d)
            assert d <= A.ukkonen_allowed_difference(max_t) and len(t) <= max_t
            seen.add(d)
            orient.add((d, len(q) > len(t)))
        assert len(orient) == 2 * len({d for d, _ in orient})  # query longer and target longer
    assert seen == set(want)
    assert A.ukkonen_allowed_difference(8240) == 824 and A.ukkonen_allowed_difference(8239) == 823
    # every batch Ukkonen runs is inside the rule at the capacity its test uses
    for name, pairs in BATCHES.items():
        _, max_t = A.capacity(pairs, "ukkonen")
        for q, t in pairs:
            assert abs(len(q) - len(t)) <= A.ukkonen_allowed_difference(max_t), name
            assert len(t) <= max_t


def test_alphabet_family_separates_the_letter_rules():
    pairs = A.alphabet()
    used = set()
    for q, t in pairs:
        used |= set(q) | set(t)
        if len(q) >= 600 and len(t) >= 600:
            assert A.edit_distance(q, t, "myers") != A.edit_distance(q, t, "raw"), (len(q), len(t))
    assert used >= set(A.ALPHABET) and any(c >= 0x80 for c in used)
    assert any(set(t) - set(b"ACGT") for _, t in pairs)  # odd bytes on the target side
    q, t = "ACGGGT", "ACGNNT"
    assert oracle.cigar(A.oracle_states(q, t, oracle.ALIGN_MYERS, 6)) == "6M"
    assert A.oracle_states(q, t, oracle.ALIGN_UKKONEN, 6) == [0, 0, 0, 1, 1, 0]
    assert A.reverse_complement(b"ACGTNacgt\xc1-") == b"-\xc1tgcaNACGT"


def test_seam_lengths_are_exact():
    for f in ("homopolymer", "two_letter", "tandem"):
        pairs = A.seams(f)
        assert tuple(len(q) for q, _ in pairs[:len(A.SEAM_QUERY)]) == A.SEAM_QUERY
        rest = pairs[len(A.SEAM_QUERY):]
        assert [len(t) for _, t in rest] == [n for n in A.SEAM_TARGET for _ in range(2)] + list(A.SEAM_TARGET_TILE)
        assert [len(q) for q, _ in rest[:2 * len(A.SEAM_TARGET):2]] == [40] * len(A.SEAM_TARGET)
    assert tuple(len(q) for q, _ in A.seams_8k()) == A.SEAM_QUERY_8K
    gaps = A.long_gap()
    assert len(gaps) == 42 and sorted({abs(len(q) - len(t)) for q, t in gaps}) == sorted(A.LONG_GAPS)
