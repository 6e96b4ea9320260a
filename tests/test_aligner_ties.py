"""GPU parity of the four global aligners on the case families of
aligner_cases.py: inputs with many co-optimal paths (homopolymer runs, a
two-letter alphabet, tandem repeats, out-of-phase repeats), long gaps, bytes
outside ACGT on the target side, every seam length of the kernels, the band
classes of banded Myers and the band rows of Ukkonen, on every kernel route.
Each result must equal the oracle's path and pass a checker that does not use
the oracle; test_aligner_cases_cpu.py shows that the families really have
these properties."""
import pytest

import aligner_cases as A
from claragenomicsanalysis_amd.cudaaligner import CudaAlignerBatch

pytestmark = pytest.mark.gpu

BATCHES = A.batches()
ALGO = {name: (oalgo, rule) for name, oalgo, rule in A.ALGORITHMS}
SWITCHES = ("GWAMD_HM_STRIPE_BLOCKS", "GWAMD_BAND_WAVES", "GWAMD_BAND_TILE_BYTES", "GWAMD_BAND_SPEC",
            "GWAMD_UK_TILE_BYTES")
HM_ROUTES = [{}, {"GWAMD_HM_STRIPE_BLOCKS": "1"}, {"GWAMD_HM_STRIPE_BLOCKS": "2"}]
BANDED_ROUTES = [{}, {"GWAMD_BAND_WAVES": "1"}, {"GWAMD_BAND_WAVES": "4"}, {"GWAMD_BAND_TILE_BYTES": "4096"},
                 {"GWAMD_BAND_SPEC": "0"}, {"GWAMD_BAND_SPEC": "2"}]
UKKONEN_ROUTES = [{}, {"GWAMD_UK_TILE_BYTES": "1024"}]
ROUTES = ([("hirschberg_myers", r) for r in HM_ROUTES] + [("myers", {})] +
          [("myers_banded", r) for r in BANDED_ROUTES] + [("ukkonen", r) for r in UKKONEN_ROUTES])


def _route_id(r):
    algo, env = r
    return algo + "".join("-%s=%s" % (k[6:].lower(), v) for k, v in env.items())


def _set_route(monkeypatch, env):
    monkeypatch.setenv("GWAMD_DIAG", "1")
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _states(b, n):
    b.sync_alignments()
    paths, plen = b.raw_paths()
    return [paths[i, :plen[i]][::-1].tolist() for i in range(n)]


def gpu_states(pairs, algorithm, max_q=None, max_t=None, rc=False, stats=None, **kw):
    mq, mt = A.capacity(pairs, algorithm)
    b = CudaAlignerBatch(max_q or mq, max_t or mt, len(pairs), algorithm=algorithm, **kw)
    for q, t in pairs:
        assert b.add_alignment(q, t, rc, rc) == 0
    b.align_all()
    got = _states(b, len(pairs))
    if stats is not None:
        stats.update(b.stats())
    return got, (max_q or mq), b


def assert_parity(pairs, got, algorithm, max_q, exact=True):
    oalgo, rule = ALGO[algorithm]
    for k, ((q, t), g) in enumerate(zip(pairs, got)):
        assert g == A.oracle_states(q, t, oalgo, max_q), (algorithm, k, len(q), len(t))
        A.check_alignment(q, t, g, rule, band_limited=algorithm == "ukkonen", exact=exact)


@pytest.mark.parametrize("batch", sorted(BATCHES))
@pytest.mark.parametrize("route", ROUTES, ids=_route_id)
def test_family_matches_oracle(route, batch, monkeypatch):
    algorithm, env = route
    _set_route(monkeypatch, env)
    pairs = BATCHES[batch]
    got, mq, _ = gpu_states(pairs, algorithm)
    assert_parity(pairs, got, algorithm, mq)


@pytest.mark.parametrize("algorithm", sorted(ALGO))
def test_alphabet_reverse_complemented(algorithm, monkeypatch):
    # both flags set: A/C/G/T are complemented, every other byte is kept
    _set_route(monkeypatch, {})
    pairs = A.alphabet()
    got, mq, _ = gpu_states(pairs, algorithm, rc=True)
    flipped = [(A.reverse_complement(q), A.reverse_complement(t)) for q, t in pairs]
    assert flipped != list(pairs)
    assert_parity(flipped, got, algorithm, mq)


def test_alphabet_results_are_readable(monkeypatch):
    # get_alignments() on sequences with bytes >= 0x80 (it decoded the stored
    # sequences as UTF-8 and raised): one character per byte, the same states
    # as the raw paths, and a formatted alignment as long as the path
    _set_route(monkeypatch, {})
    pairs = A.alphabet()
    got, _, b = gpu_states(pairs, "myers")
    inv = {"m": 0, "mm": 1, "i": 2, "d": 3}
    for (q, t), g, a in zip(pairs, got, b.get_alignments()):
        assert a.query.encode("latin-1") == q and a.target.encode("latin-1") == t
        assert [inv[s] for s in a.alignment] == g and a.status == 0
        assert [len(row) for row in a.format_alignment] == [len(g)] * 3
        assert a.format_alignment[0].replace("-", "").encode("latin-1") == q.replace(b"-", b"")


def test_myers_8k_stripe_seam(monkeypatch):
    # queries of 8,191 / 8,192 / 8,193 rows: the last crosses the 8,192-row stripe
    _set_route(monkeypatch, {})
    pairs = A.seams_8k()
    got, mq, _ = gpu_states(pairs, "myers")
    assert_parity(pairs, got, "myers", mq)


@pytest.mark.parametrize("env", BANDED_ROUTES, ids=lambda e: _route_id(("banded", e)))
def test_banded_multi_chunk(env, monkeypatch):
    # bands of 58 and 258 words (2 and 9 chunks of 32): equal to the oracle,
    # which restates the reference's inexact chunk hand-over (check_alignment,
    # exact); a 4 KiB tile holds 256 band words, so the second pair's chunk
    # state goes through HBM
    _set_route(monkeypatch, env)
    pairs = A.banded()["multi_chunk"]
    st = {}
    got, mq, _ = gpu_states(pairs, "myers_banded", stats=st)
    assert_parity(pairs, got, "myers_banded", mq, exact=False)
    if "GWAMD_BAND_TILE_BYTES" in env:
        assert st["hbm_state_sweeps"] > 0
    else:
        assert st["hbm_state_sweeps"] == 0


@pytest.mark.parametrize("tile", [None, "1024"])
@pytest.mark.parametrize("diff", A.UKKONEN_WIDE_DIFFS)
def test_ukkonen_512_row_hand_over(diff, tile, monkeypatch):
    # a difference of 822 is 512 band rows, the single-wave kernel's last;
    # 824 is 513 rows: ukkonen_wide_kernel
    _set_route(monkeypatch, {"GWAMD_UK_TILE_BYTES": tile} if tile else {})
    pairs = A.ukkonen_wide(diff)
    st = {}
    got, mq, _ = gpu_states(pairs, "ukkonen", max_t=A.UKKONEN_WIDE_MAX_TARGET, stats=st)
    assert st["ukkonen_wide_pairs"] == (len(pairs) if A.ukkonen_band_rows(diff) > 512 else 0)
    assert_parity(pairs, got, "ukkonen", mq)


def test_max_query_length_changes_hirschberg_myers(monkeypatch):
    # one aligner per max_query_length; each equals the oracle at that value,
    # and the results differ between two values wherever the oracle's do
    _set_route(monkeypatch, {})
    pairs = A.max_query()
    values = A.MAX_QUERY_VALUES + (max(len(q) for q, _ in pairs),)
    got, want = {}, {}
    for mq in values:
        got[mq], _, _ = gpu_states(pairs, "hirschberg_myers", max_q=mq)
        assert_parity(pairs, got[mq], "hirschberg_myers", mq)
        want[mq] = [A.oracle_states(q, t, 0, mq) for q, t in pairs]
    for k, pair in enumerate(pairs):
        for a in values:
            for b in values:
                assert (got[a][k] == got[b][k]) == (want[a][k] == want[b][k]), (k, a, b)
        assert len({tuple(got[mq][k]) for mq in values}) >= A.max_query_regimes(pair)


def _unlike_pairs():
    tie, gap, alpha = A.tie_family("homopolymer"), A.long_gap(), A.alphabet()
    seam = A.seams("tandem")
    return [seam[12], ("", ""), gap[8], ("A", "A"), alpha[2],
            tie[11], ("", "ACGT"), gap[39], ("C", "G"), alpha[4],
            seam[10], ("ACGT", "")]


@pytest.mark.parametrize("algorithm", sorted(ALGO))
def test_two_slots_reused_by_unlike_pairs(algorithm, monkeypatch):
    # a caching budget of the fixed buffers plus two workspace slots: 12 pairs
    # that alternate a long tie-heavy pair, an empty one, a long gap, a single
    # base and an alphabet pair run six to a slot, each after an unlike one;
    # then again in the reverse order after reset()
    from test_aligner_plan import ENV_NAMES, _lib, plan
    for k in ENV_NAMES:  # plan() clears them (restored after the test)
        monkeypatch.setenv(k, "")
    pairs = _unlike_pairs()
    assert len(pairs) == 12
    mq, mt = A.capacity(pairs, algorithm)
    p = plan(_lib(), {}, [[a for a, _, _ in A.ALGORITHMS].index(algorithm), mq, mt, len(pairs), 0, 0, 0, 0, 0, 0, 0, 0])
    assert "error" not in p, p
    _set_route(monkeypatch, {})
    budget = p["fixed_bytes"] + 2 * p["slot_bytes"]
    b = CudaAlignerBatch(mq, mt, len(pairs), algorithm=algorithm, max_device_memory_allocator_caching_size=budget)
    assert b.config()[0] == 2
    for order in (pairs, pairs[::-1]):
        for q, t in order:
            assert b.add_alignment(q, t) == 0
        b.align_all()
        assert_parity(order, _states(b, len(order)), algorithm, mq)
        b.reset()
