"""cudapolish's cut from CIGAR runs on the GPU against the plain-Python model
(tests/polish_model.py) on the expanded state path: every word of every record.

The kernel walks an overlap's ops in tiles of TILE = 64, a lane one op, one
wave per overlap, four waves per workgroup.  A match run that crosses more
than OWN_CROSSINGS = 2 window boundaries is spread over the wave, boundaries
lane, lane + 64, ...; the cases sit below, at and above each of these sizes.
"""
import random

import numpy as np
import pytest

import polish_cases as pc
import polish_cigar_cases as cc
import polish_model as pm

pytestmark = pytest.mark.gpu

T = cc.TILE
CONVENTIONS = ("genomeworks", "sam")


@pytest.fixture(scope="module")
def cudapolish():
    from claragenomicsanalysis_amd import cudapolish
    return cudapolish


def expected_of(overlaps, texts, w, convention="genomeworks"):
    out = []
    for i, (o, text) in enumerate(zip(overlaps, texts)):
        out += pm.segments(i, o, cc.expand(text, o[6], convention), w)
    return out


def check(cudapolish, overlaps, texts, w, convention="genomeworks"):
    """The cut of the texts equals the model; returns the records."""
    got = pc.as_tuples(cudapolish.window_segments_cigar(overlaps, texts, w, convention))
    assert got == expected_of(overlaps, texts, w, convention), (w, convention)
    return got


def spans_of(text, convention="genomeworks"):
    """(query span, target span) a CIGAR advances."""
    states = cc.expand(text, "+", convention)
    return sum(s != 2 for s in states), sum(s != 3 for s in states)


def overlap_for(text, strand, ts, qs, convention="genomeworks"):
    ql, tl = spans_of(text, convention)
    return (0, 0, qs, qs + ql, ts, ts + tl, strand)


def random_ops(rng, count, letters="=XIDM", longest=6):
    return "".join("%d%s" % (rng.randint(0, longest), rng.choice(letters)) for _ in range(count))


@pytest.mark.parametrize("convention", CONVENTIONS)
def test_hand_cases(cudapolish, convention):
    cases = pc.hand_cases()
    overlaps = [c[1] for c in cases]
    texts = [cc.cigar_of(c[2], c[1][6], convention, use_m=i % 2 == 1) for i, c in enumerate(cases)]
    got = check(cudapolish, overlaps, texts, pc.W, convention)
    expected = []
    for i, case in enumerate(cases):
        expected += [(i,) + r[1:] for r in case[3]]
    assert got == expected


@pytest.mark.parametrize("w", [1, 3, 500])
def test_op_counts_at_tile_edges(cudapolish, w):
    rng = random.Random(1000 + w)
    overlaps, texts = [], []
    for count in (0, 1, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1):
        for strand in "+-":
            text = random_ops(rng, count)
            assert len(cc.parse(text)) == count
            overlaps.append(overlap_for(text, strand, rng.randint(0, 20), rng.randint(0, 20)))
            texts.append(text)
    check(cudapolish, overlaps, texts, w)
    sam = [cc.to_sam(t, o[6]) for o, t in zip(overlaps, texts)]
    assert check(cudapolish, overlaps, sam, w, "sam") == expected_of(overlaps, texts, w)


CROSSINGS = [0, 1, cc.OWN_CROSSINGS, cc.OWN_CROSSINGS + 1, 63, 64, 65, 127, 128, 129, 200]


@pytest.mark.parametrize("strand", "+-")
def test_one_match_run_over_many_windows(cudapolish, strand):
    w = 5
    overlaps, texts = [], []
    for crossings in CROSSINGS:
        for ts in (13, 10):  # not a multiple of w, and one
            # the run's last base sits in window ts // w + crossings: at its first place, or at its last (te on a
            # boundary)
            for length in (crossings * w + 1, (crossings + 1) * w - ts % w):
                assert (ts + length - 1) // w - ts // w == crossings
                # alone, and in another lane than the first with gaps and a match state around it
                for text in ("%d=" % length, "2I1D%dM3D" % length, "1=3I%dX2I1=" % length):
                    overlaps.append(overlap_for(text, strand, ts, 7))
                    texts.append(text)
    assert any(o[5] % w == 0 for o in overlaps) and any(o[5] % w for o in overlaps)
    got = check(cudapolish, overlaps, texts, w)
    assert not any(r[6] & pm.BAD_PATH for r in got)
    # windows of one base: every base of a run of 300 is a window of its own
    run = [overlap_for("300=", strand, 17, 4), overlap_for("3D300M2I", strand, 0, 0)]
    got = check(cudapolish, run, ["300=", "3D300M2I"], 1)
    assert len(got) == 602 and sum(bool(r[6] & pm.EMPTY) for r in got) == 2


@pytest.mark.parametrize("w", [4, 7])
def test_windows_without_a_match_state_between_runs(cudapolish, w):
    rng = random.Random(w)
    gaps = "".join("3I2D" for _ in range(T // 2))  # a whole tile of gap ops: 96 target bases
    texts = [
        # the last match op of tile 0, a tile of gaps only, the first op of tile 2
        random_ops(rng, T - 1, "=XID", 2) + "5=" + gaps + "6X" + random_ops(rng, 9),
        # gap stretches that cover whole windows inside one tile
        "3=%dI2X%dI%dD1=" % (3 * w, 2 * w + 1, w),
        "%dI4=%dI" % (2 * w, 2 * w),
        # a tile of gaps before the first match run and after the last
        gaps + "9=" + gaps,
    ]
    overlaps = [overlap_for(t, "+-"[i % 2], i * 3, i) for i, t in enumerate(texts)]
    overlaps += [o[:6] + ("-" if o[6] == "+" else "+",) for o in overlaps]
    got = check(cudapolish, overlaps, texts + texts, w)
    assert sum(bool(r[6] & pm.EMPTY) for r in got) > 40 and not any(r[6] & pm.BAD_PATH for r in got)


@pytest.mark.parametrize("w", [3, 500])
def test_adjacent_match_ops_in_one_window(cudapolish, w):
    texts = [
        "1=1X",
        "2M3M",
        # neighbouring lanes all along tile 0, and = then X across the seam to tile 1
        "1=1X" * (T // 2) + "1=1X",
        "1I" * (T - 1) + "1=" + "1X" + "2D",
        "1M" * (2 * T + 1),
    ]
    overlaps = [overlap_for(t, "+-"[i % 2], 2 * i + 1, 5) for i, t in enumerate(texts)]
    overlaps += [o[:6] + ("-" if o[6] == "+" else "+",) for o in overlaps]
    check(cudapolish, overlaps, texts + texts, w)


def test_zero_length_ops(cudapolish):
    texts = ["0M0I3=0D0X2I0=4X0D", "0=", "0I0D", "0M" * (T + 1) + "9=" + "0X" * T, "5=0I5=", "0D7M"]
    overlaps = [overlap_for(t, "+-"[i % 2], i, 2 * i) for i, t in enumerate(texts)]
    got = check(cudapolish, overlaps, texts, 4)
    assert not any(r[6] & pm.BAD_PATH for r in got)
    plain = ["3=2I4X", "", "", "9=", "10=", "7M"]
    assert got == expected_of(overlaps, plain, 4)


def test_ops_begin_at_every_word_offset(cudapolish):
    rng = random.Random(8)
    counts = [1] * 8 + [3, 5, 7, 2, T + 3, 6, 1, 1]
    texts = [random_ops(rng, c, "=XID") for c in counts]
    assert {sum(counts[:i]) % 8 for i in range(len(counts))} == set(range(8))
    overlaps = [overlap_for(t, "+-"[i % 2], rng.randint(0, 30), rng.randint(0, 30)) for i, t in enumerate(texts)]
    check(cudapolish, overlaps, texts, 3)
    # ops handed over as arrays, the first overlap's not at the start of the caller's array
    arrays = [cudapolish.cigar_ops(t) for t in texts]
    got = pc.as_tuples(cudapolish.window_segments_cigar(overlaps, arrays, 3))
    assert got == expected_of(overlaps, texts, 3)


def random_overlaps(rng, count, longest=90):
    overlaps, texts = [], []
    for _ in range(count):
        tl, ql = rng.randint(0, longest), rng.randint(0, longest)
        strand = rng.choice("+-")
        texts.append(cc.cigar_of(pc.random_path(rng, tl, ql), strand, use_m=rng.random() < 0.3))
        ts, qs = rng.randint(0, 50), rng.randint(0, 50)
        overlaps.append((0, 0, qs, qs + ql, ts, ts + tl, strand))
    return overlaps, texts


@pytest.mark.parametrize("count", range(1, 10))
def test_overlap_counts(cudapolish, count):
    overlaps, texts = random_overlaps(random.Random(count), count)
    check(cudapolish, overlaps, texts, 8)


@pytest.mark.parametrize("w", [1, 2, 3, 500, (1 << 31) - 1])
def test_window_lengths(cudapolish, w):
    # the kernel divides by w with a reciprocal the host prepares, and multiplies back at a boundary
    rng = random.Random(w)
    overlaps, texts = [], []
    for _ in range(6):
        tl, ql = rng.randint(1, 700), rng.randint(1, 700)
        strand = rng.choice("+-")
        texts.append(cc.cigar_of(pc.random_path(rng, tl, ql), strand))
        ts = rng.choice((0, 5, w - 1, w, 2 * w + 3, (1 << 31) - 1 - tl))
        ts = max(0, min(ts, (1 << 31) - 1 - tl))
        overlaps.append((0, 0, 7, 7 + ql, ts, ts + tl, strand))
    # one run across the boundary at the largest positions there are
    for strand in "+-":
        overlaps.append((0, 0, (1 << 31) - 1 - 400, (1 << 31) - 1, (1 << 31) - 1 - 400, (1 << 31) - 1, strand))
        texts.append("400M")
    check(cudapolish, overlaps, texts, w)


@pytest.mark.parametrize("w", [7, 64, 500])
def test_random_overlaps(cudapolish, w):
    rng = random.Random(5000 + w)
    overlaps, texts = random_overlaps(rng, 200, 1500)
    check(cudapolish, overlaps, texts, w)
    sam = [cc.to_sam(t, o[6]) for o, t in zip(overlaps, texts)]
    assert check(cudapolish, overlaps, sam, w, "sam") == expected_of(overlaps, texts, w)


# ---- misfits ------------------------------------------------------------------------------------------


def misfit_call(rng):
    """(overlaps, CIGARs as ops, which are misfits): each misfit between two overlaps that fit."""
    def good():
        tl, ql = rng.randint(20, 300), rng.randint(20, 300)
        strand = rng.choice("+-")
        text = cc.cigar_of(pc.random_path(rng, tl, ql), strand)
        ts, qs = rng.randint(0, 50), rng.randint(0, 50)
        return (0, 0, qs, qs + ql, ts, ts + tl, strand), text

    bad = [
        ((0, 0, 3, 103, 11, 111, "+"), "60=39X"),                      # short by one
        ((0, 0, 3, 103, 11, 111, "-"), "50=1I1D50X"),                   # long by one
        ((0, 0, 3, 103, 11, 112, "+"), "100M"),                         # the target short by one
        ((0, 0, 3, 104, 11, 111, "-"), "100M"),                         # the query short by one
        ((0, 0, 0, 100, 0, 100, "+"), cc.WRAP_CIGAR),                   # 2^32 + 100 of each: no wrap into a fit
        ((0, 0, 5, 105, 40, 140, "-"), cc.WRAP_CIGAR),
        ((0, 0, 0, 100, 0, 100, "+"), "%dI%dD" % (cc.MAX_LENGTH, cc.MAX_LENGTH) * 16 + "116I116D"),
        ((0, 0, 0, 20, 7, 17, "+"), "5=5D10="),                         # the last run overshoots only the target
        ((0, 0, 0, 20, 7, 17, "-"), "5=5D10="),
        ((0, 0, 0, 10, 7, 27, "+"), "5=5I10="),                         # ... only the query
        ((0, 0, 0, 9, 7, 16, "+"), ""),                                 # no op for spans that are not empty
    ]
    ops = [cudapolish_ops(text) for _, text in bad]
    for code in (3, 4, 5, 6) + tuple(range(9, 16)):                     # each forbidden op code
        bad.append(((0, 0, 2, 10, 9, 17, "+-"[code % 2]), None))
        ops.append(np.array([4 << 4 | 7, (code % 2) << 4 | code, 4 << 4 | 8], np.uint32))
    overlaps, cigars, flagged = [], [], []
    for (overlap, _), packed in zip(bad, ops):
        o, text = good()
        overlaps += [o, overlap]
        cigars += [cudapolish_ops(text), packed]
        flagged.append(len(overlaps) - 1)
    o, text = good()
    return overlaps + [o], cigars + [cudapolish_ops(text)], flagged


def cudapolish_ops(text):
    from claragenomicsanalysis_amd import cudapolish
    return cudapolish.cigar_ops(text)


@pytest.mark.parametrize("w", [3, 16])
def test_misfits_in_the_middle_of_a_call(cudapolish, w):
    overlaps, cigars, flagged = misfit_call(random.Random(31))
    assert len(flagged) == 22
    expected = []
    for i, (o, ops) in enumerate(zip(overlaps, cigars)):
        if i in flagged:
            expected += cc.misfit_records(i, o, w)
        else:
            records = pm.segments(i, o, cc.expand(cc.text_of(ops)), w)
            assert not any(r[6] & pm.BAD_PATH for r in records)
            expected += records
    assert pc.as_tuples(cudapolish.window_segments_cigar(overlaps, cigars, w)) == expected
    # the host walk says the same of each
    for i, (o, ops) in enumerate(zip(overlaps, cigars)):
        assert pc.as_tuples(cudapolish.window_segments_cigar_host(o, ops, w, overlap_index=i)) == \
            [r for r in expected if r[0] == i]


def test_pool_is_returned(cudapolish):
    from claragenomicsanalysis_amd.cudaaligner import DeviceAllocator
    pool = DeviceAllocator(64 << 20)
    overlaps, texts = random_overlaps(random.Random(5), 20, 400)
    assert pool.used == 0
    got = pc.as_tuples(cudapolish.window_segments_cigar(overlaps, texts, 8, allocator=pool))
    assert pool.used == 0 and got == expected_of(overlaps, texts, 8)
    small = DeviceAllocator(1 << 10)
    with pytest.raises(RuntimeError):
        cudapolish.window_segments_cigar(overlaps, texts, 8, allocator=small)
    assert small.used == 0


# ---- the routes agree ---------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def resident_input():
    """12 reads of about 1.2 kb against two targets, both strands, partial overlaps among them."""
    rng = random.Random(12)
    truth = ["".join(rng.choice("ACGT") for _ in range(1200)) for _ in range(2)]
    queries, overlaps = [], []
    for i in range(12):
        t = i % 2
        read = pc.mutate(rng, truth[t], 0.08)
        reverse = i % 3 == 0
        queries.append(pm.reverse_complement(read) if reverse else read)
        if i < 8:
            overlaps.append((i, t, 0, len(read), 0, 1200, "-" if reverse else "+"))
        else:  # a part of the read against a part of the target
            overlaps.append((i, t, 100, len(read) - 150, 130, 1010, "-" if reverse else "+"))
    overlaps.append((3, 1, 40, 40, 500, 500, "+"))  # nothing to align, no record
    overlaps.append((4, 0, 10, 10, 300, 420, "-"))  # a target span without a query base
    return truth, queries, overlaps


@pytest.mark.parametrize("w", [16, 500])
def test_cigar_route_equals_resident_route(cudapolish, resident_input, w):
    from claragenomicsanalysis_amd.cudamapper import DeviceReads, align_overlaps, format_paf, read_paf
    targets, queries, overlaps = resident_input
    with DeviceReads(queries) as q, DeviceReads(targets) as t:
        cigars = align_overlaps(overlaps, q, t)
        resident = pc.as_tuples(cudapolish.window_segments_resident(overlaps, q, t, w))
    assert not any(r[6] & (pm.BAD_PATH | pm.NOT_ALIGNED) for r in resident)
    assert pc.as_tuples(cudapolish.window_segments_cigar(overlaps, cigars, w)) == resident
    sam = [cc.to_sam(c, o[6]) for o, c in zip(overlaps, cigars)]
    assert sam != cigars
    assert pc.as_tuples(cudapolish.window_segments_cigar(overlaps, sam, w, convention="sam")) == resident
    # and through PAF text, as cudamapper -a prints it
    names = ["q%d" % i for i in range(len(queries))], ["t%d" % i for i in range(len(targets))]
    paf = format_paf(overlaps, cigars, list(zip(names[0], queries)), list(zip(names[1], targets)), 15)
    read, read_cigars = read_paf(paf, *names, kmer_size=15)
    assert pc.as_tuples(cudapolish.window_segments_cigar(read, read_cigars, w)) == resident


@pytest.mark.parametrize("device_windows", [False, True])
def test_polish_with_cigars_equals_polish(cudapolish, monkeypatch, device_windows):
    from claragenomicsanalysis_amd.cudamapper import align_overlaps
    _, draft, queries, overlaps = pc.e2e_input()
    kwargs = dict(window_length=pc.E2E_W, device_windows=device_windows, max_gpu_mem=1 << 30)
    expected = cudapolish.polish([draft], queries, overlaps, **kwargs)
    cigars = align_overlaps(overlaps, queries, [draft])

    def no_aligner(*args, **kw):
        raise AssertionError("polish(cigars=) aligned the overlaps again")

    monkeypatch.setattr(cudapolish, "window_segments_resident", no_aligner)
    assert cudapolish.polish([draft], queries, overlaps, cigars=cigars, **kwargs) == expected
    if device_windows:  # and from ops in SAM's convention
        sam = [cudapolish.cigar_ops(cc.to_sam(c, o[6])) for o, c in zip(overlaps, cigars)]
        assert cudapolish.polish([draft], queries, overlaps, cigars=sam, cigar_convention="sam", **kwargs) == expected
    assert expected[1]["windows"] > 1 and expected[1]["backbone_by_rule"] == 0


def test_cpp_interface(tmp_path):
    import subprocess
    r = subprocess.run([cc.build_cpp_check(tmp_path), "gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == [word for name in cc.CPP_HOST + cc.CPP_GPU for word in ("ok", name)]
