"""Host parts of cudapolish's cut from CIGAR runs (include/gwamd_polish.h),
without a GPU: CIGAR text to ops, the host walk over runs against the model
(tests/polish_model.py) and against the walk over states on the expanded path,
the PAF reader against format_paf, and every refusal of
gwamd_window_segments_cigar before a device call."""
import ctypes as C
import random

import numpy as np
import pytest

import polish_cases as pc
import polish_cigar_cases as cc
import polish_model as pm
from claragenomicsanalysis_amd import cudamapper, cudapolish, load_library
from claragenomicsanalysis_amd._lib import last_error
from claragenomicsanalysis_amd.cudamapper import _overlap_array

CONVENTIONS = ("genomeworks", "sam")
WINDOW_LENGTHS = (1, 2, 7, 64, 500)

# ---- parsing ----------------------------------------------------------------------------------------


def test_cigar_ops_round_trips_every_letter_and_the_length_limits():
    for letter in cc.LETTERS:
        for length in (1, cc.MAX_LENGTH):
            ops = cudapolish.cigar_ops("%d%s" % (length, letter))
            assert ops.dtype == np.uint32 and ops.tolist() == [length << 4 | cc.LETTERS.index(letter)]
    assert [cc.LETTERS.index(c) for c in "MID=X"] == [0, 1, 2, 7, 8]  # BAM numbering
    text = "12M3I4D5=1X0M7N2S1H1P%d=" % cc.MAX_LENGTH
    assert cc.text_of(cudapolish.cigar_ops(text)) == text
    assert cudapolish.cigar_ops(text.encode()).tolist() == cudapolish.cigar_ops(text).tolist()
    assert len(cudapolish.cigar_ops("")) == 0


@pytest.mark.parametrize("text", ["M", "3M=", "3MI2D", "3Q", "3m", "3M 2I", "*", "%dM" % (1 << 28),
                                  "99999999999999999999M", "3M4", "7", "-3M"])
def test_cigar_ops_refuses_malformed_text(text):
    with pytest.raises(ValueError):
        cudapolish.cigar_ops(text)


def test_gwamd_cigar_ops_counts_and_checks_the_capacity():
    L = load_library()
    n = C.c_int64(-1)
    assert L.gwamd_cigar_ops(b"3M2I", 4, None, 0, C.byref(n)) == 0 and n.value == 2
    out = (C.c_uint32 * 1)()
    assert L.gwamd_cigar_ops(b"3M2I", 4, out, 1, C.byref(n)) == -1 and n.value == 2 and "capacity" in last_error()
    assert L.gwamd_cigar_ops(b"3M2I", 2, out, 1, C.byref(n)) == 0 and n.value == 1 and out[0] == 3 << 4
    assert L.gwamd_cigar_ops(None, 4, None, 0, C.byref(n)) == -1
    assert L.gwamd_cigar_ops(b"3M", 2, None, 0, None) == -1


# ---- the host walk ----------------------------------------------------------------------------------


def host_walk(overlap, text, w, convention, index=0):
    return pc.as_tuples(cudapolish.window_segments_cigar_host(overlap, text, w, convention, overlap_index=index))


CASES = pc.hand_cases()


@pytest.mark.parametrize("convention", CONVENTIONS)
@pytest.mark.parametrize("name,overlap,path,expected", CASES, ids=[c[0] for c in CASES])
def test_host_walk_on_hand_cases(name, overlap, path, expected, convention):
    strand = overlap[6]
    for use_m in (False, True):
        text = cc.cigar_of(path, strand, convention, use_m)
        states = [9 if s not in (0, 1, 2, 3) else 0 if s == 1 and use_m else s for s in path]
        assert cc.expand(text, strand, convention) == states
        assert host_walk(overlap, text, pc.W, convention) == expected
        # ops in place of text
        got = cudapolish.window_segments_cigar_host(overlap, cudapolish.cigar_ops(text), pc.W, convention)
        assert pc.as_tuples(got) == expected


def random_case(rng, max_length=120):
    """(spans, path): a path that fits, or one with a state too many or too few."""
    tl, ql = rng.randint(0, max_length), rng.randint(0, max_length)
    ts, qs = rng.randint(0, 40), rng.randint(0, 40)
    path = pc.random_path(rng, tl, ql)
    kind = rng.random()
    if kind < 0.1 and path:
        del path[rng.randrange(len(path))]
    elif kind < 0.2 and len(path) < tl + ql:
        path.insert(rng.randrange(len(path) + 1), rng.choice((0, 2, 3)))
    return (qs, qs + ql, ts, ts + tl), path


def test_host_walk_on_random_paths():
    rng = random.Random(20250301)
    flagged = 0
    for i in range(300):
        spans, path = random_case(rng)
        for strand in "+-":
            overlap = pc.overlap_of(spans, strand)
            for convention in CONVENTIONS:
                text = cc.cigar_of(path, strand, convention, use_m=i % 3 == 0)
                states = cc.expand(text, strand, convention)
                for w in WINDOW_LENGTHS:
                    expected = pm.segments(i, overlap, states, w)
                    assert host_walk(overlap, text, w, convention, i) == expected, (overlap, text, w, convention)
                    by_states = cudapolish.window_segments_host(overlap, states, w, overlap_index=i)
                    assert pc.as_tuples(by_states) == expected
                    if convention == "sam":  # SAM's own definition, without the normalisation
                        assert cc.sam_segments(i, overlap, text, w) == expected
            flagged += any(r[6] & pm.BAD_PATH for r in expected)
    assert 50 < flagged < 400  # both kinds are exercised


@pytest.mark.parametrize("convention", CONVENTIONS)
@pytest.mark.parametrize("strand", "+-")
def test_host_walk_misfits(strand, convention):
    overlap = pc.overlap_of((3, 11, 5, 13), strand)
    bad = cc.misfit_records(0, overlap, 4)
    assert len(bad) == 3
    assert host_walk(overlap, "8M", 4, convention) == pm.segments(0, overlap, [0] * 8, 4)
    for letter in "NSHP":  # forbidden ops, also of length 0
        for text in ("4M1%s4M" % letter, "8M0%s" % letter, "1%s" % letter):
            assert host_walk(overlap, text, 4, convention) == bad, text
    for code in range(9, 16):
        ops = np.array([4 << 4, code, 4 << 4], np.uint32)
        assert pc.as_tuples(cudapolish.window_segments_cigar_host(overlap, ops, 4, convention)) == bad
    for text in ("7M", "9M", "8M1I", "8M1D", "4M1I4M", "", "8I7D"):
        assert host_walk(overlap, text, 4, convention) == bad, text
    # a path without a match state fits: every window empty, none flagged bad
    assert host_walk(overlap, "8I8D", 4, convention) == [r[:6] + (r[6] & ~pm.BAD_PATH, 0) for r in bad]
    # zero-length ops contribute nothing
    assert host_walk(overlap, "0M0I4=0D0X4X0=", 4, convention) == host_walk(overlap, "8M", 4, convention)
    # advances of 2^32 + 100 do not wrap into the spans (100, 100)
    wrap = pc.overlap_of(cc.WRAP_SPANS, strand)
    assert host_walk(wrap, cc.WRAP_CIGAR, 64, convention) == cc.misfit_records(0, wrap, 64)
    assert host_walk(wrap, "100M", 64, convention) == pm.segments(0, wrap, [0] * 100, 64)


def test_host_walk_refusals():
    overlap = pc.overlap_of((0, 8, 0, 8), "+")
    with pytest.raises(ValueError):
        cudapolish.window_segments_cigar_host(overlap, "8M", 0)
    with pytest.raises(ValueError):
        cudapolish.window_segments_cigar_host(pc.overlap_of((8, 0, 0, 8), "+"), "8M", 4)
    with pytest.raises(ValueError):
        cudapolish.window_segments_cigar_host(overlap, "8M", 4, convention="bam")
    with pytest.raises(ValueError):
        cudapolish.window_segments_cigar_host(overlap, "8Q", 4)
    L = load_library()
    p, m = C.c_void_p(), C.c_int64()
    ops = (C.c_uint32 * 1)(8 << 4)
    arr = _overlap_array([overlap])
    assert L.gwamd_window_segments_cigar_host(arr, ops, 1, 2, 4, 0, C.byref(p), C.byref(m)) == -1
    assert "convention" in last_error() and not p.value
    assert L.gwamd_window_segments_cigar_host(arr, None, 1, 0, 4, 0, C.byref(p), C.byref(m)) == -1
    assert L.gwamd_window_segments_cigar_host(arr, ops, -1, 0, 4, 0, C.byref(p), C.byref(m)) == -1
    assert L.gwamd_window_segments_cigar_host(None, ops, 1, 0, 4, 0, C.byref(p), C.byref(m)) == -1


# ---- PAF --------------------------------------------------------------------------------------------

QUERIES = [("read/1", 900), ("read/2", 1200), ("r3", 50)]
TARGETS = [("contig_a", 5000), ("contig_b", 700)]


def paf_input():
    overlaps = [cudamapper.Overlap(0, 1, 10, 410, 100, 520, "+", num_residues=12),
                cudamapper.Overlap(1, 0, 0, 1200, 3000, 4100, "-", num_residues=40),
                cudamapper.Overlap(2, 0, 5, 5, 20, 20, "+", num_residues=0),
                cudamapper.Overlap(1, 1, 0, 700, 0, 700, "-", num_residues=3, overlap_complete=True)]
    cigars = ["400=20I", "100=100D1000X", "", "700M"]
    return overlaps, cigars


def fields(o):
    return (o.query_read_id, o.target_read_id, o.query_start, o.query_end, o.target_start, o.target_end, o.strand,
            o.num_residues)


@pytest.mark.parametrize("kmer_size", [1, 15])
def test_paf_round_trip(kmer_size, tmp_path):
    overlaps, cigars = paf_input()
    names = [q[0] for q in QUERIES], [t[0] for t in TARGETS]
    text = cudamapper.format_paf(overlaps, cigars, QUERIES, TARGETS, kmer_size)
    assert text.count("\n") == 4 and text.count("cg:Z:") == 3
    got, got_cigars = cudamapper.read_paf(text, *names, kmer_size=kmer_size)
    assert [fields(o) for o in got] == [fields(o) for o in overlaps]
    assert all(o.overlap_complete == 0 for o in got)
    assert [cc.text_of(c) for c in got_cigars] == cigars and all(c.dtype == np.uint32 for c in got_cigars)
    # from a file, with blank lines and CRLF, the tag among other tags
    lines = text.split("\n")
    lines[0] = lines[0].replace("\tcg:Z:", "\tNM:i:3\ttp:A:P\tcg:Z:") + "\tzz:Z:5M"
    path = tmp_path / "overlaps.paf"
    path.write_bytes(("\n" + "\r\n".join(lines)).encode())
    for source in (str(path), path):
        again, again_cigars = cudamapper.read_paf(source, *names, kmer_size=kmer_size)
        assert [fields(o) for o in again] == [fields(o) for o in overlaps]
        assert [cc.text_of(c) for c in again_cigars] == cigars
    # no CIGARs at all
    plain = cudamapper.format_paf(overlaps, None, QUERIES, TARGETS, kmer_size)
    assert "cg:Z:" not in plain
    got, got_cigars = cudamapper.read_paf(plain, *names, kmer_size=kmer_size)
    assert [fields(o) for o in got] == [fields(o) for o in overlaps] and [len(c) for c in got_cigars] == [0] * 4
    assert cudamapper.read_paf("", *names) == ([], [])


def test_paf_refusals_name_the_line(tmp_path):
    names = [q[0] for q in QUERIES], [t[0] for t in TARGETS]
    good = "r3\t50\t0\t50\t+\tcontig_b\t700\t10\t60\t50\t50\t255"
    assert len(cudamapper.read_paf(good + "\n", *names)[0]) == 1
    cols = good.split("\t")

    def with_column(i, value):
        return "\t".join(cols[:i] + [value] + cols[i + 1:])

    bad_lines = [("unknown query", with_column(0, "r4")), ("unknown target", with_column(5, "contig")),
                 ("12 columns", "\t".join(cols[:11])), ("strand", with_column(4, "*")),
                 ("start > end", with_column(2, "51")), ("start > end", with_column(7, "61")),
                 ("beyond", with_column(3, "51")), ("beyond", with_column(8, "701")),
                 ("not a number", with_column(2, "x")), ("CIGAR", good + "\tcg:Z:5Q")]
    for what, line in bad_lines:
        for number in (1, 3):
            text = (good + "\n") * (number - 1) + line + "\n" + good + "\n"
            with pytest.raises(ValueError) as e:
                cudamapper.read_paf(text, *names)
            assert "line %d:" % number in str(e.value) and what in str(e.value), (what, str(e.value))
    with pytest.raises(ValueError):
        cudamapper.read_paf(good + "\n", *names, kmer_size=0)
    with pytest.raises(RuntimeError):
        cudamapper.read_paf(str(tmp_path / "missing.paf"), *names)
    L = load_library()
    h = C.c_void_p()
    off = (C.c_int64 * 1)(0)
    assert L.gwamd_read_paf(None, None, 0, None, off, 0, None, off, 0, 1, C.byref(h)) == -1 and not h.value
    assert L.gwamd_read_paf(b"a", b"b", 1, None, off, 0, None, off, 0, 1, C.byref(h)) == -1 and not h.value
    assert L.gwamd_read_paf(None, b"", 0, None, off, 0, None, off, 0, 1, None) == -1


# ---- refusals of the device entry point -------------------------------------------------------------


def call_cigar(overlaps, n, ops, offsets, w, convention=0, device_id=1 << 20, out=True, num_out=True):
    L = load_library()
    p, m = C.c_void_p(), C.c_int64(-5)
    rc = L.gwamd_window_segments_cigar(overlaps, n, ops, offsets, convention, w, device_id, None,
                                       C.byref(p) if out else None, C.byref(m) if num_out else None)
    assert not p.value
    return rc


def test_window_segments_cigar_refusals():
    arr = _overlap_array([pc.overlap_of((0, 8, 0, 8), "+")])
    ops = (C.c_uint32 * 4)(8 << 4)
    off = (C.c_int64 * 2)(0, 1)
    # the device does not exist and is never reached: each of these is refused before a device call
    assert call_cigar(None, 1, ops, off, 4) == -1 and "overlaps is NULL" in last_error()
    assert call_cigar(arr, 1, None, off, 4) == -1 and "ops is NULL" in last_error()
    assert call_cigar(arr, 1, ops, None, 4) == -1 and "op_offsets is NULL" in last_error()
    assert call_cigar(arr, 1, ops, off, 4, out=False) == -1
    assert call_cigar(arr, 1, ops, off, 4, num_out=False) == -1
    assert call_cigar(arr, -1, ops, off, 4) == -1
    assert call_cigar(arr, 1 << 31, ops, off, 4) == -1
    assert call_cigar(arr, 1, ops, off, 0) == -1 and "window_length" in last_error()
    assert call_cigar(arr, 1, ops, off, -4) == -1
    assert call_cigar(arr, 1, ops, off, 4, device_id=-1) == -1 and "device_id" in last_error()
    for convention in (-1, 2, 7):
        assert call_cigar(arr, 1, ops, off, 4, convention=convention) == -1 and "convention" in last_error()
    assert call_cigar(arr, 1, ops, (C.c_int64 * 2)(1, 0), 4) == -1 and "non-decreasing" in last_error()
    assert call_cigar(arr, 1, ops, (C.c_int64 * 2)(-1, 1), 4) == -1
    for bad in ((0, 0, 9, 8, 0, 8, "+"), (0, 0, 0, 8, 9, 8, "+"), (0, 0, 0, 8, 0, 8, "x")):
        assert call_cigar(_overlap_array([bad]), 1, ops, off, 4) == -1, bad
    wide = _overlap_array([(0, 0, 0, 0, 0, (1 << 31) - 1, "+")] * 3)
    assert call_cigar(wide, 3, ops, (C.c_int64 * 4)(0, 0, 0, 0), 1) == -1 and "2^31" in last_error()
    # nothing to do: no device call either
    p, m = C.c_void_p(), C.c_int64(-5)
    assert load_library().gwamd_window_segments_cigar(None, 0, None, None, 0, 4, 1 << 20, None, C.byref(p),
                                                      C.byref(m)) == 0
    assert not p.value and m.value == 0
    with pytest.raises(ValueError):
        cudapolish.window_segments_cigar([pc.overlap_of((0, 8, 0, 8), "+")], [], 4)
    with pytest.raises(ValueError):
        cudapolish.window_segments_cigar([pc.overlap_of((0, 8, 0, 8), "+")], ["8M"], 4, convention="bam")
    with pytest.raises(ValueError):
        cudapolish.window_segments_cigar([pc.overlap_of((0, 8, 0, 8), "+")], ["8Q"], 4)


def test_polish_refuses_another_number_of_cigars_before_any_device_call():
    _, draft, queries, overlaps = pc.e2e_input(length=60, reads=3)
    # the device does not exist: a call that reached it would not raise ValueError
    with pytest.raises(ValueError, match="CIGARs for 3 overlaps"):
        cudapolish.polish([draft], queries, overlaps, cigars=["60M"] * 2, device_id=1 << 20)
    with pytest.raises(ValueError, match="convention"):
        cudapolish.polish([draft], queries, overlaps, cigars=["60M"] * 3, cigar_convention="bam", device_id=1 << 20)


def test_cpp_interface_host_part(tmp_path):
    import subprocess
    r = subprocess.run([cc.build_cpp_check(tmp_path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == [word for name in cc.CPP_HOST for word in ("ok", name)]
