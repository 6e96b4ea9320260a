"""Host parts of cudapolish over the C ABI (include/gwamd_polish.h), without a
GPU: every argument refusal of gwamd_window_segments and _resident comes back
before a device call, gwamd_window_segments_host equals the model
(tests/polish_model.py) and gwamd_build_windows equals the model's grouping."""
import ctypes as C
import random

import numpy as np
import pytest

import polish_cases as pc
import polish_model as pm
from claragenomicsanalysis_amd import cudapolish, load_library
from claragenomicsanalysis_amd._lib import last_error
from claragenomicsanalysis_amd.cudamapper import Overlap, _overlap_array

CASES = pc.hand_cases()


@pytest.mark.parametrize("name,overlap,path,expected", CASES, ids=[c[0] for c in CASES])
def test_host_walk_on_hand_cases(name, overlap, path, expected):
    assert pc.as_tuples(cudapolish.window_segments_host(overlap, path, pc.W)) == expected


def random_case(rng, max_length=120):
    tl, ql = rng.randint(0, max_length), rng.randint(0, max_length)
    ts, qs = rng.randint(0, 40), rng.randint(0, 40)
    path = pc.random_path(rng, tl, ql)
    kind = rng.random()
    if kind < 0.1 and path:
        path[rng.randrange(len(path))] = rng.choice((4, 7, -1, 127, -128))
    elif kind < 0.2 and path:
        del path[rng.randrange(len(path))]
    elif kind < 0.3 and len(path) < tl + ql:
        path.insert(rng.randrange(len(path) + 1), rng.choice((0, 2, 3)))
    return (0, 0, qs, qs + ql, ts, ts + tl, rng.choice("+-")), path


def test_host_walk_on_random_paths():
    rng = random.Random(20240607)
    flagged = 0
    for i in range(400):
        overlap, path = random_case(rng)
        w = rng.choice((1, 3, 4, 7, 8, 16, 50, 1000))
        expected = pm.segments(i, overlap, path, w)
        assert pc.as_tuples(cudapolish.window_segments_host(overlap, path, w, overlap_index=i)) == expected, \
            (overlap, path, w)
        flagged += any(r[6] & pm.BAD_PATH for r in expected)
    assert 40 < flagged < 200  # both kinds are exercised


# ---- refusals ---------------------------------------------------------------------------------------


def call_segments(overlaps, n, states, offsets, w, device_id=0, out=True, num_out=True):
    L = load_library()
    p, m = C.c_void_p(), C.c_int64(-5)
    rc = L.gwamd_window_segments(overlaps, n, states, offsets, w, device_id, None,
                                 C.byref(p) if out else None, C.byref(m) if num_out else None)
    assert not p.value
    return rc


def test_window_segments_refusals():
    arr = _overlap_array([pc.overlap_of((0, 8, 0, 8), "+")])
    states = (C.c_int8 * 32)()
    off = (C.c_int64 * 2)(0, 8)
    # a device that does not exist is never reached: each of these is refused before a device call
    dev = 1 << 20
    assert call_segments(None, 1, states, off, 4, dev) == -1 and "overlaps is NULL" in last_error()
    assert call_segments(arr, 1, None, off, 4, dev) == -1 and "states is NULL" in last_error()
    assert call_segments(arr, 1, states, None, 4, dev) == -1 and "state_offsets is NULL" in last_error()
    assert call_segments(arr, 1, states, off, 4, dev, out=False) == -1
    assert call_segments(arr, 1, states, off, 4, dev, num_out=False) == -1
    assert call_segments(arr, -1, states, off, 4, dev) == -1
    assert call_segments(arr, 1 << 31, states, off, 4, dev) == -1
    assert call_segments(arr, 1, states, off, 0, dev) == -1 and "window_length" in last_error()
    assert call_segments(arr, 1, states, off, -4, dev) == -1
    assert call_segments(arr, 1, states, off, 4, -1) == -1 and "device_id" in last_error()
    assert call_segments(arr, 1, states, (C.c_int64 * 2)(8, 0), 4, dev) == -1
    assert call_segments(arr, 1, states, (C.c_int64 * 2)(0, 17), 4, dev) == -1 and "longer" in last_error()
    for bad in ((0, 0, 9, 8, 0, 8, "+"), (0, 0, 0, 8, 9, 8, "+"), (0, 0, 0, 8, 0, 8, "x")):
        assert call_segments(_overlap_array([bad]), 1, states, off, 4, dev) == -1, bad
    # more than 2^31 records: 2^31 - 1 target bases in windows of 1, three times
    wide = _overlap_array([(0, 0, 0, 0, 0, (1 << 31) - 1, "+")] * 3)
    assert call_segments(wide, 3, states, (C.c_int64 * 4)(0, 0, 0, 0), 1, dev) == -1 and "2^31" in last_error()
    # nothing to do: no device call either
    p, m = C.c_void_p(), C.c_int64(-5)
    assert load_library().gwamd_window_segments(None, 0, None, None, 4, dev, None, C.byref(p), C.byref(m)) == 0
    assert not p.value and m.value == 0


def test_window_segments_resident_refusals():
    L = load_library()
    arr = _overlap_array([pc.overlap_of((0, 8, 0, 8), "+")])
    p, m = C.c_void_p(), C.c_int64()
    fake = C.c_void_p(0)
    assert L.gwamd_window_segments_resident(fake, fake, arr, 1, 4, 1, C.byref(p), C.byref(m)) == -1
    assert "NULL" in last_error() and not p.value
    with pytest.raises(TypeError):
        cudapolish.window_segments_resident([pc.overlap_of((0, 8, 0, 8), "+")], ["ACGT"], ["ACGT"], 4)


def test_host_walk_refusals():
    with pytest.raises(ValueError):
        cudapolish.window_segments_host(pc.overlap_of((0, 8, 0, 8), "+"), [0] * 17, 4)
    with pytest.raises(ValueError):
        cudapolish.window_segments_host(pc.overlap_of((0, 8, 0, 8), "+"), [0] * 8, 0)
    with pytest.raises(ValueError):
        cudapolish.window_segments_host(pc.overlap_of((8, 0, 0, 8), "+"), [0] * 8, 4)


# ---- grouping ---------------------------------------------------------------------------------------


def random_reads(rng, n, lo, hi, alphabet="ACGT"):
    return ["".join(rng.choice(alphabet) for _ in range(rng.randint(lo, hi))) for _ in range(n)]


def segment_array(records):
    return np.array(records, dtype=cudapolish.SEGMENT_DTYPE) if records else np.zeros(0, cudapolish.SEGMENT_DTYPE)


def test_build_windows_equals_model_on_random_overlaps():
    rng = random.Random(77)
    targets = random_reads(rng, 4, 0, 90) + [""]
    targets[2] = "ACGTNACGTN" * 5  # no overlap touches target 2: backbone-only windows
    queries = random_reads(rng, 6, 30, 80, "ACGTN")
    overlaps, paths = [], []
    for _ in range(40):
        t = rng.choice((0, 1, 3))
        q = rng.randrange(len(queries))
        if len(targets[t]) == 0:
            continue
        ts = rng.randint(0, len(targets[t]) - 1)
        te = rng.randint(ts, len(targets[t]))
        qs = rng.randint(0, len(queries[q]) - 1)
        qe = rng.randint(qs, len(queries[q]))
        overlaps.append((q, t, qs, qe, ts, te, rng.choice("+-")))
        paths.append(pc.random_path(rng, te - ts, qe - qs))
    for w in (7, 16, 50):
        records = pm.window_segments(overlaps, paths, w)
        for cap in (100, 3, 1):
            expected, dropped = pm.build_windows(targets, queries, overlaps, records, w, cap)
            got, got_dropped = cudapolish.build_windows(targets, queries, overlaps, segment_array(records), w, cap)
            assert got == expected and got_dropped == dropped, (w, cap)
            backbone_only = [x for x in got if x["target"] == 2]
            assert backbone_only and all(x["overlap"] == [-1] for x in backbone_only)
        assert dropped > 0  # the cap of 1 leaves every kept piece out


def test_build_windows_two_percent_rule():
    # w = 100: (q_end - q_begin) * 50 == w at two bases, one below at one base
    targets, queries = ["A" * 100], ["CG"]
    overlaps = [(0, 0, 0, 2, 0, 100, "+")] * 2
    records = [(0, 0, 0, 2, 0, 2, 0, 0), (1, 0, 0, 1, 0, 1, 0, 0)]
    got, dropped = cudapolish.build_windows(targets, queries, overlaps, segment_array(records), 100)
    assert got == pm.build_windows(targets, queries, overlaps, records, 100)[0]
    assert got[0]["sequences"] == ["A" * 100, "CG"] and got[0]["overlap"] == [-1, 0] and dropped == 0


def test_build_windows_reverse_complements_odd_lengths():
    targets, queries = ["ACGTACGTA"], ["AACGN"]
    overlaps = [(0, 0, 0, 5, 0, 9, "-")]
    records = [(0, 0, 0, 5, 0, 9, pm.REVERSE, 0), (0, 0, 1, 4, 2, 5, pm.REVERSE, 0)]
    got, _ = cudapolish.build_windows(targets, queries, overlaps, segment_array(records), 9)
    # every position is complemented, the middle one too; N stays
    assert got[0]["sequences"] == ["ACGTACGTA", "NCGTT", "CGT"]
    assert got == pm.build_windows(targets, queries, overlaps, records, 9)[0]
    assert got[0]["t_begin"] == [0, 0, 2] and got[0]["t_end"] == [9, 9, 5]


def test_build_windows_skips_flagged_segments_and_checks_the_rest():
    targets, queries = ["ACGTACGT"], ["ACGT"]
    overlaps = [(0, 0, 0, 4, 0, 8, "+")]
    flagged = [(0, 0, 0, 4, 0, 4, f, 0) for f in (pm.EMPTY, pm.EMPTY | pm.BAD_PATH, pm.EMPTY | pm.NOT_ALIGNED)]
    got, _ = cudapolish.build_windows(targets, queries, overlaps, segment_array(flagged), 4)
    assert [x["sequences"] for x in got] == [["ACGT"], ["ACGT"]]
    for bad in ((1, 0, 0, 4, 0, 4, 0, 0), (0, 2, 0, 4, 0, 4, 0, 0), (0, 0, 0, 5, 0, 4, 0, 0), (0, 0, 3, 2, 0, 4, 0, 0)):
        with pytest.raises(ValueError):
            cudapolish.build_windows(targets, queries, overlaps, segment_array([bad]), 4)
    with pytest.raises(ValueError):
        cudapolish.build_windows(targets, queries, overlaps, segment_array([]), 0)
    with pytest.raises(ValueError):
        cudapolish.build_windows(targets, queries, overlaps, segment_array([]), 4, 0)


def test_overlap_struct_matches():
    assert C.sizeof(Overlap) == 36 and cudapolish.SEGMENT_DTYPE.itemsize == 32


def test_cpp_interface_host_part(tmp_path):
    import subprocess
    r = subprocess.run([pc.build_cpp_check(tmp_path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == [word for name in pc.CPP_HOST for word in ("ok", name)]
