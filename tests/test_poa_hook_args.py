"""Argument checks of the POA test hooks (csrc/poa_hooks.hip): every launcher
returns -2 for a bad argument before anything is sized or allocated from it,
so these calls make no device call and run without a GPU.  Each case takes the
valid call of a 4-node chain and spoils one argument."""
import ctypes as C

import numpy as np
import pytest

from claragenomicsanalysis_amd import load_library

N, E, A = 4, 50, 50  # nodes; kMaxEdges and kMaxAlignments slots per node


def _chain():
    g = dict(base=np.frombuffer(b"ACGT", np.uint8).copy(), in_cnt=np.array([0, 1, 1, 1], np.uint16),
             out_cnt=np.array([1, 1, 1, 0], np.uint16), aln_cnt=np.zeros(N, np.uint16), cov=np.ones(N, np.uint16),
             in_w=np.ones((N, E), np.uint16), in_e=np.zeros((N, E), np.int32), out_e=np.zeros((N, E), np.int32),
             aln=np.zeros((N, A), np.int32), order=np.arange(N, dtype=np.int32), hint=np.zeros(N, np.int32),
             sorted=np.zeros(N, np.int32), mpos=np.zeros(N, np.int32))
    for v in range(1, N):
        g["in_e"][v, 0] = v - 1
        g["out_e"][v - 1, 0] = v
    return g


def _call(name, argtypes, args):
    f = getattr(load_library(), name)
    f.restype = C.c_int
    f.argtypes = argtypes
    return f(*[a.ctypes.data if isinstance(a, np.ndarray) else a for a in args])


THREADS = [("threads", 63), ("threads", 65), ("threads", 2048)]
SCRATCH = [("scratch", -1), ("scratch", 163841)]
NODES = [("n", 0), ("n", -1)]


@pytest.mark.parametrize("size_bits", [16, 32])
@pytest.mark.parametrize("bad", NODES + THREADS + SCRATCH + [("n_prev", N + 1), ("n_prev", -1), ("hint", None),
                                                             ("order_prev", None),
                                                             ("order_prev", np.array([0, 1, 1, 3], np.int32)),
                                                             ("order_prev", np.array([0, 1, 2, 4], np.int32))])
@pytest.mark.parametrize("timed", [False, True])
def test_topsort_levels(size_bits, bad, timed):
    g = _chain()
    a = dict(n=N, n_prev=N, n_hint=N, hint=g["hint"], order_prev=g["order"], threads=128, scratch=64 << 10)
    a[bad[0]] = bad[1]
    args = [size_bits, a["n"], a["n_prev"], a["n_hint"], g["in_cnt"], g["in_e"], g["out_cnt"], g["out_e"], a["hint"],
            a["order_prev"], a["threads"], a["scratch"], g["sorted"]]
    types = [C.c_int] * 4 + [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_void_p]
    if timed:
        ms, prof = np.zeros(1, np.float64), np.zeros(10, np.uint64)
        assert _call("gwamd_internal_topsort_levels_timed", types + [C.c_int, C.c_void_p, C.c_void_p],
                     args + [3, ms, prof]) == -2
    else:
        assert _call("gwamd_internal_topsort_levels", types, args) == -2


@pytest.mark.parametrize("bad", [("V", 0), ("V", -1), ("n", N - 1), ("n", 32768), ("L", 0), ("L", 32768)] + THREADS + [
    ("sorted", [0, 1, 1, 3]), ("sorted", [0, 1, 2, 4]), ("kind", [0, 0, 0]),  # new node 4 marked old
    ("kind", [0, 2, 2]),                                                       # old node 2 marked new
    ("curr", [1, 2, 6]), ("curr", [1, -1, 4])])
def test_order_splice(bad):
    # 4 old nodes in id order, 2 new ones; the path: old 1, old 2, new 4
    a = dict(V=N, n=N + 2, L=3, sorted=[0, 1, 2, 3], curr=[1, 2, 4], kind=[0, 0, 2], threads=128)
    a[bad[0]] = bad[1]
    so = np.full(max(a["n"], N), -1, np.int32)
    so[:N] = a["sorted"]
    po = np.full(len(so), -1, np.int32)
    assert _call("gwamd_internal_order_splice", [C.c_int] * 3 + [C.c_void_p] * 4 + [C.c_int],
                 [a["V"], a["n"], a["L"], so, po, np.array(a["curr"], np.int32), np.array(a["kind"], np.uint8),
                  a["threads"]]) == -2


@pytest.mark.parametrize("bad", NODES + [("n", 8193), ("threads", 63), ("threads", 65), ("threads", 1024),
                                         ("threads", 2048), ("xl_cap", 63), ("xl_cap", 68), ("ring_rows", 0),
                                         ("ring_rows", -1), ("xl_cap", 1 << 17),  # more LDS than a workgroup has
                                         ("sorted", np.array([0, 1, 1, 3], np.int32)),
                                         ("sorted", np.array([0, 1, 2, 4], np.int32))])
def test_row_program(bad):
    g = _chain()
    a = dict(n=N, sorted=g["order"], xl_cap=72, ring_rows=64, threads=128)
    a[bad[0]] = bad[1]
    rec, xl = np.zeros((2, N + 2), np.uint32), np.zeros((2, 72 + 72), np.uint16)
    assert _call("gwamd_internal_row_program", [C.c_int] + [C.c_void_p] * 5 + [C.c_int] * 3 + [C.c_void_p] * 2,
                 [a["n"], g["base"], g["in_cnt"], g["out_cnt"], g["in_e"], a["sorted"], a["xl_cap"], a["ring_rows"],
                  a["threads"], rec, xl]) == -2


@pytest.mark.parametrize("size_bits", [16, 32])
@pytest.mark.parametrize("bad", NODES + [("n", 65536)] + SCRATCH + [("scratch", 163840 - 63)])
@pytest.mark.parametrize("reps", [0, 3])
def test_topsort_racon(size_bits, bad, reps):
    g = _chain()
    a = dict(n=N, scratch=64 << 10)
    a[bad[0]] = bad[1]
    ncols, ms = np.zeros(1, np.int32), np.zeros(1, np.float64)
    assert _call("gwamd_internal_topsort_racon",
                 [C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_int, C.c_void_p],
                 [size_bits, a["n"], g["in_cnt"], g["in_e"], g["aln_cnt"], g["aln"], a["scratch"], 0, g["sorted"],
                  g["mpos"], ncols, reps, ms]) == -2


@pytest.mark.parametrize("size_bits", [16, 32])
@pytest.mark.parametrize("bad", NODES + [("n", 32768)] + SCRATCH + [("scratch", 163840 - 63), ("max_cons", 0),
                                                                    ("max_cons", -1)])
def test_consensus(size_bits, bad):
    g = _chain()
    a = dict(n=N, scratch=64 << 10, max_cons=16)
    a[bad[0]] = bad[1]
    st, ln = np.zeros(1, np.int32), np.zeros(1, np.int32)
    cons, cov = np.zeros(16, np.uint8), np.zeros(16, np.uint16)
    assert _call("gwamd_internal_consensus",
                 [C.c_int, C.c_int] + [C.c_void_p] * 11 + [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 4,
                 [size_bits, a["n"], g["base"], g["order"], g["order"], g["in_cnt"], g["in_e"], g["in_w"],
                  g["out_cnt"], g["out_e"], g["aln_cnt"], g["aln"], g["cov"], a["max_cons"], 0, a["scratch"], st, ln,
                  cons, cov]) == -2
