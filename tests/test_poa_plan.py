"""The host's kernel plan, pinned (CPU only): for a grid of batch capacities,
scores and diagnostic switches, gwamd_internal_poa_plan must return exactly the
score/size widths and Dims fields recorded in tests/golden/poa_plan.json, and
must find a kernel for every plan it makes.  The plan decides LDS layouts and
HBM offsets that the kernels index by, so any change to it shows up here first.

`python tests/test_poa_plan.py --record` rewrites the fixture from the built
library (only when the plan is meant to change).
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "poa_plan.json")

DEFAULT = (-8, -6, 8)    # gap, mismatch, match: 16-bit scores up to 1,489 bases
BIG = (-80, -60, 80)     # 32-bit scores at every length
# every max_sequence_size of the tests and of bench.py's configs, and the
# lengths the full-alignment plan branches on
FULL_LENGTHS = [128, 130, 256, 400, 600, 700, 900, 1000, 1100, 1600, 1700, 2200, 4400, 10600,
                512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 8192]
BAND_LENGTHS = [256, 600, 1100, 4400, 10600]
SCORE_SETS = [(-4, -6, 8), (-2, -4, 5), (-8, -9, 8), (-8, -8, 8), (-8, -16, 8), (0, -6, 8), (-8, -6, 0), (-8, 0, 8),
              (-1, -1, 1), (0, 0, 0), (-127, -1, 128), (-127, -6, 128), (-127, -1, 129), (-127, -6, 129),
              (-20, -1, 40), (-15, -20, 45), (-30, -70, 90)]
SHAPES = ["8,1", "16,1", "24,1", "32,1", "8,2", "8,3", "8,4", "16,4", "4,4", "8,8", "16,8"]


def _args(ms, banded=0, bw=256, msa=0, scores=DEFAULT, reads=10, nodes=None, nodes_banded=None):
    up4 = lambda v: (v + 3) // 4 * 4
    return [ms, reads, bw, nodes or up4(3 * ms), nodes_banded or up4(4 * ms), banded, msa] + list(scores)


def grid():
    """[(environment, arguments of gwamd_internal_poa_plan)]"""
    g = []
    for ms in FULL_LENGTHS:
        for sc in (DEFAULT, BIG):
            g.append(({}, _args(ms, scores=sc)))
    g.append(({}, _args(1100, msa=1, reads=32)))
    g.append(({}, _args(130, nodes=140, bw=128, reads=8)))
    for ms in BAND_LENGTHS:
        for bw in list(range(128, 1025, 128)) + [1152]:
            for sc in (DEFAULT, BIG):
                g.append(({}, _args(ms, banded=1, bw=bw, scores=sc)))
        g.append(({}, _args(ms, banded=1, scores=(2, -6, 8))))  # a positive gap: v1
        g.append(({}, _args(ms, banded=1, msa=1, reads=16)))
    d = {"GWAMD_DIAG": "1"}
    for shape in SHAPES + ["5,5"]:
        g.append((dict(d, GWAMD_POA_LDS_SHAPE=shape), _args(1100)))
        g.append((dict(d, GWAMD_POA_LDS_SHAPE=shape), _args(2200, scores=BIG)))
    some = [_args(1100), _args(2200, scores=BIG), _args(1100, banded=1), _args(1700, banded=1, bw=128),
            _args(10600, banded=1, bw=512, scores=BIG), _args(600, msa=1), _args(4400, banded=1, bw=1024)]
    switches = [("GWAMD_POA_KERNEL", ["v1"]), ("GWAMD_POA_LDS_PAD", ["20000"]), ("GWAMD_BAND_FWD", ["ad", "row"]),
                ("GWAMD_BAND_AD_WAVES", ["2"]),
                ("GWAMD_TB_WALK", ["rank", "scalar", "rect", "scalar_rect", "strip32", "scalar_strip32"]),
                ("GWAMD_TB_ABOVE", ["0", "6"]), ("GWAMD_TOPSORT_RING", ["1"]), ("GWAMD_POA_FWD", ["v1"]),
                ("GWAMD_TOPSORT", ["fifo"]), ("GWAMD_RACON", ["v1"]), ("GWAMD_CONSENSUS", ["hbm"]),
                ("GWAMD_CONSENSUS_LDS_BYTES", ["4096"]), ("GWAMD_POA_ADD", ["wave0", "serial"])]
    for name, values in switches:
        for v in values:
            for a in some:
                g.append((dict(d, **{name: v}), a))
    # the score sets of tests/test_poa_scores.py: widths by the reference's rule, and no
    # packed 16-bit rows where the E domain does not fit ((-20, -1, 40) and (-15, -20, 45) at 600,
    # (-127, -1, 129) at 128: lds_kernel 0)
    for sc in SCORE_SETS:
        for ms in (128, 400, 600):
            g.append(({}, _args(ms, scores=sc)))
            g.append(({}, _args(ms, banded=1, bw=128 if ms == 128 else 256, scores=sc)))
    # forced anti-diagonal pass with fewer waves, and the switches without GWAMD_DIAG=1: ignored
    g.append((dict(d, GWAMD_BAND_FWD="ad", GWAMD_BAND_AD_WAVES="2"), _args(1100, banded=1)))
    g.append(({"GWAMD_DIAG": "0", "GWAMD_POA_KERNEL": "v1", "GWAMD_TB_WALK": "scalar", "GWAMD_POA_ADD": "serial"},
              _args(1100)))
    return g


ENV_NAMES = sorted({k for env, _ in grid() for k in env})


def _lib():
    sys.path.insert(0, ROOT)
    from claragenomicsanalysis_amd import load_library
    L = load_library()
    L.gwamd_internal_poa_plan_fields.restype = C.c_char_p
    L.gwamd_internal_poa_plan.restype = C.c_int32
    L.gwamd_internal_poa_plan.argtypes = [C.c_int32] * 10 + [C.POINTER(C.c_int64), C.c_int32]
    L.gwamd_last_error.restype = C.c_char_p
    return L


def plan(L, env, args):
    """{field: value} of the plan under `env`, or {"error": message}."""
    for k in ENV_NAMES:
        os.environ.pop(k, None)
    os.environ.update(env)
    names = L.gwamd_internal_poa_plan_fields().decode().split(",")
    out = (C.c_int64 * len(names))()
    n = L.gwamd_internal_poa_plan(*args, out, len(names))
    if n < 0:
        return {"error": L.gwamd_last_error().decode()}
    assert n == len(names)
    return dict(zip(names, out))


def test_plan_matches_fixture(monkeypatch):
    for k in ENV_NAMES:  # (restored after the test)
        monkeypatch.setenv(k, "")
    L = _lib()
    fx = json.load(open(GOLDEN))
    assert [(c["env"], c["args"]) for c in fx["cases"]] == [(e, a) for e, a in grid()]
    bad = []
    for c in fx["cases"]:
        got = plan(L, c["env"], c["args"])
        found = got.pop("kernel", 1)  # the resolver's answer is not part of the recorded plan
        want = {"error": c["error"]} if "error" in c else dict(zip(fx["fields"], c["plan"]))
        if got != want:
            bad.append((c["env"], c["args"], {k: (got.get(k), want.get(k)) for k in set(got) | set(want)
                                             if got.get(k) != want.get(k)}))
        elif "error" not in c and found != 1:
            bad.append((c["env"], c["args"], "no kernel for this plan"))
    assert not bad, bad[:5]


def test_unsupported_shape_is_refused(monkeypatch):
    for k in ENV_NAMES:
        monkeypatch.setenv(k, "")
    got = plan(_lib(), {"GWAMD_DIAG": "1", "GWAMD_POA_LDS_SHAPE": "5,5"}, _args(1100))
    assert got == {"error": "GWAMD_POA_LDS_SHAPE: unsupported columns/waves pair"}


if __name__ == "__main__" and sys.argv[1:] == ["--record"]:
    L = _lib()
    fields = [f for f in L.gwamd_internal_poa_plan_fields().decode().split(",") if f != "kernel"]
    cases = []
    for env, args in grid():
        p = plan(L, env, args)
        rec = {"env": env, "args": args}
        if "error" in p:
            rec["error"] = p["error"]
        else:
            rec["plan"] = [p[f] for f in fields]
        cases.append(rec)
    with open(GOLDEN, "w") as f:
        f.write('{"fields": %s,\n "cases": [\n' % json.dumps(fields))
        f.write(",\n".join("  " + json.dumps(c) for c in cases))
        f.write("\n ]}\n")
    print("recorded %d cases" % len(cases))
