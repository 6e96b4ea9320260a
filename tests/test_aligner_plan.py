"""The aligner host's plan, pinned (CPU only): for a grid of capacities, device
facts, diagnostic switches and launches, gwamd_internal_aligner_plan must
return exactly the layout, slot count, pipeline stages and launch decisions
recorded in tests/golden/aligner_plan.json, and must find a kernel for every
plan it makes.  The plan decides LDS offsets and workspace-slot offsets that
the kernels index by, so any change to it shows up here first.

`python tests/test_aligner_plan.py --record` rewrites the fixture from the
built library (only when the plan is meant to change).
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "aligner_plan.json")

HM, MYERS, BANDED, UKKONEN = range(4)
ALGOS = [HM, MYERS, BANDED, UKKONEN]
# every (max_query_length, max_target_length) of the tests and of bench.py's configs
SHAPES = [(300, 330), (1000, 1000), (5000, 5000), (12000, 12000), (16000, 16000), (16384, 16384), (40000, 40000),
          (65536, 65536), (100000, 100000)]
MAX_N = [1, 32, 4000, 100000]
GB = 10 ** 9
LIMITS = {HM: (1 << 24, 1 << 24), MYERS: (1 << 24, 1 << 24), BANDED: (65536, 65536), UKKONEN: (65536, 65536)}
D = {"GWAMD_DIAG": "1"}


def _args(algo, q, t, n, per_cu=8, wide=1, free=250 * GB, cus=256, count=0, nslots=0, mq=0, diff=0):
    """count, nslots, mq of 0: max_alignments, the planned slots, max_query_length"""
    return [algo, q, t, n, cus, per_cu, wide, free, count, nslots, mq, diff]


def grid():
    """[(environment, arguments of gwamd_internal_aligner_plan)]"""
    g = []
    for algo in ALGOS:
        for q, t in SHAPES:
            for n in MAX_N:
                g.append(({}, _args(algo, q, t, n)))
    # occupancies, a wide Ukkonen kernel that is resident more often than the narrow one, little free memory
    for algo in ALGOS:
        for q, t in [(300, 330), (5000, 5000), (16000, 16000), (65536, 65536)]:
            for per_cu in (1, 5, 13):
                g.append(({}, _args(algo, q, t, 4000, per_cu=per_cu)))
    g.append(({}, _args(UKKONEN, 16000, 16000, 4000, per_cu=1, wide=2)))
    for algo in (BANDED, UKKONEN):  # the 3/4-of-free cap bites on 32 pairs of 65,536 bases
        for free in (250 * GB, 40 * GB):
            g.append(({}, _args(algo, 65536, 65536, 32, per_cu=1, free=free)))
    # branch points: Hirschberg-Myers short / long, target codes in HBM, banded waves, Ukkonen tile
    # classes and narrow / wide (band rows cross 512 at a target of 8,240)
    for algo in (HM, MYERS):
        for q, t in [(16384, 1000), (16385, 1000), (1000, 65535), (1000, 65536), (1000, 131072), (1000, 131073)]:
            g.append(({}, _args(algo, q, t, 32)))
    for s in (8192, 8193):
        g.append(({}, _args(BANDED, s, s, 32)))
    for s in (8192, 8193, 32767, 32768, 8239, 8240):
        g.append(({}, _args(UKKONEN, s, s, 32)))
    # the length limits and one past each, the Ukkonen band bound, the full-Myers slot bound
    for algo in ALGOS:
        lq, lt = LIMITS[algo]
        for q, t in [(lq, 1000), (lq + 1, 1000), (1000, lt), (1000, lt + 1)]:
            g.append(({}, _args(algo, q, t, 1)))
    g.append(({}, _args(UKKONEN, 1000, 100000, 1)))
    g.append(({}, _args(MYERS, 300000, 300000, 1)))
    g.append(({}, _args(MYERS, 310000, 310000, 1)))
    # a banded aligner's LDS image past 160 KiB
    g.append((dict(D, GWAMD_UK_TILE_BYTES="65536"), _args(UKKONEN, 65536, 65536, 1)))
    # each switch at the values the tests use and one bad value
    some = {HM: [_args(HM, 300, 330, 64), _args(HM, 5000, 5000, 4000), _args(HM, 40000, 40000, 4)],
            BANDED: [_args(BANDED, 300, 330, 64), _args(BANDED, 12000, 12000, 6), _args(BANDED, 65536, 65536, 32)],
            UKKONEN: [_args(UKKONEN, 5000, 5000, 4000), _args(UKKONEN, 40000, 40000, 5)]}
    every = [_args(a, 5000, 5000, 4000) for a in ALGOS] + [_args(a, 300, 330, 2) for a in ALGOS]
    switches = [("GWAMD_HM_STRIPE_BLOCKS", ["1", "2", "4", "0", "5"], some[HM] + [_args(MYERS, 300, 330, 64)]),
                ("GWAMD_BAND_TILE_BYTES", ["4096", "2048", "49152", "4k", "1024", "4100"], some[BANDED]),
                ("GWAMD_BAND_WAVES", ["1", "4", "8", "16", "2"], some[BANDED]),
                ("GWAMD_BAND_SPEC", ["0", "1", "2", "3", "8", "9"], some[BANDED]),
                ("GWAMD_UK_TILE_BYTES", ["16384", "24576", "1024", "512", "70000"], some[UKKONEN]),
                ("GWAMD_ALIGNER_GRID", ["1", "32", "0", "33"], every),
                ("GWAMD_ALIGNER_PIPELINE", ["0", "1", "3", "4", "8", "9"], every)]
    for name, values, cases in switches:
        for v in values:
            for a in cases:
                g.append((dict(D, **{name: v}), a))
    # a switch of one algorithm does not refuse another's aligner
    bad = dict(D, GWAMD_BAND_TILE_BYTES="4k", GWAMD_BAND_WAVES="2", GWAMD_BAND_SPEC="9", GWAMD_UK_TILE_BYTES="1")
    g.append((bad, _args(HM, 5000, 5000, 4000)))
    g.append((bad, _args(MYERS, 5000, 5000, 4000)))
    # the pipelined tests' settings together, and the run-ahead tests'
    g.append((dict(D, GWAMD_ALIGNER_GRID="1", GWAMD_ALIGNER_PIPELINE="4"), _args(MYERS, 1200, 1200, 1500)))
    for spec in ("0", "3", "8"):
        for waves in ("4", "8"):
            g.append((dict(D, GWAMD_BAND_SPEC=spec, GWAMD_BAND_WAVES=waves), _args(BANDED, 12000, 12000, 6)))
    # without GWAMD_DIAG=1 every switch is ignored
    off = {"GWAMD_DIAG": "0", "GWAMD_HM_STRIPE_BLOCKS": "1", "GWAMD_BAND_TILE_BYTES": "4k", "GWAMD_BAND_WAVES": "2",
           "GWAMD_BAND_SPEC": "9", "GWAMD_UK_TILE_BYTES": "1", "GWAMD_ALIGNER_GRID": "99",
           "GWAMD_ALIGNER_PIPELINE": "9"}
    for algo in ALGOS:
        g.append((off, _args(algo, 12000, 12000, 4000)))
    # launches.  Banded Myers planned for long queries: all-short queries take one wave per pair
    # (not when the waves are forced)
    for mq in (8192, 8193, 300):
        g.append(({}, _args(BANDED, 12000, 12000, 4000, count=100, mq=mq)))
        g.append((dict(D, GWAMD_BAND_WAVES="8"), _args(BANDED, 12000, 12000, 4000, count=100, mq=mq)))
    # Ukkonen: the batch's widest band just within and past the one-wave kernel, and past 1,024 rows
    for q, n in [(16000, 4000), (65536, 32)]:
        for diff in (0, 823, 824, 825, 1847, 1848, 6553):
            g.append(({}, _args(UKKONEN, q, q, n, diff=diff)))
    # the run-ahead: count against the slots of the launch, what is resident (8 x 256 = 2,048
    # workgroups, 5 sweeps by default) and half the CUs (128)
    for count, nslots in [(1, 1), (32, 32), (32, 31), (33, 32), (128, 128), (129, 129), (128, 64), (2, 2048)]:
        g.append(({}, _args(BANDED, 65536, 65536, 4000, count=count, nslots=nslots)))
    for count in (128, 51, 52):  # 5 x 52 > 256 resident at one workgroup per CU
        g.append(({}, _args(BANDED, 12000, 12000, 4000, per_cu=1, count=count, nslots=256)))
    for spec in ("0", "8"):
        for count in (32, 33):  # 8 x 33 > 256
            g.append((dict(D, GWAMD_BAND_SPEC=spec),
                      _args(BANDED, 12000, 12000, 4000, per_cu=1, count=count, nslots=256)))
        g.append((dict(D, GWAMD_BAND_SPEC=spec), _args(BANDED, 300, 330, 64, count=6)))  # on the one-wave plan
    # the chunk state of a 65,536-base band does not fit a forced 4 KiB tile: no run-ahead
    g.append((dict(D, GWAMD_BAND_TILE_BYTES="4096"), _args(BANDED, 65536, 65536, 32, count=32, nslots=32)))
    return g


ENV_NAMES = sorted({k for env, _ in grid() for k in env})


def _lib():
    sys.path.insert(0, ROOT)
    from claragenomicsanalysis_amd import load_library
    L = load_library()
    L.gwamd_internal_aligner_plan_fields.restype = C.c_char_p
    L.gwamd_internal_aligner_plan.restype = C.c_int32
    L.gwamd_internal_aligner_plan.argtypes = ([C.c_int32] * 7 + [C.c_int64] + [C.c_int32] * 4 +
                                              [C.POINTER(C.c_int64), C.c_int32])
    L.gwamd_last_error.restype = C.c_char_p
    return L


def plan(L, env, args):
    """{field: value} of the plan under `env`, or {"error": message}."""
    for k in ENV_NAMES:
        os.environ.pop(k, None)
    os.environ.update(env)
    names = L.gwamd_internal_aligner_plan_fields().decode().split(",")
    out = (C.c_int64 * len(names))()
    n = L.gwamd_internal_aligner_plan(*args, out, len(names))
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
    assert not bad, (len(bad), bad[:5])


def test_limits_have_one_statement(monkeypatch):
    # gwamd_aligner_pair_fits and the planner refuse the same capacities
    for k in ENV_NAMES:
        monkeypatch.setenv(k, "")
    L = _lib()
    for env, a in grid():
        if env:
            continue
        refused = "error" in plan(L, {}, a)
        assert bool(L.gwamd_aligner_pair_fits(a[0], a[1], a[2])) == (not refused), a


if __name__ == "__main__" and sys.argv[1:] == ["--record"]:
    L = _lib()
    fields = [f for f in L.gwamd_internal_aligner_plan_fields().decode().split(",") if f != "kernel"]
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
