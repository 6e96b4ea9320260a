"""The POA host's capacity, device layout and window order, pinned (CPU only).

For a grid of batch capacities, device memory and device facts,
gwamd_internal_poa_capacity must return exactly the window capacity, slots,
resident grid, score budget, byte counts and the offset of every device array
recorded in tests/golden/poa_capacity.json; gwamd_internal_poa_window_order
must return the recorded queue orders.  The fixture was recorded from the batch
class as it stood before these numbers moved into poa_plan.cpp (its constructor
and upload() run over stand-in HIP entry points), so it pins that the move
changed none of them.  A null in the fixture is a value that run could not
observe (the order and dequeue-head offsets of a batch too small to be
reordered) and is not compared.

`python tests/test_poa_capacity.py --record` rewrites the fixture from the
built library (only when these numbers are meant to change).
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_poa_plan import BIG, _args  # noqa: E402  (the same capacities as the kernel plan's grid)

GOLDEN = os.path.join(ROOT, "tests", "golden", "poa_capacity.json")

D = {"GWAMD_DIAG": "1"}
V1 = dict(D, GWAMD_POA_KERNEL="v1")
SLOTS3 = dict(D, GWAMD_POA_SLOTS="3")
# (environment, arguments of gwamd_internal_poa_plan, the reference's bytes per
# window: below that much memory the constructor refuses the batch)
BATCHES = [
    ({}, _args(256, reads=8), 411952),                                   # full, 16-bit scores
    ({}, _args(1100), 1774352),
    ({}, _args(600, reads=32), 994296),
    ({}, _args(1600), 2580852),                                          # full, 32-bit scores
    ({}, _args(2200, scores=BIG), 3548652),
    ({}, _args(10600), 17097852),
    ({}, _args(1100, banded=1, bw=256), 2356252),                        # banded, two widths and more
    ({}, _args(1700, banded=1, bw=128), 3641452),
    ({}, _args(4400, banded=1, bw=1024), 9424852),
    ({}, _args(10600, banded=1, bw=512, scores=BIG), 35934072),
    ({}, _args(1100, msa=1, reads=32), 12765660),                        # MSA
    ({}, _args(1100, banded=1, msa=1, reads=16), 9862696),
    (V1, _args(1100), 1774352),                                          # the global-memory kernel
    (V1, _args(1100, banded=1), 2356252),
    (SLOTS3, _args(1100), 1774352),                                      # a forced small grid
    (SLOTS3, _args(1100, banded=1), 2356252),
    (SLOTS3, _args(1600), 2580852),
]
FACTS = [(256, 4), (256, 1), (2, 2), (256, 0)]  # CUs, resident workgroups per CU (0: no occupancy answer)


def grid():
    """[(environment, arguments of gwamd_internal_poa_capacity)]"""
    g = []
    for env, args, min_mem in BATCHES:
        for mem in (min_mem - 1, 256 << 20, 2 << 30, 64 << 30):
            for cus, per_cu in FACTS:
                g.append((env, args + [mem, cus, per_cu]))
    return g


def order_grid():
    """[{lens: read lengths per window, cus, slots, persistent}]"""
    def wins(n, seed=1):  # n windows of 1-4 reads, lengths from a small LCG: distinct costs and some equal ones
        out, x = [], seed
        for _ in range(n):
            x = (x * 1103515245 + 12345) % (1 << 31)
            out.append([50 + (x >> (8 + 3 * r)) % 40 * 10 for r in range(1 + x % 4)])
        return out
    g = []
    for cus in (1, 2, 3, 256):
        # below, at and above the CU count; the last round partial, in odd and even rounds
        for n in (cus - 1, cus, cus + 1, 2 * cus + 1, 4 * cus - 1) if cus > 3 else range(0, 4 * cus + 2):
            if n >= 0:
                g.append({"lens": wins(n, cus), "cus": cus, "slots": 1 << 20, "persistent": 0})
    for cus, slots, n in [(2, 3, 8), (3, 5, 9), (2, 4, 4), (2, 4, 5), (256, 3, 7), (4, 6, 20), (1, 1, 3), (0, 2, 5),
                          (0, 8, 5)]:
        g.append({"lens": wins(n, 7 + n), "cus": cus, "slots": slots, "persistent": 1})  # more windows than slots
        g.append({"lens": wins(n, 7 + n), "cus": cus, "slots": slots, "persistent": 0})  # ... on the v1 kernel
    same = [[100, 200, 300]] * 7  # equal costs: ties go by window
    odd = [[300, 300], [70], [], [300, 300], [9], [], [120, 40, 40], [300, 300]]  # one-read and empty windows
    for lens in (same, odd, same[:3] + odd):
        g.append({"lens": lens, "cus": 2, "slots": 1 << 20, "persistent": 0})
        g.append({"lens": lens, "cus": 3, "slots": 4, "persistent": 1})
    return g


ENV_NAMES = sorted({k for env, _, _ in BATCHES for k in env})


def _lib():
    sys.path.insert(0, ROOT)
    from claragenomicsanalysis_amd import load_library
    L = load_library()
    L.gwamd_internal_poa_capacity_fields.restype = C.c_char_p
    L.gwamd_internal_poa_capacity.restype = C.c_int32
    L.gwamd_internal_poa_capacity.argtypes = ([C.c_int32] * 10 + [C.c_int64, C.c_int32, C.c_int32] +
                                              [C.POINTER(C.c_int64), C.c_int32])
    L.gwamd_internal_poa_window_order.restype = C.c_int32
    L.gwamd_internal_poa_window_order.argtypes = ([C.POINTER(C.c_int32)] * 2 + [C.c_int32] * 4 +
                                                  [C.POINTER(C.c_int32)])
    L.gwamd_last_error.restype = C.c_char_p
    return L


def capacity(L, env, args):
    """{field: value} of the capacity and layout under `env`, or {"error": message}."""
    for k in ENV_NAMES:
        os.environ.pop(k, None)
    os.environ.update(env)
    names = L.gwamd_internal_poa_capacity_fields().decode().split(",")
    out = (C.c_int64 * len(names))()
    n = L.gwamd_internal_poa_capacity(*args, out, len(names))
    if n < 0:
        return {"error": L.gwamd_last_error().decode()}
    assert n == len(names)
    return dict(zip(names, out))


def window_order(L, case):
    """(kind, order) of gwamd_internal_poa_window_order: 0 no order, 1 an order, 2 an order and a dequeue head."""
    lens = case["lens"]
    flat = [l for w in lens for l in w]
    first = [sum(len(w) for w in lens[:i]) for i in range(len(lens))]
    windows = [v for f, w in zip(first, lens) for v in (f, len(w))]
    order = (C.c_int32 * max(1, len(lens)))()
    kind = L.gwamd_internal_poa_window_order((C.c_int32 * max(1, len(windows)))(*windows),
                                             (C.c_int32 * max(1, len(flat)))(*flat), len(lens), case["cus"],
                                             case["slots"], case["persistent"], order)
    assert kind >= 0, L.gwamd_last_error().decode()
    return kind, (list(order)[:len(lens)] if kind else [])


def test_capacity_matches_fixture(monkeypatch):
    for k in ENV_NAMES:  # (restored after the test)
        monkeypatch.setenv(k, "")
    L = _lib()
    fx = json.load(open(GOLDEN))
    assert [(c["env"], c["args"]) for c in fx["cases"]] == [(e, a) for e, a in grid()]
    assert L.gwamd_internal_poa_capacity_fields().decode().split(",") == fx["fields"]
    bad = []
    for c in fx["cases"]:
        got = capacity(L, c["env"], c["args"])
        want = {"error": c["error"]} if "error" in c else dict(zip(fx["fields"], c["plan"]))
        diff = {k: (got.get(k), want.get(k)) for k in set(got) | set(want)
                if want.get(k, 0) is not None and got.get(k) != want.get(k)}
        if diff:
            bad.append((c["env"], c["args"], diff))
    assert not bad, bad[:5]


def test_layout_is_consistent(monkeypatch):
    # what the fixture cannot say by itself: the arrays lie in the slab in list
    # order without overlap, the scores are 256-B aligned, the order array and
    # the dequeue head fit the window buffer, and device_bytes is the sum
    for k in ENV_NAMES:
        monkeypatch.setenv(k, "")
    L = _lib()
    names = L.gwamd_internal_poa_capacity_fields().decode().split(",")
    arrays = names[names.index("slot_bytes") + 1:names.index("scores")]
    for env, args in grid():
        p = capacity(L, env, args)
        if "error" in p:
            continue
        offs = [p[a] for a in arrays if p[a] >= 0]
        assert offs == sorted(offs) and len(set(offs)) == len(offs) and offs[0] == 0, (env, args)
        assert all(o % 8 == 0 for o in offs) and offs[-1] < p["scores"] <= p["slab_bytes"], (env, args)
        assert p["scores"] % 256 == 0
        P = p["max_poas"]
        assert 8 * P <= p["order_off"] and p["order_off"] + 4 * P <= p["head_off"], (env, args)
        assert p["head_off"] + 4 <= p["win_bytes"] and p["order_off"] % 16 == 0 and p["head_off"] % 16 == 0
        assert p["device_bytes"] == sum(p[k] for k in names if k.endswith("_bytes") and k not in
                                        ("window_bytes", "slot_bytes", "device_bytes"))
        assert 1 <= p["slots"] <= P and (p["resident"] == 0 or p["slots"] == min(p["resident"], P))


def test_window_order_matches_fixture():
    L = _lib()
    fx = json.load(open(GOLDEN))
    assert len(fx["orders"]) == len(order_grid())  # (in order_grid()'s order)
    bad = []
    for case, c in zip(order_grid(), fx["orders"]):
        kind, order = window_order(L, case)
        if (kind, order) != (c["kind"], c["order"]):
            bad.append((case, kind, order, c["kind"], c["order"]))
        assert not kind or sorted(order) == list(range(len(case["lens"])))  # a permutation of the windows
    assert not bad, bad[:3]
    assert {c["kind"] for c in fx["orders"]} == {0, 1, 2}


def write_fixture(fields, cases, orders):
    with open(GOLDEN, "w") as f:
        f.write('{"fields": %s,\n "cases": [\n' % json.dumps(fields))
        f.write(",\n".join("  " + json.dumps(c, separators=(",", ":")) for c in cases))
        f.write('\n ],\n "orders": [\n')
        f.write(",\n".join("  " + json.dumps(c, separators=(",", ":")) for c in orders))
        f.write("\n ]}\n")


if __name__ == "__main__" and sys.argv[1:] == ["--record"]:
    L = _lib()
    fields = L.gwamd_internal_poa_capacity_fields().decode().split(",")
    cases = []
    for env, args in grid():
        p = capacity(L, env, args)
        rec = {"env": env, "args": args}
        if "error" in p:
            rec["error"] = p["error"]
        else:
            rec["plan"] = [p[f] for f in fields]
        cases.append(rec)
    orders = []
    for case in order_grid():
        kind, order = window_order(L, case)
        orders.append({"kind": kind, "order": order})
    write_fixture(fields, cases, orders)
    print("recorded %d capacities, %d orders" % (len(cases), len(orders)))
