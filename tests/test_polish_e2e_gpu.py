"""cudapolish.polish() against the model and the oracle (polish_e2e_cases.expected)
on polish_e2e_cases.hard_input(): banded and full POA, other scores, band widths
and caps than the defaults, the defaults themselves, on every route polish() has
(host windows, resident windows, device grouping, CIGARs in both conventions),
with qualities, trimming, rounds, more than one target, targets without
overlaps, an empty target, windows that keep their backbone by rule between
windows that go to the POA, and a window whose POA runs out of nodes.

Everything polish() returns is compared by exact equality; that the reference
meets the conditions that make this worth something is asserted without a GPU in
test_polish_e2e_cpu.py.
"""
import contextlib

import numpy as np
import pytest

import polish_cigar_cases as cc
import polish_e2e_cases as ec
from claragenomicsanalysis_amd import cudamapper
from claragenomicsanalysis_amd.cudamapper import DeviceReads
from claragenomicsanalysis_amd.cudapoa import CudaPoaBatch

pytestmark = pytest.mark.gpu

MEM = 256 << 20  # for the POA batch: its host staging is sized by it, and the default is half the device

# name: (w, banded, band_width, scores, cap); None: the argument is left to polish()'s default
CONFIGS = {
    "w200-full": (200, False, 256, None, 100),
    "w200-band128-cap6": (200, True, 128, None, 6),
    "w200-band256-scores": (200, True, 256, (4, -4, -6), 100),
    "defaults": (500, None, None, None, None),
    # backbone and four junk reads: more nodes than full mode's 768 and fewer than banded mode's 1,024, so
    # window 1 succeeds only if the banded flag reaches the batch
    "w200-band128-cap5": (200, True, 128, None, 5),
    # window 3 (w = 500) has another consensus at a band of 128 than at 256 (and than in full mode)
    "w500-band128": (500, True, 128, None, 100),
}
ROUTES = ["default", "device_windows", "device_grouping", "cigars", "sam_cigars_device_grouping"]
RESIDENT = {"default": False, "device_windows": True, "device_grouping": True, "cigars": False,
            "sam_cigars_device_grouping": True}


@pytest.fixture(scope="module")
def cudapolish():
    from claragenomicsanalysis_amd import cudapolish
    return cudapolish


@pytest.fixture(scope="module")
def inputs():
    return {w: ec.hard_input(w) for w in (200, 500)}


@pytest.fixture(scope="module")
def cigars(cudapolish, inputs):
    """Per w: the aligner's CIGARs of the overlaps, and the same as ops in SAM's convention."""
    out = {}
    for w, (_, targets, queries, overlaps, _, _) in inputs.items():
        text = cudamapper.align_overlaps(overlaps, queries, targets)
        out[w] = text, [cudapolish.cigar_ops(cc.to_sam(c, o[6])) for o, c in zip(overlaps, text)]
    return out


def reference_kwargs(config):
    w, banded, band_width, scores, cap = CONFIGS[config]
    return w, dict(banded=True if banded is None else banded, band_width=band_width or 256,
                   scores=scores or ec.DEFAULT_SCORES, cap=cap or 100)


def polish_kwargs(config):
    """polish()'s arguments for a configuration; what it leaves to the defaults is not passed."""
    w, banded, band_width, scores, cap = CONFIGS[config]
    given = dict(window_length=None if config == "defaults" else w, banded=banded, band_width=band_width,
                 scores=scores, max_sequences_per_window=cap)
    return {k: v for k, v in given.items() if v is not None}


@pytest.fixture(scope="module")
def references(inputs):
    """expected() per (configuration, qualities, threshold, trim), computed once."""
    cache = {}

    def get(config, qualities=False, threshold=10.0, trim=False):
        key = (config, qualities, threshold, trim)
        if key not in cache:
            w, kwargs = reference_kwargs(config)
            cache[key] = ec.expected(inputs[w], w, qualities=qualities, threshold=threshold, trim=trim, **kwargs)
        return cache[key]
    return get


@contextlib.contextmanager
def no_aligner(cudapolish):
    """polish(cigars=) must not align the overlaps again."""
    def refuse(*args, **kw):
        raise AssertionError("polish(cigars=) aligned the overlaps again")
    kept = cudapolish.window_segments_resident
    cudapolish.window_segments_resident = refuse
    try:
        yield
    finally:
        cudapolish.window_segments_resident = kept


def run(cudapolish, inp, route, cigars=None, **kwargs):
    _, targets, queries, overlaps, _, _ = inp
    kwargs = dict(kwargs, return_windows=True, max_gpu_mem=kwargs.get("max_gpu_mem", MEM))
    if route == "default":
        return cudapolish.polish(targets, queries, overlaps, **kwargs)
    if route == "device_windows":
        return cudapolish.polish(targets, queries, overlaps, device_windows=True, **kwargs)
    if route == "device_grouping":
        return cudapolish.polish(targets, queries, overlaps, device_grouping=True, **kwargs)
    with no_aligner(cudapolish):
        if route == "cigars":
            return cudapolish.polish(targets, queries, overlaps, cigars=cigars[0], **kwargs)
        assert route == "sam_cigars_device_grouping"
        return cudapolish.polish(targets, queries, overlaps, cigars=cigars[1], cigar_convention="sam",
                                 device_grouping=True, **kwargs)


def assert_equals_reference(got, want, resident):
    polished, stats, windows, consensus, status = got
    assert status == want["status"]
    assert consensus == want["consensus"]
    assert stats == want["stats"]
    assert polished == want["polished"]
    assert windows == (want["slice_windows"] if resident else want["windows"])


@pytest.fixture(scope="module")
def results():
    """What polish() returned per (configuration, route), for the comparison of the routes."""
    return {}


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("config", list(CONFIGS))
def test_every_route_equals_the_reference(cudapolish, inputs, cigars, references, results, config, route):
    w = CONFIGS[config][0]
    got = run(cudapolish, inputs[w], route, cigars[w], **polish_kwargs(config))
    results[config, route] = got
    want = references(config)
    assert_equals_reference(got, want, RESIDENT[route])
    # what the comparison rests on (test_polish_e2e_cpu.py): backbones by rule after POA windows, and
    # a window that fails, except where the configuration is there to let it succeed
    assert want["stats"]["backbone_by_rule"] > 0
    assert (want["status"][1] == 0) == (config == "w200-band128-cap5")
    assert want["status"][1] in (0, ec.NODE_LIMIT_STATUS)


@pytest.mark.parametrize("config", list(CONFIGS))
def test_routes_equal_each_other(cudapolish, inputs, cigars, results, config):
    w = CONFIGS[config][0]
    for route in ROUTES:
        if (config, route) not in results:
            results[config, route] = run(cudapolish, inputs[w], route, cigars[w], **polish_kwargs(config))
    first = results[config, ROUTES[0]]
    for route in ROUTES[1:]:
        got = results[config, route]
        assert (got[0], got[1], got[3], got[4]) == (first[0], first[1], first[3], first[4]), route
        for a, b in zip(got[2], first[2]):  # the windows: the keys both routes give
            assert {k: a[k] for k in a if k in b} == {k: b[k] for k in b if k in a}, route
        assert len(got[2]) == len(first[2])
    resident = [results[config, r][2] for r in ROUTES if RESIDENT[r]]
    assert all(x == resident[0] for x in resident[1:])


@pytest.mark.parametrize("route", ["device_windows", "device_grouping"])
@pytest.mark.parametrize("threshold", [10.0, 0.0])
@pytest.mark.parametrize("config", ["w200-band128-cap6", "defaults"])
def test_qualities_and_threshold(cudapolish, inputs, references, config, threshold, route):
    w = CONFIGS[config][0]
    inp = inputs[w]
    got = run(cudapolish, inp, route, query_qualities=inp[4], target_qualities=inp[5], quality_threshold=threshold,
              **polish_kwargs(config))
    want = references(config, qualities=True, threshold=threshold)
    assert_equals_reference(got, want, True)
    assert want["stats"]["dropped_by_quality"] == (ec.JUNK_READS if threshold else 0)
    assert want["status"][1] == (0 if threshold else ec.NODE_LIMIT_STATUS)


@pytest.mark.parametrize("qualities", [True, False])
@pytest.mark.parametrize("route", ["device_windows", "device_grouping"])
def test_trim(cudapolish, inputs, references, route, qualities):
    config = "w200-band256-scores"
    inp = inputs[200]
    more = dict(query_qualities=inp[4], target_qualities=inp[5]) if qualities else {}
    got = run(cudapolish, inp, route, trim=True, **more, **polish_kwargs(config))
    want = references(config, qualities=qualities, trim=True)
    assert want["stats"]["trimmed_bases"] > 0
    assert_equals_reference(got, want, True)


# ---- rounds ---------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def partial_budget(cudapolish, inputs, references):
    """(max_gpu_mem, windows it holds): a budget that holds some of the POA windows of "w200-full" in
    one batch and not all of them, found as test_polish_group_e2e_gpu.py finds its own."""
    _, targets, queries, overlaps, _, _ = inputs[200]
    size = references("w200-full")["stats"]["max_sequence_size"]
    with DeviceReads(queries) as q, DeviceReads(targets) as t:
        ws = cudapolish.window_slices_resident(overlaps, q, t, 200)
        first = np.concatenate([[0], np.cumsum(ws.counts)])
        todo = [i for i, c in enumerate(ws.counts.tolist()) if c >= 3]
        tried = []
        for mem in [m << 19 for m in (8, 6, 12, 4, 3, 16, 24, 32, 64, 128)]:
            try:
                one = CudaPoaBatch(100, size, mem, device_id=0, cuda_banded_alignment=False)
            except (RuntimeError, ValueError):
                tried.append((mem, None))
                continue
            fits = 0
            while fits < len(todo) and \
                    one.add_poa_group_resident([t, q], ws.slices[first[todo[fits]]:first[todo[fits] + 1]])[0] == 0:
                fits += 1
            del one
            tried.append((mem, fits))
            if 0 < fits < len(todo):
                return mem, fits
    pytest.fail("no budget holds some of the %d POA windows and not all: %r" % (len(todo), tried))


@pytest.mark.parametrize("route", ["default", "device_grouping"])
def test_rounds_equal_one_round(cudapolish, inputs, references, partial_budget, route):
    """A batch that does not hold every POA window: the statuses, the failing window's among them,
    arrive at the indices they have in one round."""
    mem, fits = partial_budget
    print("max_gpu_mem %d holds %d POA windows" % (mem, fits))
    got = run(cudapolish, inputs[200], route, max_gpu_mem=mem, **polish_kwargs("w200-full"))
    want = references("w200-full")
    assert want["status"].index(ec.NODE_LIMIT_STATUS) == 1
    assert_equals_reference(got, want, RESIDENT[route])


# ---- edge inputs ----------------------------------------------------------------------------------------


@pytest.mark.parametrize("route", ROUTES)
def test_reordered_targets(cudapolish, inputs, cigars, route):
    """The empty target first and the one without overlaps between the two with reads: on the
    device-grouping routes the windows that go to the POA are then a true subset in the middle."""
    inp = ec.reordered(inputs[200])
    w, kwargs = reference_kwargs("w200-full")
    want = ec.expected(inp, w, **kwargs)
    counts = [len(x["sequences"]) for x in want["slice_windows"]]
    first_poa_after = max(i for i, n in enumerate(counts) if n >= 3)
    assert any(n < 3 for n in counts[:first_poa_after])
    assert [x["target"] for x in want["slice_windows"]] == [1] * 6 + [2] * 2 + [3] * 3
    got = run(cudapolish, inp, route, cigars[200], **polish_kwargs("w200-full"))
    assert_equals_reference(got, want, RESIDENT[route])
    assert got[0][0] == "" and got[0][2] == inp[1][2]


@pytest.mark.parametrize("route", ["default", "device_windows", "device_grouping"])
def test_no_overlaps(cudapolish, inputs, monkeypatch, route):
    """Every window keeps its backbone and no POA batch is made."""
    import claragenomicsanalysis_amd.cudapoa as cudapoa

    def no_batch(*args, **kw):
        raise AssertionError("a POA batch without a POA window")

    inp = ec.without_overlaps(inputs[200])
    w, kwargs = reference_kwargs("w200-full")
    want = ec.expected(inp, w, **kwargs)
    monkeypatch.setattr(cudapoa, "CudaPoaBatch", no_batch)
    got = run(cudapolish, inp, route, **polish_kwargs("w200-full"))
    assert_equals_reference(got, want, RESIDENT[route])
    assert got[0] == inp[1] and got[1]["backbone_by_rule"] == got[1]["windows"] == 11


@pytest.mark.parametrize("route", ["default", "device_grouping"])
def test_two_alignment_engines(cudapolish, inputs, references, route):
    got = run(cudapolish, inputs[200], route, num_alignment_engines=2, **polish_kwargs("w200-band128-cap6"))
    assert_equals_reference(got, references("w200-band128-cap6"), RESIDENT[route])
