"""The fused route of cudapolish (cut, then group, on the device), many POA groups
in one call, and polish(device_grouping=True), each against the route it
replaces: window_segments_resident / window_segments_cigar followed by the host's
build_window_slices, add_poa_group_resident group by group, and
polish(device_windows=True).
"""
import os
import random
import subprocess

import numpy as np
import pytest

import polish_cases as pc
import polish_model as pm
from claragenomicsanalysis_amd import cudamapper, cudapolish
from claragenomicsanalysis_amd.cudamapper import DeviceReads
from claragenomicsanalysis_amd.cudapoa import CudaPoaBatch

pytestmark = pytest.mark.gpu

W = 16


@pytest.fixture(scope="module")
def resident_input():
    """The recipe of test_polish_gpu.py: 12 reads of about 1.2 kb against two targets, both
    strands, partial overlaps among them."""
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


def synthetic_qualities(draft, queries):
    """The recipe of test_polish_resident_gpu.py: 20..40 everywhere, but 2..8 on bases 150..650
    of reads 3 and 8."""
    rng = random.Random(9)
    quals = []
    for i, q in enumerate(queries):
        values = [rng.randint(20, 40) for _ in q]
        if i in (3, 8):
            values[150:650] = [rng.randint(2, 8) for _ in values[150:650]]
        quals.append("".join(chr(33 + v) for v in values))
    target = ["".join(chr(33 + rng.randint(5, 30)) for _ in draft)]
    return quals, target


def view(ws):
    return ws.windows(), ws.dropped_by_cap, ws.dropped_by_quality


def two_step(targets, queries, overlaps, q, t, w, cap=100, engines=1, qualities=None, threshold=10.0):
    records = cudapolish.window_segments_resident(overlaps, q, t, w, num_alignment_engines=engines)
    return cudapolish.build_window_slices(targets, queries, overlaps, records, w, cap, query_qualities=qualities,
                                          quality_threshold=threshold)


@pytest.mark.parametrize("engines", [1, 2])
def test_fused_route_equals_cut_then_host_grouping(resident_input, engines):
    targets, queries, overlaps = resident_input
    with DeviceReads(queries) as q, DeviceReads(targets) as t:
        expected = two_step(targets, queries, overlaps, q, t, W, engines=engines)
        got = view(cudapolish.window_slices_resident(overlaps, q, t, W, num_alignment_engines=engines))
        with pytest.raises(ValueError):
            cudapolish.window_slices_resident(overlaps, q, t, 0)
        with pytest.raises(ValueError):
            cudapolish.window_slices_resident(overlaps, q, t, W, num_alignment_engines=0)
        with pytest.raises(ValueError):
            cudapolish.window_slices_resident(overlaps, q, t, W, max_sequences_per_window=0)
        with pytest.raises(ValueError):
            cudapolish.window_slices_resident([(0, 0, 0, 5000, 0, 10, "+")], q, t, W)
        no_overlaps = view(cudapolish.window_slices_resident([], q, t, W))
    assert got == expected
    assert sum(len(w["slices"]) for w in got[0]) > len(got[0])  # not backbones alone
    assert no_overlaps == cudapolish.build_window_slices(targets, queries, [], [], W)


@pytest.mark.parametrize("engines", [1, 2])
def test_fused_route_with_an_overlap_past_the_aligners_limit(resident_input, engines):
    from claragenomicsanalysis_amd.cudaaligner import max_lengths
    targets, queries, overlaps = resident_input
    limit = max_lengths("hirschberg_myers")[0]
    queries = queries + ["ACGT" * (limit // 4) + "A"]
    at = len(overlaps) // 2
    overlaps = overlaps[:at] + [(len(queries) - 1, 0, 0, limit + 1, 0, 100, "+")] + overlaps[at:]
    with DeviceReads(queries) as q, DeviceReads(targets) as t:
        expected = two_step(targets, queries, overlaps, q, t, W, engines=engines)
        got = view(cudapolish.window_slices_resident(overlaps, q, t, W, num_alignment_engines=engines))
    assert got == expected
    assert not any(at in w["overlap"] for w in got[0])
    assert any(at + 1 in w["overlap"] for w in got[0])


@pytest.fixture(scope="module")
def e2e():
    truth, draft, queries, overlaps = pc.e2e_input()
    quals, target_quals = synthetic_qualities(draft, queries)
    return draft, queries, overlaps, quals, target_quals


def test_fused_route_with_qualities_and_a_cap(e2e):
    draft, queries, overlaps, quals, _ = e2e
    with DeviceReads(queries, qualities=quals) as q, DeviceReads([draft]) as t:
        expected = two_step([draft], queries, overlaps, q, t, pc.E2E_W, cap=4, qualities=quals)
        got = view(cudapolish.window_slices_resident(overlaps, q, t, pc.E2E_W, max_sequences_per_window=4))
    assert expected[1] > 0 and expected[2] > 0
    assert got == expected


def cigars_of(e2e, convention):
    """One CIGAR per overlap from the aligner's paths, written in `convention`."""
    draft, queries, overlaps, _, _ = e2e
    with DeviceReads(queries) as q, DeviceReads([draft]) as t:
        cigars = cudamapper.align_overlaps(overlaps, q, t)
    ops = [cudapolish.cigar_ops(c) for c in cigars]
    if convention == "sam":
        # I and D exchanged and, for a '-' overlap, the order of the ops reversed
        swapped = []
        for o, c in zip(overlaps, ops):
            c = np.where((c & 15) == 1, c ^ 3, np.where((c & 15) == 2, c ^ 3, c)).astype(np.uint32)
            swapped.append(c[::-1].copy() if o[6] == "-" else c)
        ops = swapped
    # the advances of the fourth no longer match its overlap's spans
    ops[3] = np.concatenate([ops[3], np.array([5 << 4 | 0], np.uint32)])
    return ops


@pytest.mark.parametrize("convention", ["genomeworks", "sam"])
def test_fused_route_from_cigars(e2e, convention):
    draft, queries, overlaps, quals, _ = e2e
    ops = cigars_of(e2e, convention)
    records = cudapolish.window_segments_cigar(overlaps, ops, pc.E2E_W, convention)
    assert all(r[6] & pm.BAD_PATH for r in pc.as_tuples(records) if r[0] == 3)
    assert not any(r[6] & pm.BAD_PATH for r in pc.as_tuples(records) if r[0] != 3)
    expected = cudapolish.build_window_slices([draft], queries, overlaps, records, pc.E2E_W, 4, query_qualities=quals)
    with DeviceReads(queries, qualities=quals) as q, DeviceReads([draft]) as t:
        got = view(cudapolish.window_slices_resident(overlaps, q, t, pc.E2E_W, max_sequences_per_window=4,
                                                     cigars=ops, cigar_convention=convention))
        with pytest.raises(ValueError):
            cudapolish.window_slices_resident(overlaps, q, t, pc.E2E_W, cigars=ops[:-1])
        with pytest.raises(ValueError):
            cudapolish.window_slices_resident(overlaps, q, t, pc.E2E_W, cigars=ops, cigar_convention="bam")
    assert got == expected
    assert not any(3 in w["overlap"] for w in got[0])


# ---- many groups in one call ----------------------------------------------------------------------------


def poa_batch(size, max_gpu_mem=1 << 30):
    return CudaPoaBatch(100, size, max_gpu_mem, device_id=0, cuda_banded_alignment=False)


def result_of(batch):
    batch.generate_poa()
    inputs = batch._download_inputs()
    return inputs, batch.get_consensus()


def test_many_groups_equal_one_by_one(e2e):
    draft, queries, overlaps, quals, target_quals = e2e
    with DeviceReads(queries, qualities=quals) as q, DeviceReads([draft], qualities=target_quals) as t:
        ws = cudapolish.window_slices_resident(overlaps, q, t, pc.E2E_W)
        one, many = poa_batch(batch_size_of(ws)), poa_batch(batch_size_of(ws))
        statuses, at = [], 0
        for c in ws.counts.tolist():
            statuses.append(one.add_poa_group_resident([t, q], ws.slices[at:at + c]))
            at += c
        added, group_status, per_seq = many.add_poa_groups_resident([t, q], ws.slices, ws.counts)
        assert added == len(ws.counts) and group_status == [s[0] for s in statuses]
        assert per_seq == [s[1] for s in statuses]
        assert result_of(many) == result_of(one)
        # an invalid slice in the last group: refused, and the batch unchanged
        many.reset()
        bad = ws.slices.copy()
        bad["end"][-1] = len(queries[bad["read"][-1]]) + 1
        with pytest.raises(ValueError):
            many.add_poa_groups_resident([t, q], bad, ws.counts)
        assert many.total_poas == 0
        with pytest.raises(ValueError):
            many.add_poa_groups_resident([t, q], ws.slices, [len(ws.slices) + 1])
        assert many.add_poa_groups_resident([t, q], ws.slices[:0], []) == (0, [], [])


def batch_size_of(ws):
    """polish's max_sequence_size for these windows."""
    return (int((ws.slices["end"] - ws.slices["begin"]).max()) + 1 + 63) // 64 * 64


@pytest.fixture(scope="module")
def partial_budget(e2e):
    """(max_gpu_mem, windows it holds): a budget of a few that holds some of the windows of the
    end-to-end input in one batch, and not all of them."""
    draft, queries, overlaps, _, _ = e2e
    with DeviceReads(queries) as q, DeviceReads([draft]) as t:
        ws = cudapolish.window_slices_resident(overlaps, q, t, pc.E2E_W)
        first = np.concatenate([[0], np.cumsum(ws.counts)])
        tried = []
        # (a window of this size costs about 1 MiB; the first budget that qualifies is taken)
        for mem in [m << 19 for m in (8, 6, 12, 4, 3, 16, 24, 32, 64, 128)]:
            try:
                one = poa_batch(batch_size_of(ws), mem)
            except (RuntimeError, ValueError):
                tried.append((mem, None))
                continue
            fits = 0
            while fits < len(ws.counts) and \
                    one.add_poa_group_resident([t, q], ws.slices[first[fits]:first[fits + 1]])[0] == 0:
                fits += 1
            del one
            tried.append((mem, fits))
            if 0 < fits < len(ws.counts):
                return mem, fits
    pytest.fail("no budget holds some of the %d windows and not all: %r" % (len(ws.counts), tried))


def test_many_groups_stop_where_the_batch_is_full(e2e, partial_budget):
    draft, queries, overlaps, _, _ = e2e
    mem, fits = partial_budget
    with DeviceReads(queries) as q, DeviceReads([draft]) as t:
        ws = cudapolish.window_slices_resident(overlaps, q, t, pc.E2E_W)
        size = batch_size_of(ws)
        first = np.concatenate([[0], np.cumsum(ws.counts)])
        print("max_gpu_mem %d holds %d of %d windows" % (mem, fits, len(ws.counts)))
        one, many = poa_batch(size, mem), poa_batch(size, mem)
        for g in range(fits):
            assert one.add_poa_group_resident([t, q], ws.slices[first[g]:first[g + 1]])[0] == 0
        assert one.add_poa_group_resident([t, q], ws.slices[first[fits]:first[fits + 1]])[0] == 1
        added, group_status, _ = many.add_poa_groups_resident([t, q], ws.slices, ws.counts)
        assert added == fits and group_status == [0] * fits
        assert many.total_poas == one.total_poas == fits
        first_round = result_of(many)
        assert first_round == result_of(one)
        # the following round continues from there
        many.reset()
        one.reset()
        again, group_status, _ = many.add_poa_groups_resident([t, q], ws.slices[first[fits]:], ws.counts[fits:])
        more = 0
        while fits + more < len(ws.counts) and one.add_poa_group_resident(
                [t, q], ws.slices[first[fits + more]:first[fits + more + 1]])[0] == 0:
            more += 1
        assert again == more > 0
        assert result_of(many) == result_of(one)


# ---- polish ---------------------------------------------------------------------------------------------


MEM = 256 << 20  # for the POA batch: its host staging is sized by it, and the default is half the device


def assert_same_polish(got, want):
    assert got[0] == want[0] and got[1] == want[1]
    assert got[2] == want[2]  # the windows, with slices, sequences and weights
    assert got[3] == want[3] and got[4] == want[4]


def test_polish_with_device_grouping(e2e, partial_budget):
    draft, queries, overlaps, _, _ = e2e
    mem = partial_budget[0]
    kwargs = dict(window_length=pc.E2E_W, banded=False, return_windows=True)
    want = cudapolish.polish([draft], queries, overlaps, device_windows=True, max_gpu_mem=MEM, **kwargs)
    got = cudapolish.polish([draft], queries, overlaps, device_grouping=True, max_gpu_mem=MEM, **kwargs)
    assert_same_polish(got, want)
    assert got[1]["windows"] == len(got[2]) and all(s == 0 for s in got[4])
    # in rounds: a batch that does not hold every window
    rounds = cudapolish.polish([draft], queries, overlaps, device_grouping=True, max_gpu_mem=mem, **kwargs)
    assert_same_polish(rounds, want)


def test_polish_with_device_grouping_qualities_and_trim(e2e):
    draft, queries, overlaps, quals, target_quals = e2e
    kwargs = dict(window_length=pc.E2E_W, banded=False, return_windows=True, query_qualities=quals,
                  target_qualities=target_quals, trim=True, max_sequences_per_window=6, max_gpu_mem=MEM)
    want = cudapolish.polish([draft], queries, overlaps, **kwargs)
    got = cudapolish.polish([draft], queries, overlaps, device_grouping=True, **kwargs)
    assert want[1]["dropped_by_quality"] > 0 and want[1]["dropped_by_cap"] > 0
    assert_same_polish(got, want)


def test_polish_with_device_grouping_from_cigars(e2e):
    draft, queries, overlaps, _, _ = e2e
    ops = cigars_of(e2e, "sam")
    kwargs = dict(window_length=pc.E2E_W, banded=False, return_windows=True, cigars=ops, cigar_convention="sam",
                  max_gpu_mem=MEM)
    want = cudapolish.polish([draft], queries, overlaps, device_windows=True, **kwargs)
    got = cudapolish.polish([draft], queries, overlaps, device_grouping=True, **kwargs)
    assert_same_polish(got, want)


def test_cpp_interface(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "claragenomicsanalysis_amd", "lib")
    exe = str(tmp_path / "polish_group_cpp_check")
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-std=c++17", "-O1", "-Wall",
                           "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(root, "include"), "-I", "/opt/rocm/include",
                           "-x", "c++", os.path.join(root, "tests", "polish_group_cpp_check.cpp"), "-L", lib,
                           "-lgwamd", "-Wl,-rpath," + lib, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == [word for name in ("fused_counts", "fused_slices", "device_grouping", "cigar_route",
                                                  "groups_added", "groups_consensus") for word in ("ok", name)]
