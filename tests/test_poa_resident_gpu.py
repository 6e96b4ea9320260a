"""GPU tests of POA groups added as slices of resident reads
(gwamd_poa_add_poa_group_resident, polish_gather.hip).

Kernel bytes: after upload() the batch's packed bases and weights are copied
back (gwamd_internal_poa_download_inputs) and compared byte for byte, the 16
trailing zeros included, with the model (polish_resident_model.py).  Sequences
are packed back to back, so slice lengths that run through the edge cases put
destinations on every alignment mod 16 and make neighbours share 16-byte chunks.

Equivalence: the same windows added from the host (strings + weights) and as
slices give the same statuses, consensus, coverage and graphs, and both equal
the oracle with those weights, on the LDS full kernel, the banded route and the
global-memory kernel.
"""
import random

import numpy as np
import pytest

import polish_resident_model as rm
from claragenomicsanalysis_amd import synth
from claragenomicsanalysis_amd.cudamapper import DeviceReads
from claragenomicsanalysis_amd.cudapoa import CudaPoaBatch
from oracle import oracle

pytestmark = pytest.mark.gpu
MEM = 1 << 30
PIECE = 4096  # bytes of a sequence one wave writes (kPieceChunks * kChunk, mapper_gather.hpp)
WAVES = 4     # waves of one workgroup of the gather
LENGTHS = [0, 1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 1023, 1024, 1025, PIECE - 16, PIECE - 15, PIECE - 1, PIECE,
           PIECE + 1, 2 * PIECE + 1]
MAX_SEQ = 2 * PIECE + 64


@pytest.fixture(scope="module")
def reads():
    """Two read sets on the device: set 0 with qualities, set 1 without.  Bases
    include N and lower case; the first and last read of a set touch its pad."""
    rng = random.Random(20)

    def text(n):
        return "".join(rng.choice("ACGTACGTNacgtn") for _ in range(n))

    def quality(n):
        return "".join(chr(rng.randint(33, 126)) for _ in range(n))

    lengths = [[2 * PIECE + 40, 1, 37, 0, 3000, 2 * PIECE + 7], [19, 2 * PIECE + 50, 5, 700]]
    sets = [[text(n) for n in lens] for lens in lengths]
    qualities = [[quality(len(r)) for r in sets[0]], None]
    device = [DeviceReads(sets[0], qualities=qualities[0]), DeviceReads(sets[1])]
    assert device[0].has_qualities and not device[1].has_qualities
    yield sets, qualities, device
    for d in device:
        d.close()


@pytest.fixture(scope="module")
def batch():
    # banded: a window's share of the score budget does not grow with its longest sequence
    return CudaPoaBatch(64, MAX_SEQ, 2 << 30, cuda_banded_alignment=True)


def add_and_check(batch, reads, groups):
    """groups: ("resident", [slices]) or ("host", [(text, weights or None)]).  Adds them to the
    reset batch, uploads, and compares the device's bytes with the model's."""
    sets, qualities, device = reads
    batch.reset()
    expected = []
    for kind, members in groups:
        if kind == "resident":
            st, per_seq = batch.add_poa_group_resident(device, members)
            expected += [(rm.slice_bases(sets, sl), rm.slice_weights(qualities, sl)) for sl in members]
        else:
            st, per_seq = batch.add_poa_group([t for t, _ in members], weights=[w for _, w in members])
            expected += [(t, [1] * len(t) if w is None else list(w)) for t, w in members]
        assert st == 0 and per_seq == [0] * len(members)
    batch.upload()
    bases, weights = batch._download_inputs()
    want_bases, want_weights = rm.packed_inputs(expected)
    assert len(bases) == len(want_bases) and len(weights) == len(want_weights)
    assert bases == want_bases
    assert weights == want_weights
    batch.reset()


def slices_of_lengths(sets, lengths, rng, turn=1):
    """One slice per length, from a read long enough, at a random begin; the set and
    the strand change every `turn` slices through all four combinations."""
    out = []
    for i, n in enumerate(lengths):
        s, flags = (i // turn) % 2, (i // turn // 2) % 2
        r = rng.choice([j for j, read in enumerate(sets[s]) if len(read) >= n])
        b = rng.randint(0, len(sets[s][r]) - n)
        out.append((s, r, b, b + n, flags))
    return out


def destination_alignments(slices):
    return set((np.cumsum([0] + [sl[3] - sl[2] for sl in slices[:-1]]) % 16).tolist())


@pytest.mark.parametrize("order", ["ladder", "shuffled"])
def test_slice_lengths_through_every_edge(batch, reads, order):
    rng = random.Random(31)
    # four passes up the ladder of lengths: each length from both sets and on both strands
    slices = slices_of_lengths(reads[0], [n for _ in range(4) for n in LENGTHS], rng, turn=len(LENGTHS))
    assert len(set((sl[3] - sl[2], sl[0], sl[4]) for sl in slices)) == 4 * len(LENGTHS)
    if order == "shuffled":  # the first seeded order that also puts a destination on every alignment
        orders = (random.Random(seed).sample(slices, len(slices)) for seed in range(100))
        slices = next(o for o in orders if len(destination_alignments(o)) == 16)
    assert len(destination_alignments(slices)) == 16
    add_and_check(batch, reads, [("resident", slices[i:i + 10]) for i in range(0, len(slices), 10)])


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("length", [40, 7])
def test_source_begin_at_sixteen_consecutive_offsets(batch, reads, flags, length):
    groups = []
    for s, r in ((0, 4), (1, 1)):
        groups.append(("resident", [(s, r, 100 + b, 100 + b + length, flags) for b in range(16)]))
        # a length that is a multiple of 16 keeps the destination alignment fixed while the source moves
        groups.append(("resident", [(s, r, 200 + b, 200 + b + 48, flags) for b in range(16)]))
    add_and_check(batch, reads, groups)


def test_first_and_last_bases_of_reads_and_sets(batch, reads):
    sets = reads[0]
    slices = []
    for s in (0, 1):
        for r, read in enumerate(sets[s]):
            n = len(read)
            for b, e in ((0, n), (0, min(n, 17)), (max(n - 17, 0), n), (0, min(n, 1)), (max(n - 1, 0), n), (n, n)):
                slices += [(s, r, b, e, 0), (s, r, b, e, 1)]
    assert len(slices) > 64  # more than one group
    add_and_check(batch, reads, [("resident", slices[i:i + 60]) for i in range(0, len(slices), 60)])


@pytest.mark.parametrize("count", [1, WAVES - 1, WAVES, WAVES + 1, 2 * WAVES + 1])
def test_sequence_counts_around_one_workgroup(batch, reads, count):
    rng = random.Random(count)
    slices = slices_of_lengths(reads[0], [rng.randint(1, 90) for _ in range(count)], rng)
    add_and_check(batch, reads, [("resident", slices)])
    # the same count with pieces: a long first sequence makes every sequence own three waves
    add_and_check(batch, reads, [("resident", [(0, 0, 3, 3 + 2 * PIECE + 5, 1)] + slices[1:])])


def test_non_acgt_bytes_are_kept(batch, reads):
    sets, qualities, _ = reads
    with DeviceReads(["NNacgtNRYKMnACGT", "acgtn"], qualities=["I" * 16, "5" * 5]) as odd:
        local = ([sets[0], ["NNacgtNRYKMnACGT", "acgtn"]], [qualities[0], ["I" * 16, "5" * 5]], [reads[2][0], odd])
        slices = [(1, 0, 0, 16, 1), (1, 0, 0, 16, 0), (1, 1, 0, 5, 1), (1, 0, 3, 13, 1)]
        assert rm.slice_bases(local[0], slices[0]) == "ACGTnMKYRNtgcaNN"  # only A, C, G, T are complemented
        add_and_check(batch, local, [("resident", slices)])


def test_host_and_resident_groups_mixed_in_one_batch(batch, reads):
    rng = random.Random(41)
    host_a = [("ACGTTGCAACGTNNA", [3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5, 8, 9, 7, 9]), ("GATTACA" * 9, None), ("", None)]
    host_b = [("".join(rng.choice("ACGT") for _ in range(n)), [rng.randint(0, 93) for _ in range(n)])
              for n in (33, 1, 500)]
    res_a = slices_of_lengths(reads[0], [5, 17, 300, 0, 64], rng)
    res_b = slices_of_lengths(reads[0], [PIECE + 3, 31, 2], rng)
    for groups in ([("host", host_a), ("resident", res_a), ("host", host_b), ("resident", res_b)],
                   [("resident", res_b), ("host", host_b), ("host", host_a), ("resident", res_a), ("host", host_a)],
                   [("host", host_a), ("host", host_b)]):
        add_and_check(batch, reads, groups)


def test_batch_reused_after_reset(batch, reads):
    rng = random.Random(43)
    long_first = slices_of_lengths(reads[0], [2 * PIECE + 1, 900, 16], rng)
    short_next = slices_of_lengths(reads[0], [3, 15], rng)
    add_and_check(batch, reads, [("resident", long_first)])
    add_and_check(batch, reads, [("resident", short_next)])  # fewer and shorter than before the reset
    add_and_check(batch, reads, [("host", [("ACGT", None)])])
    add_and_check(batch, reads, [("resident", long_first), ("resident", short_next)])


# ---- equivalence with the host route ----------------------------------------------------------------

# (GWAMD_* tuning, banded, expected kernel_variant), chosen as tests/test_poa_weights.py chooses them
ROUTES = {
    "lds": ({}, False, 2),
    "banded": ({"GWAMD_BAND_FWD": "row"}, True, 3),
    "global": ({"GWAMD_POA_KERNEL": "v1"}, False, 1),
}


@pytest.fixture(scope="module")
def weighted_windows():
    """4 windows x 6 reads x about 200 bases with Phred-like weights, and the same
    sequences as slices: every sequence sits inside a read of its own with a few
    bases before and after, every second one stored reverse-complemented (with
    its quality string turned round), so a reverse slice gives it back."""
    from polish_model import reverse_complement
    rng = random.Random(77)
    wins = [[s.decode() for s in w] for w in synth.poa_windows(2101, 4, 200, 6, 12, 12, 12)]
    weights = [[[rng.randint(0, 60) for _ in s] for s in w] for w in wins]
    stored, quals, slices = [], [], []
    for w, ww in zip(wins, weights):
        group = []
        for s, x in zip(w, ww):
            reverse = len(stored) % 2
            before, after = rng.randint(0, 9), rng.randint(0, 9)
            body = reverse_complement(s) if reverse else s
            q = "".join(chr(33 + v) for v in (x[::-1] if reverse else x))
            stored.append("T" * before + body + "G" * after)
            quals.append("#" * before + q + "#" * after)
            group.append((0, len(stored) - 1, before, before + len(s), reverse))
        slices.append(group)
    results = {}

    def expect(banded, score_bits, max_seq, max_seqs):
        key = (banded, score_bits)
        if key not in results:
            mn = ((4 if banded else 3) * max_seq + 3) // 4 * 4
            results[key] = [oracle.poa_window([s.encode() for s in w], weights=[np.array(x, np.int8) for x in ww],
                                              banded=banded, band_width=256, score_bits=score_bits, max_nodes=mn,
                                              max_consensus=2 * max_seq, max_seqs=max_seqs, want_graph=True)
                            for w, ww in zip(wins, weights)]
        return results[key]

    return wins, weights, stored, quals, slices, expect


def graph_edges(batch):
    graphs, status = batch.get_graphs()
    return [{(u, v): g.weight(u, v) for (u, v) in g.edges} for g in graphs], status


@pytest.mark.parametrize("route", list(ROUTES))
def test_resident_groups_equal_host_groups_and_oracle(route, weighted_windows, monkeypatch):
    env, banded, variant = ROUTES[route]
    for k in ("GWAMD_POA_KERNEL", "GWAMD_BAND_FWD"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    wins, weights, stored, quals, slices, expect = weighted_windows
    max_seq, max_seqs = 320, 8
    host = CudaPoaBatch(max_seqs, max_seq, MEM, cuda_banded_alignment=banded)
    dev = CudaPoaBatch(max_seqs, max_seq, MEM, cuda_banded_alignment=banded)
    assert host.kernel_variant() == dev.kernel_variant() == variant
    with DeviceReads(stored, qualities=quals) as resident:
        for w, ww, group in zip(wins, weights, slices):
            a = host.add_poa_group(w, weights=[np.array(x, np.int8) for x in ww])
            b = dev.add_poa_group_resident([resident], group)
            assert a == b == (0, [0] * len(w))
        host.generate_poa()
        dev.generate_poa()
        got_host, got_dev = host.get_consensus(), dev.get_consensus()
        edges_host, edges_dev = graph_edges(host), graph_edges(dev)
    assert got_dev == got_host and edges_dev == edges_host
    want = expect(banded, dev.get_types()[0], max_seq, max_seqs)
    cons, cov, status = got_dev
    for i, r in enumerate(want):
        assert (status[i], cons[i], cov[i]) == (r.status, r.consensus, r.coverage), (route, i)
        assert edges_dev[0][i] == {(src, v): wt for v, ins in enumerate(r.graph["in"]) for (src, wt) in ins}, i
    # the qualities are what weighs: the same slices of a set without qualities give other edge weights
    with DeviceReads(stored) as plain:
        dev.reset()
        assert dev.add_poa_group_resident([plain], slices[0])[0] == 0
        dev.generate_poa()
        assert graph_edges(dev)[0][0] != edges_dev[0][0]


def test_statuses_are_the_host_routes():
    rng = random.Random(5)
    read = "".join(rng.choice("ACGT") for _ in range(400))
    with DeviceReads([read]) as resident:
        host = CudaPoaBatch(3, 128, 64 << 20, cuda_banded_alignment=True, alignment_band_width=128)
        dev = CudaPoaBatch(3, 128, 64 << 20, cuda_banded_alignment=True, alignment_band_width=128)

        def both(spans):
            a = host.add_poa_group([read[b:e] for b, e in spans])
            b = dev.add_poa_group_resident([resident], [(0, 0, b, e, 0) for b, e in spans])
            assert a == b
            return b

        # a slice longer than max_sequence_size: exceeded_maximum_sequence_size for that one alone
        assert both([(0, 100), (0, 129), (5, 105)]) == (0, [0, 2, 0])
        assert both([(0, 128), (0, 0)]) == (0, [0, 0])
        # one sequence too many: exceeded_maximum_sequences_per_poa for the fourth
        assert both([(0, 50), (1, 51), (2, 52), (3, 53)]) == (0, [0, 0, 0, 3])
        # a batch that is full: exceeded_maximum_poas, then flush and re-add
        max_poas = dev.get_capacity()[1]
        assert host.get_capacity()[1] == max_poas and max_poas < 20000
        while dev.total_poas < max_poas:
            assert both([(0, 60), (2, 62), (4, 64)])[0] == 0
        assert both([(0, 60), (2, 62), (4, 64)]) == (1, [1, 1, 1])
        assert dev.total_poas == host.total_poas == max_poas
        host.generate_poa()
        dev.generate_poa()
        assert dev.get_consensus() == host.get_consensus()
        host.reset()
        dev.reset()
        assert both([(0, 60), (2, 62), (4, 64)]) == (0, [0, 0, 0])
        host.generate_poa()
        dev.generate_poa()
        assert dev.get_consensus() == host.get_consensus() and dev.get_consensus()[2] == [0]


# ---- argument errors --------------------------------------------------------------------------------


def test_argument_errors_leave_the_batch_usable(batch, reads):
    sets, qualities, device = reads
    batch.reset()
    assert batch.add_poa_group_resident(device, [(0, 4, 0, 10, 0)])[0] == 0
    bad = [
        [(0, len(sets[0]), 0, 0, 0)],                # a read id out of range
        [(0, 2, 0, len(sets[0][2]) + 1, 0)],         # end past the read
        [(0, 2, 5, 4, 0)],                           # begin > end
        [(2, 0, 0, 1, 0)], [(-1, 0, 0, 1, 0)],       # set out of range
        [(1, 0, 0, 5, 0), (1, 3, 0, 701, 1)],        # the second slice is bad: nothing of the group is added
    ]
    for slices in bad:
        with pytest.raises(ValueError):
            batch.add_poa_group_resident(device, slices)
        assert batch.total_poas == 1
    with pytest.raises(ValueError):
        batch.add_poa_group_resident([device[0], None], [(0, 0, 0, 1, 0)])
    closed = DeviceReads(["ACGT"])
    closed.close()
    with pytest.raises(ValueError):
        batch.add_poa_group_resident([closed], [(0, 0, 0, 1, 0)])
    assert batch.total_poas == 1
    # the batch goes on: one more group, and the bytes are those of the two good groups
    batch.reset()
    add_and_check(batch, reads, [("resident", [(0, 4, 0, 10, 0)]), ("resident", [(1, 1, 7, 90, 1), (0, 2, 0, 37, 1)])])


def test_set_on_another_device_is_refused():
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    b = CudaPoaBatch(4, 128, 64 << 20, device_id=0, alignment_band_width=128)
    with DeviceReads(["ACGTACGT"], device_id=1) as other:
        with pytest.raises(ValueError, match="device"):
            b.add_poa_group_resident([other], [(0, 0, 0, 8, 0)])
    with DeviceReads(["ACGTACGT"], device_id=0) as here:
        assert b.add_poa_group_resident([here], [(0, 0, 0, 8, 0)]) == (0, [0])
