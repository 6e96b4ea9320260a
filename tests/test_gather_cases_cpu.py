"""The long-region cases of gather_cases.py, host side (no GPU): the cases
reach the chunks, pieces and leads of gather_overlap_regions_kernel that they
are there for, so that the GPU tests of test_mapper_gather_gpu.py cannot pass
on the first piece alone.  The kernel's cut of a slot is recomputed as its
host and device code do it (gather_cases.layout and the functions next to it);
nothing here runs the kernel."""
import gather_cases as G

SETS = G.case_sets()
SLOTS = {name: G.slots_of(overlaps, stride) for name, (_, _, overlaps, stride) in SETS.items()}
STRIDE = {name: stride for name, (_, _, _, stride) in SETS.items()}
EVERY = [(name,) + s for name, slots in SLOTS.items() for s in slots]  # (set, slot, kind, length, lead, chunks)


def test_constants_and_reads():
    assert (G.CHUNK, G.PIECE, G.PIECE_CHUNKS) == (16, 4096, 256)
    reads = G.make_reads(11)
    assert [len(r) for r in reads] == [12400, 0, 9000, 1, 8300]
    assert reads != G.make_reads(12) and reads == G.make_reads(11)
    for r in G.LONG:  # the bytes the complement keeps, and the four it maps
        assert set(b"ACGTNnacgtRY\x80\xff\x00") <= set(reads[r])
    assert b"ACGTNacgt\x80".translate(G.COMPLEMENT) == b"TGCANacgt\x80"
    assert sum(1 for c in range(256) if G.COMPLEMENT[c] != c) == 4


def test_expected_is_the_plain_reverse_complement():
    queries, targets, overlaps, stride = SETS["stride_12301"]
    slots, lens = G.expected(overlaps, queries, targets, stride)
    assert len(slots) == len(lens) == 2 * len(overlaps) and lens == [len(s) for s in slots]
    pair = {ord("A"): ord("T"), ord("T"): ord("A"), ord("C"): ord("G"), ord("G"): ord("C")}
    reverse = [i for i, o in enumerate(overlaps) if o[6] == "-" and o[5] - o[4] > G.PIECE]
    for i in reverse[::20]:  # byte by byte, without translate or a reversed slice
        q, t, qs, qe, ts, te, strand = overlaps[i]
        assert slots[2 * i] == queries[q][qs:qe]
        for j in range(te - ts):
            c = targets[t][te - 1 - j]
            assert slots[2 * i + 1][j] == pair.get(c, c)
        assert set(slots[2 * i + 1]) - set(b"ACGT")
    assert len(reverse[::20]) >= 3


def test_every_overlap_lies_inside_its_reads_and_its_stride():
    for name, (queries, targets, overlaps, stride) in SETS.items():
        assert overlaps
        for q, t, qs, qe, ts, te, strand in overlaps:
            assert 0 <= qs <= qe <= len(queries[q]) and 0 <= ts <= te <= len(targets[t]), name
            assert max(qe - qs, te - ts) <= stride and strand in "+-"
        # the hook's own limit
        assert 2 * len(overlaps) * stride < 2**31
        assert 2 * len(overlaps) * stride <= 8 << 20  # and a few MB per launch
    assert len(SETS["one_overlap_12301"][2]) == 1


def test_the_strides_are_what_they_are_there_for():
    assert G.STRIDES == (12301, 12304, 12288)
    assert {G.pieces_of(s) for s in G.STRIDES + G.EVEN_LEAD_STRIDES} == {4}
    assert {(slot * 12301) % 16 for slot in range(16)} == set(range(16))
    for stride in (12304, 12288):
        assert {lead for name, _, _, _, lead, _ in EVERY if STRIDE[name] == stride} == {0}
    # what the older tests reach: one piece, whatever the slot
    assert G.pieces_of(1296) == G.pieces_of(1301) == 1 and G.pieces_of(4081) == 1 and G.pieces_of(4082) == 2
    assert G.layout(3, 1296, 1301) == (15, 82)


def test_every_seam_length_on_each_side_strand_and_source_offset():
    seen = {(kind, length) for _, _, kind, length, _, _ in EVERY}
    for length in G.SEAM_LENGTHS:
        assert {("q", length), ("+", length), ("-", length)} <= seen, length
    for name in ("stride_12301", "stride_12304", "one_read_set_flipped"):
        queries, targets, overlaps, _ = SETS[name]
        for length in G.SEAM_LENGTHS:  # in one launch
            assert {(k, n) for _, k, n, _, _ in SLOTS[name] if n == length} == {("q", length), ("+", length),
                                                                                ("-", length)}
        # the address of a region's first byte modulo 4, for the five word loads (the packed reads
        # begin on a 16-byte boundary)
        starts = {"q": [0], "t": [0]}
        for side, reads in (("q", queries), ("t", targets)):
            for r in reads:
                starts[side].append(starts[side][-1] + len(r))
        assert {(starts["q"][o[0]] + o[2]) % 4 for o in overlaps if o[3] - o[2] > G.PIECE} == {0, 1, 2, 3}
        for strand in "+-":
            assert {(starts["t"][o[1]] + o[4]) % 4 for o in overlaps
                    if o[5] - o[4] > G.PIECE and o[6] == strand} == {0, 1, 2, 3}
        assert {o[2] for o in overlaps} >= {0, 1, 2, 3} and {o[4] for o in overlaps} >= {0, 1, 2, 3}
        # both ends of the packed reads, and the reads of 0 and 1 bases
        assert any(o[0] == 0 and o[2] == 0 and o[3] > G.PIECE for o in overlaps)
        last = len(targets) - 1
        assert any(o[1] == last and o[5] == len(targets[last]) and o[5] - o[4] > G.PIECE and o[6] == "-"
                   for o in overlaps)
        assert {0, 1} <= {o[3] - o[2] for o in overlaps}


def test_leads():
    long_ = [(kind, lead, length) for _, _, kind, length, lead, _ in EVERY if length > G.PIECE]
    # a query lies at an even slot, so its lead is even at every stride and base: all of those
    assert {lead for kind, lead, _ in long_ if kind == "q"} == set(range(0, 16, 2))
    assert all((2 * i * stride) % 2 == 0 for i in range(4) for stride in (12301, 12303))
    # targets: every lead, on both strands
    for strand in "+-":
        assert {lead for kind, lead, _ in long_ if kind == strand} == set(range(16)), strand
    # the stride-12301 launch alone gives the reversed targets every odd lead and the queries every even one
    one = [(kind, lead) for _, kind, length, lead, _ in SLOTS["stride_12301"] if length > G.PIECE]
    assert {lead for kind, lead in one if kind == "-"} == set(range(1, 16, 2))
    assert {lead for kind, lead in one if kind == "q"} == set(range(0, 16, 2))
    # for each seam length: aligned, one byte into a chunk, one byte before the next
    for length in G.SEAM_LENGTHS:
        assert {0, 1, 15} <= {lead for _, _, _, n, lead, _ in EVERY if n == length}, length
        for strand in "+-":  # 1 and 15 are odd, so on targets: on both strands too
            assert {1, 15} <= {lead for _, _, kind, n, lead, _ in EVERY if n == length and kind == strand}


def test_pieces_and_their_last_chunks():
    pieces = 4
    counts = {}  # (set, slot) -> chunks taken per piece
    for name, slot, kind, length, lead, chunks in EVERY:
        per = [G.piece_chunks(chunks, p) for p in range(pieces)]
        assert sum(per) == chunks and chunks <= pieces * G.PIECE_CHUNKS, (name, slot)
        counts[(name, slot)] = (kind, length, lead, per)
    # every piece is reached, full and partly filled, on every kind of slot
    for kind in "q+-":
        for p in range(1, pieces):
            assert any(k == kind and per[p] > 0 for k, _, _, per in counts.values()), (kind, p)
            assert any(k == kind and 0 < per[p] < G.PIECE_CHUNKS for k, _, _, per in counts.values()), (kind, p)
        assert any(k == kind and per[2] == G.PIECE_CHUNKS for k, _, _, per in counts.values())
        # a region that ends with the last chunk of a piece: the next wave finds nothing and leaves
        assert any(k == kind and per[2] == G.PIECE_CHUNKS and per[3] == 0 for k, _, _, per in counts.values())
        # and one chunk for the last wave
        assert any(k == kind and per[3] == 1 for k, _, _, per in counts.values())
        assert any(k == kind and per[0] == G.PIECE_CHUNKS and per[1] == 0 for k, _, _, per in counts.values())
        assert any(k == kind and per[1] == 1 for k, _, _, per in counts.values())
    # the two the strides were chosen for
    name = "stride_12288"
    assert any(length == 12288 and lead == 0 and per == [256, 256, 256, 0]
               for (n, _), (_, length, lead, per) in counts.items() if n == name)
    name = "stride_12304"
    assert any(length == 12300 and lead == 0 and per == [256, 256, 256, 1]
               for (n, _), (_, length, lead, per) in counts.items() if n == name)
    # the single overlap: n == 1, four pieces on both slots
    for name in ("one_overlap_12301", "one_overlap_12304"):
        assert [kind for _, kind, _, _, _ in SLOTS[name]] == ["q", "-"]
        assert all(counts[(name, slot)][3][3] > 0 for slot in (0, 1))
    assert SLOTS["one_overlap_12301"][1][3] == 13


def test_chunks_at_the_piece_boundaries_on_both_paths():
    """A piece's first chunk (256 p, p >= 1) and last chunk (256 p - 1), as the one 16-byte
    store and byte by byte, and a chunk whose 16 bytes lie on both sides of byte 4096 p of the
    sequence (lead != 0), on both paths too; each on a query, a '+' and a '-' target."""
    seen = set()
    for name, slot, kind, length, lead, chunks in EVERY:
        for p in range(1, 4):
            for c, edge in ((p * G.PIECE_CHUNKS, "first"), (p * G.PIECE_CHUNKS - 1, "last")):
                if c < chunks:
                    first, last, vector = G.chunk_bytes(c, lead, length)
                    assert 0 <= first < last <= length and (last - first == G.CHUNK) == vector
                    seen.add((kind, edge, vector))
                    if first < p * G.PIECE < last:
                        seen.add((kind, "straddles", vector))
    for kind in "q+-":
        for what in ("first", "last", "straddles"):
            for vector in (True, False):
                assert (kind, what, vector) in seen, (kind, what, vector)


def test_the_chunks_of_a_slot_cover_its_sequence_once():
    for name, slot, kind, length, lead, chunks in EVERY[::7]:
        at = 0
        for c in range(chunks):
            first, last, _ = G.chunk_bytes(c, lead, length)
            assert first == at and (last > first or length == 0)  # an empty sequence mid-chunk: one chunk, no byte
            assert (slot * STRIDE[name] + first) // G.CHUNK == slot * STRIDE[name] // G.CHUNK + c
            at = last
        assert at == length
