"""Inputs shared by test_gather_cases_cpu.py (CPU) and
test_mapper_gather_gpu.py: overlaps whose regions are longer than one piece of
gather_overlap_regions_kernel (csrc/mapper_gather.hip), the bytes the kernel
has to write for them, and the kernel's cut of a slot into chunks and pieces,
restated from its host and device code so that the CPU test can say which
chunk of which piece every case reaches.

The kernel writes the sequence of slot s (2i: the query region of overlap i,
2i + 1: its target region) to bytes [s * stride, s * stride + length) of a
buffer that begins on a 16-byte boundary.  That range is cut into the aligned
16-byte chunks of the buffer, `lead` bytes of the first chunk lying before the
sequence, and the chunks into pieces of 256, one wave per piece."""
import random

CHUNK = 16    # kChunk, mapper_gather.hip
PIECE = 4096  # kPieceChunks * kChunk, mapper_gather.hip: the bytes one wave moves
PIECE_CHUNKS = PIECE // CHUNK

# A<->T and C<->G; N, lower case and every other byte stay as they are
COMPLEMENT = bytes({65: 84, 84: 65, 67: 71, 71: 67}.get(c, c) for c in range(256))

READ_LENGTHS = (12400, 0, 9000, 1, 8300)
LONG = (0, 2, 4)  # the long reads; 1 and 3 have 0 and 1 bases
# around every piece seam of a region: 4096 k, and 4096 k + 16 for a sequence that begins mid-chunk
SEAM_LENGTHS = (4080, 4081, 4095, 4096, 4097, 4111, 4112, 4113, 8191, 8192, 8193, 8209, 12288, 12289, 12300)
# 12301: odd, so slot * stride % 16 takes all 16 values over 16 consecutive slots
# 12304: lead 0 everywhere; a 12,300-byte region has 769 chunks, one of them in piece 3
# 12288: four pieces; a 12,288-byte region has exactly 768 chunks and its piece 3 is empty
STRIDES = (12301, 12304, 12288)
# A query lies at an even slot and so at an even lead whatever the stride is, and with an
# odd stride a target lies at an odd lead.  These give the targets the even leads that are
# left: 2, 6, 10 and 14, then 4 and 12, then 8.
EVEN_LEAD_STRIDES = (12302, 12308, 12296)
GRID_ROWS = 8  # overlaps per seam length: with stride 12301 the leads repeat every 8 overlaps


def make_reads(seed):
    rng = random.Random(seed)
    reads = []
    for length in READ_LENGTHS:
        read = bytearray(rng.choice(b"ACGT") for _ in range(length))
        for _ in range(length // 12):  # bytes the complement keeps
            read[rng.randrange(length)] = rng.choice(b"NnacgtRY\x80\xff\x00")
        reads.append(bytes(read))
    return reads


def _read_for(reads, length, k):
    """A long read that holds `length` bytes from any of the source offsets 0..3."""
    fits = [r for r in LONG if len(reads[r]) >= length + 3]
    return fits[k % len(fits)]


def seam_overlaps(queries, targets, stride):
    """Overlap 8 a + r has a target region of the a-th seam length that fits the
    stride and a query region of the (a + r)-th; the strands alternate with
    a + r, and both regions begin at one of the offsets 0..3 of their reads.
    After that grid: regions from base 0 of the first read and up to the last
    base of the last one, and the whole of every read that fits, the empty one
    and the single base among them."""
    lengths = [n for n in SEAM_LENGTHS if n <= stride]
    overlaps = []
    for a, target_length in enumerate(lengths):
        for r in range(GRID_ROWS):
            query_length = lengths[(a + r) % len(lengths)]
            q = _read_for(queries, query_length, a + r)
            t = _read_for(targets, target_length, a + 2 * r + 1)
            qs, ts = (a + r) % 4, (a + 3 * r + 1) % 4
            overlaps.append((q, t, qs, qs + query_length, ts, ts + target_length, "-" if (a + r) % 2 else "+"))
    last = len(queries) - 1
    for length in (4097, 8193):
        for strand in "+-":
            overlaps.append((0, 0, 0, length, 0, length, strand))
            overlaps.append((last, last, len(queries[last]) - length, len(queries[last]),
                             len(targets[last]) - length, len(targets[last]), strand))
    longest = lengths[-1]
    for strand in "+-":
        overlaps.append((0, 0, len(queries[0]) - longest, len(queries[0]), len(targets[0]) - longest,
                         len(targets[0]), strand))
    for read in range(len(queries)):
        if max(len(queries[read]), len(targets[read])) <= stride:
            for strand in "+-":
                overlaps.append((read, read, 0, len(queries[read]), 0, len(targets[read]), strand))
    return overlaps


def flip(overlaps):
    return [o[:6] + ("+" if o[6] == "-" else "-",) for o in overlaps]


# a single overlap, so n == 1: 12,300 bytes of read 0 on both sides, the target reversed
ONE_LONG_REVERSE = [(0, 0, 3, 12303, 1, 12301, "-")]


def case_sets():
    """name -> (queries, targets, overlaps, stride): one launch of the hook each."""
    a, b, c = make_reads(11), make_reads(12), make_reads(13)
    sets = {}
    for stride in STRIDES + EVEN_LEAD_STRIDES:
        sets["stride_%d" % stride] = (a, b, seam_overlaps(a, b, stride), stride)
    sets["one_read_set_flipped"] = (c, c, flip(seam_overlaps(c, c, STRIDES[0])), STRIDES[0])
    for stride in STRIDES[:2]:
        sets["one_overlap_%d" % stride] = (c, c, ONE_LONG_REVERSE, stride)
    return sets


def expected(overlaps, queries, targets, stride):
    slots, lens = [], []
    for q, t, qs, qe, ts, te, strand in overlaps:
        region = targets[t][ts:te]
        if strand == "-":
            region = region[::-1].translate(COMPLEMENT)
        slots += [queries[q][qs:qe], region]
        lens += [qe - qs, te - ts]
    assert max(lens) <= stride
    return slots, lens


# ---- the kernel's cut of a slot, restated ------------------------------------------------------

def pieces_of(stride):
    """`pieces` of gather_overlap_regions (the host side): a sequence of `stride` bytes
    that begins at any byte touches this many chunks at most."""
    return max((stride + (CHUNK - 1) + PIECE - 1) // PIECE, 1)


def layout(slot, length, stride):
    """(lead, chunks) of a slot as the kernel computes them; the buffer begins on a chunk boundary."""
    lead = slot * stride % CHUNK
    return lead, (lead + length + CHUNK - 1) // CHUNK


def piece_chunks(chunks, piece):
    """How many chunks the wave of `piece` takes: the kernel's loop bounds."""
    return max(0, min(chunks, (piece + 1) * PIECE_CHUNKS) - piece * PIECE_CHUNKS)


def chunk_bytes(c, lead, length):
    """(first, last, vector) of chunk c: the bytes [first, last) of the sequence that it
    writes, and whether it is the one 16-byte store or the byte-by-byte path."""
    j0 = c * CHUNK - lead
    if j0 >= 0 and j0 + CHUNK <= length:
        return j0, j0 + CHUNK, True
    return max(j0, 0), min(j0 + CHUNK, length), False


def slots_of(overlaps, stride):
    """(slot, kind, length, lead, chunks) per slot; kind is 'q', '+' or '-'."""
    out = []
    for i, (_, _, qs, qe, ts, te, strand) in enumerate(overlaps):
        for slot, kind, length in ((2 * i, "q", qe - qs), (2 * i + 1, strand, te - ts)):
            out.append((slot, kind, length) + layout(slot, length, stride))
    return out
