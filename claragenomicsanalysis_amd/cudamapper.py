"""Minimizer index, anchor matcher, overlapper, overlap-end rescue, overlap
alignment and PAF output of cudamapper over the C ABI (include/gwamd_cudamapper.h; reference
cudamapper/include/.../index.hpp, matcher.hpp, overlapper.hpp,
cudamapper/src/main.cu:48-175 and cudamapper/src/cudamapper_utils.cpp:30-112).

Index builds the (k,w)-minimizer index of a range of reads on the GPU,
match_anchors pairs the sketch elements of two indices that share a
representation, and get_overlaps chains sorted anchors into Overlap records
(match_overlaps does both without bringing the anchors to the host).
rescue_overlap_ends pushes the ends of overlaps out towards the read ends on
the GPU; extend_overlap_by_sequence_similarity is one round of it on the host.

Overlaps are aligned with the MI355X global aligner (Hirschberg-Myers, the
aligner create_aligner returns); a Reverse ('-') overlap aligns the query
region against the reverse complement of the target region.
"""
import ctypes as C

import numpy as np

from ._lib import load_library, last_error


class Overlap(C.Structure):
    """cudamapper::Overlap (cudamapper/include/.../types.hpp:68-89)."""
    _fields_ = [("query_read_id", C.c_uint32), ("target_read_id", C.c_uint32),
                ("query_start", C.c_uint32), ("target_start", C.c_uint32),
                ("query_end", C.c_uint32), ("target_end", C.c_uint32),
                ("relative_strand", C.c_ubyte), ("num_residues", C.c_uint32),
                ("overlap_complete", C.c_uint8)]

    def __init__(self, query_read_id, target_read_id, query_start, query_end, target_start, target_end,
                 strand="+", num_residues=0, overlap_complete=False):
        s = strand.encode() if isinstance(strand, str) else bytes([strand])
        super().__init__(query_read_id, target_read_id, query_start, target_start, query_end, target_end,
                         s[0], num_residues, int(bool(overlap_complete)))

    @property
    def strand(self):
        return chr(self.relative_strand)


class IndexInfo(C.Structure):
    """gwamd_index_info_t."""
    _fields_ = [("num_elements", C.c_int64), ("num_unique_representations", C.c_int64),
                ("number_of_reads", C.c_uint32), ("smallest_read_id", C.c_uint32),
                ("largest_read_id", C.c_uint32), ("number_of_basepairs_in_longest_read", C.c_uint32)]


# cudamapper::Anchor (types.hpp:52-62)
ANCHOR_DTYPE = np.dtype([("query_read_id", np.uint32), ("target_read_id", np.uint32),
                         ("query_position_in_read", np.uint32), ("target_position_in_read", np.uint32)])

FORWARD, REVERSE = 0, 1  # SketchElement::DirectionOfRepresentation


def _declare(L):
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    P = C.POINTER
    L.gwamd_align_overlaps.restype = i32
    L.gwamd_align_overlaps.argtypes = [C.c_char_p, vp, i32, C.c_char_p, vp, i32, vp, i32, i32, i32, P(vp)]
    L.gwamd_format_paf.restype = i32
    L.gwamd_format_paf.argtypes = [C.c_char_p, vp, vp, i32, C.c_char_p, vp, vp, i32, vp, i32, vp, i32, P(vp)]
    L.gwamd_read_fasta.restype = i32
    L.gwamd_read_fasta.argtypes = [C.c_char_p, C.c_uint32, i32, P(vp), P(vp)]
    L.gwamd_text_list_create.restype = i32
    L.gwamd_text_list_create.argtypes = [vp, vp, i32, P(vp)]
    L.gwamd_text_list_size.restype = i32
    L.gwamd_text_list_size.argtypes = [vp]
    L.gwamd_text_list_get.restype = i32
    L.gwamd_text_list_get.argtypes = [vp, i32, P(C.c_void_p), P(i64)]
    L.gwamd_text_list_free.restype = None
    L.gwamd_text_list_free.argtypes = [vp]
    index_args = [C.c_char_p, vp, i32, i32, i32, i32, i32, i32, C.c_double, i32]
    L.gwamd_index_create.restype = i32
    L.gwamd_index_create.argtypes = index_args + [P(vp)]
    L.gwamd_index_create_with_allocator.restype = i32
    L.gwamd_index_create_with_allocator.argtypes = index_args + [vp, P(vp)]
    L.gwamd_index_free.restype = None
    L.gwamd_index_free.argtypes = [vp]
    L.gwamd_index_info.restype = i32
    L.gwamd_index_info.argtypes = [vp, P(IndexInfo)]
    L.gwamd_index_copy.restype = i32
    L.gwamd_index_copy.argtypes = [vp] * 7
    L.gwamd_match_anchors.restype = i32
    L.gwamd_match_anchors.argtypes = [vp, vp, i64, P(vp), P(i64)]
    L.gwamd_match_anchors_with_allocator.restype = i32
    L.gwamd_match_anchors_with_allocator.argtypes = [vp, vp, i64, vp, P(vp), P(i64)]
    L.gwamd_anchors_free.restype = None
    L.gwamd_anchors_free.argtypes = [vp]
    filter_args = [i64, i64, i64, C.c_float]
    L.gwamd_get_overlaps.restype = i32
    L.gwamd_get_overlaps.argtypes = [vp, i64] + filter_args + [i32, P(vp), P(i64)]
    L.gwamd_get_overlaps_with_allocator.restype = i32
    L.gwamd_get_overlaps_with_allocator.argtypes = [vp, i64] + filter_args + [i32, vp, P(vp), P(i64)]
    L.gwamd_match_overlaps.restype = i32
    L.gwamd_match_overlaps.argtypes = [vp, vp, i64] + filter_args + [P(vp), P(i64), P(i64)]
    L.gwamd_match_overlaps_with_allocator.restype = i32
    L.gwamd_match_overlaps_with_allocator.argtypes = [vp, vp, i64] + filter_args + [vp, P(vp), P(i64), P(i64)]
    L.gwamd_post_process_overlaps.restype = i32
    L.gwamd_post_process_overlaps.argtypes = [vp, i64, i32, P(vp), P(i64)]
    L.gwamd_overlaps_free.restype = None
    L.gwamd_overlaps_free.argtypes = [vp]
    rescue_args = [C.c_char_p, vp, i32, C.c_char_p, vp, i32, vp, i64, i32, C.c_float, i32]
    L.gwamd_rescue_overlap_ends.restype = i32
    L.gwamd_rescue_overlap_ends.argtypes = rescue_args + [P(vp), P(i64)]
    L.gwamd_rescue_overlap_ends_with_allocator.restype = i32
    L.gwamd_rescue_overlap_ends_with_allocator.argtypes = rescue_args + [vp, P(vp), P(i64)]
    L.gwamd_extend_overlap_by_sequence_similarity.restype = i32
    L.gwamd_extend_overlap_by_sequence_similarity.argtypes = [P(Overlap), C.c_char_p, i64, C.c_char_p, i64, i32,
                                                              C.c_float]


def _check(rc):
    if rc == -1:
        raise ValueError(last_error())
    if rc < 0:
        raise RuntimeError(last_error())
    return rc


def _pack(items):
    data = [x.encode() if isinstance(x, str) else bytes(x) for x in items]
    offs = (C.c_int64 * (len(data) + 1))()
    for i, d in enumerate(data):
        offs[i + 1] = offs[i] + len(d)
    return b"".join(data), offs


def _overlap_array(overlaps):
    arr = (Overlap * max(len(overlaps), 1))()
    for i, o in enumerate(overlaps):
        arr[i] = o if isinstance(o, Overlap) else Overlap(*o)
    return arr


def _take(L, handle):
    try:
        out = []
        for i in range(L.gwamd_text_list_size(handle)):
            p, n = C.c_void_p(), C.c_int64()
            _check(L.gwamd_text_list_get(handle, i, C.byref(p), C.byref(n)))
            out.append(C.string_at(p, n.value).decode())
        return out
    finally:
        L.gwamd_text_list_free(handle)


def align_overlaps(overlaps, query_reads, target_reads, num_alignment_engines=1, device_id=0):
    """CIGAR of every overlap (align_overlaps, main.cu:125-175).

    query_reads / target_reads: sequences indexed by the overlaps' read ids."""
    L = load_library()
    qb, qo = _pack(query_reads)
    tb, to = _pack(target_reads)
    arr = _overlap_array(overlaps)
    h = C.c_void_p()
    _check(L.gwamd_align_overlaps(qb, qo, len(query_reads), tb, to, len(target_reads), arr, len(overlaps),
                                  num_alignment_engines, device_id, C.byref(h)))
    return _take(L, h)


def format_paf(overlaps, cigars, query_reads, target_reads, kmer_size):
    """PAF text of print_paf (cudamapper_utils.cpp:30-112).

    query_reads / target_reads: (name, sequence or length) per read id; cigars
    may be None or empty (no cg:Z: tag)."""
    L = load_library()
    qn, qno = _pack([r[0] for r in query_reads])
    tn, tno = _pack([r[0] for r in target_reads])
    qlen = (C.c_int64 * max(len(query_reads), 1))(*[r[1] if isinstance(r[1], int) else len(r[1])
                                                    for r in query_reads])
    tlen = (C.c_int64 * max(len(target_reads), 1))(*[r[1] if isinstance(r[1], int) else len(r[1])
                                                     for r in target_reads])
    arr = _overlap_array(overlaps)
    cig = None
    if cigars:
        data = [c.encode() if isinstance(c, str) else bytes(c) for c in cigars]
        ptrs = (C.c_char_p * len(data))(*data)
        lens = (C.c_int64 * len(data))(*[len(d) for d in data])
        cig = C.c_void_p()
        _check(L.gwamd_text_list_create(ptrs, lens, len(data), C.byref(cig)))
    h = C.c_void_p()
    try:
        _check(L.gwamd_format_paf(qn, qno, qlen, len(query_reads), tn, tno, tlen, len(target_reads), arr,
                                  len(overlaps), cig, kmer_size, C.byref(h)))
    finally:
        if cig is not None:
            L.gwamd_text_list_free(cig)
    return _take(L, h)[0]


def read_fasta(path, min_sequence_length=0, shuffle=True):
    """(name, sequence) records as io::create_kseq_fasta_parser holds them
    (kseqpp_fasta_parser.cpp:31-72): shorter records dropped, shuffled with
    std::mt19937(0) unless shuffle is False."""
    L = load_library()
    n, s = C.c_void_p(), C.c_void_p()
    _check(L.gwamd_read_fasta(str(path).encode(), int(min_sequence_length), int(bool(shuffle)), C.byref(n),
                              C.byref(s)))
    return list(zip(_take(L, n), _take(L, s)))


class Index:
    """(k,w)-minimizer index of reads[first_read_id:past_the_last_read_id]
    (Index::create_index, index.hpp:97-106), built on the GPU.

    reads: sequences (str or bytes), or (name, sequence) records as read_fasta
    returns them.  The six arrays are numpy arrays ordered by (representation,
    read_id, position_in_read); read ids are indices into reads.  A read
    shorter than window_size + kmer_size - 1 contributes nothing and keeps its
    id.  allocator: a cudaaligner.DeviceAllocator whose pool the device memory
    is counted against."""

    def __init__(self, reads, kmer_size, window_size, first_read_id=0, past_the_last_read_id=None,
                 hash_representations=True, filtering_parameter=1.0, device_id=0, allocator=None):
        self._lib = load_library()
        self._handle = C.c_void_p()
        seqs = [r[1] if isinstance(r, tuple) else r for r in reads]
        if past_the_last_read_id is None:
            past_the_last_read_id = len(seqs)
        bases, offsets = _pack(seqs)
        args = [bases, offsets, len(seqs), int(first_read_id), int(past_the_last_read_id), int(kmer_size),
                int(window_size), int(bool(hash_representations)), float(filtering_parameter), int(device_id)]
        if allocator is not None:
            _check(self._lib.gwamd_index_create_with_allocator(*args, allocator._handle, C.byref(self._handle)))
            self._allocator = allocator  # the index holds bytes of its pool
        else:
            _check(self._lib.gwamd_index_create(*args, C.byref(self._handle)))
        try:
            info = IndexInfo()
            _check(self._lib.gwamd_index_info(self._handle, C.byref(info)))
            n, u = info.num_elements, info.num_unique_representations
            self.representations = np.empty(n, np.uint64)
            self.read_ids = np.empty(n, np.uint32)
            self.positions_in_reads = np.empty(n, np.uint32)
            self.directions_of_reads = np.empty(n, np.uint8)
            self.unique_representations = np.empty(u, np.uint64)
            self.first_occurrence_of_representations = np.empty(u + 1 if n else 0, np.uint32)
            _check(self._lib.gwamd_index_copy(
                self._handle, *[a.ctypes.data_as(C.c_void_p) for a in (
                    self.representations, self.read_ids, self.positions_in_reads, self.directions_of_reads,
                    self.unique_representations, self.first_occurrence_of_representations)]))
        except Exception:
            self.close()
            raise
        self.number_of_reads = int(info.number_of_reads)
        self.smallest_read_id = int(info.smallest_read_id)
        self.largest_read_id = int(info.largest_read_id)
        self.number_of_basepairs_in_longest_read = int(info.number_of_basepairs_in_longest_read)

    def close(self):
        """Frees the index's device memory; the numpy arrays stay valid."""
        h, self._handle = self._handle, C.c_void_p()
        if h:
            self._lib.gwamd_index_free(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def match_anchors(query_index, target_index, max_anchors=None, allocator=None):
    """Anchors of two indices (Matcher::create_matcher, matcher.hpp:45-48): a
    structured numpy array (ANCHOR_DTYPE) of every pair of a query and a target
    sketch element with the same representation, sorted by (query_read_id,
    target_read_id, query_position_in_read, target_position_in_read).

    RuntimeError when there are more than max_anchors (default 2^31)."""
    L = load_library()
    if not query_index._handle or not target_index._handle:
        raise ValueError("index is closed")
    p, n = C.c_void_p(), C.c_int64()
    cap = -1 if max_anchors is None else int(max_anchors)
    if cap < 0 and max_anchors is not None:
        raise ValueError("max_anchors must not be negative")
    if allocator is not None:
        _check(L.gwamd_match_anchors_with_allocator(query_index._handle, target_index._handle, cap,
                                                    allocator._handle, C.byref(p), C.byref(n)))
    else:
        _check(L.gwamd_match_anchors(query_index._handle, target_index._handle, cap, C.byref(p), C.byref(n)))
    try:
        out = np.empty(n.value, ANCHOR_DTYPE)
        if n.value:
            C.memmove(out.ctypes.data, p, n.value * ANCHOR_DTYPE.itemsize)
        return out
    finally:
        L.gwamd_anchors_free(p)


def _filter_args(min_residues, min_overlap_len, min_bases_per_residue, min_overlap_fraction):
    return [int(min_residues), int(min_overlap_len), int(min_bases_per_residue), float(min_overlap_fraction)]


def _copy(overlap):
    c = Overlap.__new__(Overlap)
    C.memmove(C.byref(c), C.byref(overlap), C.sizeof(Overlap))
    return c


def _take_overlaps(L, p, n):
    try:
        arr = (Overlap * n.value).from_address(p.value) if n.value else []
        return [_copy(o) for o in arr]
    finally:
        L.gwamd_overlaps_free(p)


def get_overlaps(anchors, min_residues=20, min_overlap_len=50, min_bases_per_residue=50, min_overlap_fraction=0.9,
                 device_id=0, allocator=None):
    """Overlaps of sorted anchors (OverlapperTriggered::get_overlaps,
    overlapper_triggered.cu:232-427), chained, fused and filtered on the GPU.

    anchors: an ANCHOR_DTYPE array, as match_anchors returns it, or (query_read_id,
    target_read_id, query_position_in_read, target_position_in_read) tuples.
    Returns a list of Overlap in anchor order, ready for align_overlaps and
    format_paf.  ValueError for a negative or NaN parameter, for anchors that
    are not sorted and for a position of 2^31 or more."""
    L = load_library()
    if not (isinstance(anchors, np.ndarray) and anchors.dtype == ANCHOR_DTYPE):
        anchors = np.array([tuple(a) for a in anchors], dtype=ANCHOR_DTYPE)
    anchors = np.ascontiguousarray(anchors)
    p, n = C.c_void_p(), C.c_int64()
    args = [anchors.ctypes.data_as(C.c_void_p), len(anchors)] + \
        _filter_args(min_residues, min_overlap_len, min_bases_per_residue, min_overlap_fraction) + [int(device_id)]
    if allocator is not None:
        _check(L.gwamd_get_overlaps_with_allocator(*args, allocator._handle, C.byref(p), C.byref(n)))
    else:
        _check(L.gwamd_get_overlaps(*args, C.byref(p), C.byref(n)))
    return _take_overlaps(L, p, n)


def match_overlaps(query_index, target_index, min_residues=20, min_overlap_len=50, min_bases_per_residue=50,
                   min_overlap_fraction=0.9, max_anchors=None, allocator=None, return_num_anchors=False):
    """get_overlaps(match_anchors(query_index, target_index)) with the anchors
    staying on the device (main.cu:227-240).  With return_num_anchors the
    result is (overlaps, number of anchors)."""
    L = load_library()
    if not query_index._handle or not target_index._handle:
        raise ValueError("index is closed")
    cap = -1 if max_anchors is None else int(max_anchors)
    if cap < 0 and max_anchors is not None:
        raise ValueError("max_anchors must not be negative")
    p, n, na = C.c_void_p(), C.c_int64(), C.c_int64()
    args = [query_index._handle, target_index._handle, cap] + \
        _filter_args(min_residues, min_overlap_len, min_bases_per_residue, min_overlap_fraction)
    if allocator is not None:
        _check(L.gwamd_match_overlaps_with_allocator(*args, allocator._handle, C.byref(p), C.byref(n), C.byref(na)))
    else:
        _check(L.gwamd_match_overlaps(*args, C.byref(p), C.byref(n), C.byref(na)))
    overlaps = _take_overlaps(L, p, n)
    return (overlaps, na.value) if return_num_anchors else overlaps


def post_process_overlaps(overlaps, drop_fused_overlaps=False):
    """Overlapper::post_process_overlaps (overlapper.cpp:127-228) on the host:
    the overlaps (without those that were fused, with drop_fused_overlaps)
    followed by the fusion of every run of mergeable neighbours."""
    L = load_library()
    arr = _overlap_array(overlaps)
    p, n = C.c_void_p(), C.c_int64()
    _check(L.gwamd_post_process_overlaps(arr, len(overlaps), int(bool(drop_fused_overlaps)), C.byref(p), C.byref(n)))
    return _take_overlaps(L, p, n)


def rescue_overlap_ends(overlaps, query_reads, target_reads, extension=100, required_similarity=0.9, device_id=0,
                        allocator=None):
    """Overlaps with their ends pushed out towards the read ends
    (Overlapper::rescue_overlap_ends, overlapper.cpp:295-365) on the GPU, one
    wave per overlap: three rounds of extend_overlap_by_sequence_similarity, a
    Reverse overlap against the reverse complement of its target.

    query_reads / target_reads: sequences indexed by the overlaps' read ids;
    one object given for both is uploaded once.  Unlike the reference, which
    runs every round with 100 and 0.9 whatever it is given, extension (0..128)
    and required_similarity are honoured.  Returns a new list of Overlap.
    ValueError for a read id or a position beyond its read, a strand other
    than '+' and '-', an extension out of range and a NaN similarity."""
    L = load_library()
    qb, qo = _pack(query_reads)
    tb, to = (qb, qo) if target_reads is query_reads else _pack(target_reads)
    arr = _overlap_array(overlaps)
    p, n = C.c_void_p(), C.c_int64()
    args = [qb, qo, len(query_reads), tb, to, len(target_reads), arr, len(overlaps), int(extension),
            float(required_similarity), int(device_id)]
    if allocator is not None:
        _check(L.gwamd_rescue_overlap_ends_with_allocator(*args, allocator._handle, C.byref(p), C.byref(n)))
    else:
        _check(L.gwamd_rescue_overlap_ends(*args, C.byref(p), C.byref(n)))
    return _take_overlaps(L, p, n)


def extend_overlap_by_sequence_similarity(overlap, query, target, extension, required_similarity):
    """One round of end rescue on one overlap, on the host
    (details::overlapper::extend_overlap_by_sequence_similarity,
    overlapper.cpp:254-293): a copy of the overlap with each end moved out by
    min(extension, room on both reads) bases where the windows there are at
    least required_similarity similar.  The strand is not looked at."""
    L = load_library()
    o = _copy(overlap if isinstance(overlap, Overlap) else Overlap(*overlap))
    q = query.encode() if isinstance(query, str) else bytes(query)
    t = target.encode() if isinstance(target, str) else bytes(target)
    _check(L.gwamd_extend_overlap_by_sequence_similarity(C.byref(o), q, len(q), t, len(t), int(extension),
                                                         float(required_similarity)))
    return o
