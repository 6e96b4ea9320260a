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
DeviceReads puts a read set on the device once; rescue_overlap_ends and
align_overlaps take it in place of the sequences.  group_reads_into_indices,
generate_batches_of_indices and IndexHostCopy are the building blocks of the
cudamapper tool's loop over index pairs (csrc/cudamapper_main.cpp).

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
    L.gwamd_read_fasta_with_qualities.restype = i32
    L.gwamd_read_fasta_with_qualities.argtypes = [C.c_char_p, C.c_uint32, i32, P(vp), P(vp), P(vp)]
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
    L.gwamd_group_reads_into_indices.restype = i32
    L.gwamd_group_reads_into_indices.argtypes = [vp, i32, i64, P(vp), P(i64)]
    L.gwamd_index_descriptors_free.restype = None
    L.gwamd_index_descriptors_free.argtypes = [vp]
    L.gwamd_index_descriptor_hash.restype = C.c_uint64
    L.gwamd_index_descriptor_hash.argtypes = [C.c_uint32, C.c_uint32]
    L.gwamd_generate_batches_of_indices.restype = i32
    L.gwamd_generate_batches_of_indices.argtypes = [i32, i32, i32, i32, vp, i32, vp, i32, i64, i64, i32, P(vp), P(i64)]
    L.gwamd_batches_of_indices_free.restype = None
    L.gwamd_batches_of_indices_free.argtypes = [vp]
    L.gwamd_index_host_copy_create.restype = i32
    L.gwamd_index_host_copy_create.argtypes = [vp, C.c_uint32, i32, i32, P(vp)]
    L.gwamd_index_host_copy_to_device.restype = i32
    L.gwamd_index_host_copy_to_device.argtypes = [vp, i32, vp, P(vp)]
    L.gwamd_index_host_copy_info.restype = i32
    L.gwamd_index_host_copy_info.argtypes = [vp, P(IndexInfo), P(C.c_uint32), P(i32), P(i32)]
    L.gwamd_index_host_copy_free.restype = None
    L.gwamd_index_host_copy_free.argtypes = [vp]
    L.gwamd_device_reads_create.restype = i32
    L.gwamd_device_reads_create.argtypes = [C.c_char_p, vp, i32, i32, vp, P(vp)]
    L.gwamd_device_reads_create_with_qualities.restype = i32
    L.gwamd_device_reads_create_with_qualities.argtypes = [C.c_char_p, C.c_char_p, vp, i32, i32, vp, P(vp)]
    L.gwamd_device_reads_has_qualities.restype = i32
    L.gwamd_device_reads_has_qualities.argtypes = [vp]
    L.gwamd_device_reads_free.restype = None
    L.gwamd_device_reads_free.argtypes = [vp]
    L.gwamd_device_reads_info.restype = i32
    L.gwamd_device_reads_info.argtypes = [vp, P(i64), P(i64), P(i32)]
    L.gwamd_rescue_overlap_ends_resident.restype = i32
    L.gwamd_rescue_overlap_ends_resident.argtypes = [vp, vp, vp, i64, i32, C.c_float, vp, P(vp), P(i64)]
    L.gwamd_align_overlaps_resident.restype = i32
    L.gwamd_align_overlaps_resident.argtypes = [vp, vp, vp, i32, i32, P(vp)]
    L.gwamd_internal_gather_overlap_regions.restype = i32
    L.gwamd_internal_gather_overlap_regions.argtypes = [vp, vp, vp, i64, i64, vp, vp]
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


class DeviceReads:
    """A read set resident on one device (gwamd_device_reads): the packed bases
    and the offsets, uploaded once.  rescue_overlap_ends and align_overlaps take
    one per side in place of the sequences and then move only the overlaps.

    reads: sequences (str or bytes), or (name, sequence) records as read_fasta
    returns them.  qualities: one quality string (str or bytes, Phred + 33)
    per read, each of its read's length, kept in a second device array of the
    same layout for CudaPoaBatch.add_poa_group_resident's base weights;
    ValueError, before any device call, for another count or length and for a
    character outside 33..126.  allocator: a cudaaligner.DeviceAllocator whose
    pool the device bytes are counted against until close()."""

    def __init__(self, reads, device_id=0, allocator=None, qualities=None):
        self._lib = load_library()
        self._handle = C.c_void_p()
        seqs = [r[1] if isinstance(r, tuple) else r for r in reads]
        bases, offsets = _pack(seqs)
        pool = allocator._handle if allocator is not None else None
        if qualities is None:
            _check(self._lib.gwamd_device_reads_create(bases, offsets, len(seqs), int(device_id), pool,
                                                       C.byref(self._handle)))
        else:
            qualities = list(qualities)
            if len(qualities) != len(seqs):
                raise ValueError("%d quality strings for %d reads" % (len(qualities), len(seqs)))
            for i, (q, r) in enumerate(zip(qualities, seqs)):
                if len(q) != len(r):
                    raise ValueError("read %d has %d quality characters for %d bases" % (i, len(q), len(r)))
            quals, _ = _pack(qualities)
            _check(self._lib.gwamd_device_reads_create_with_qualities(bases, quals, offsets, len(seqs),
                                                                      int(device_id), pool, C.byref(self._handle)))
        self._allocator = allocator  # the handle holds bytes of its pool
        n, b, d = C.c_int64(), C.c_int64(), C.c_int32()
        _check(self._lib.gwamd_device_reads_info(self._handle, C.byref(n), C.byref(b), C.byref(d)))
        self.number_of_reads, self.number_of_basepairs, self.device_id = n.value, b.value, d.value
        self.has_qualities = bool(_check(self._lib.gwamd_device_reads_has_qualities(self._handle)))

    def __len__(self):
        return self.number_of_reads

    def close(self):
        """Frees the device memory."""
        h, self._handle = self._handle, C.c_void_p()
        if h:
            self._lib.gwamd_device_reads_free(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _handles(query_reads, target_reads):
    """The two handles when both sides are DeviceReads, None when neither is."""
    resident = [isinstance(r, DeviceReads) for r in (query_reads, target_reads)]
    if not any(resident):
        return None
    if not all(resident):
        raise TypeError("query_reads and target_reads must both be DeviceReads, or neither")
    if not query_reads._handle or not target_reads._handle:
        raise ValueError("DeviceReads is closed")
    return query_reads._handle, target_reads._handle


def gather_overlap_regions(overlaps, query_reads, target_reads, stride):
    """Test hook: gather_overlap_regions_kernel on two DeviceReads.  Returns
    (seqs, lens): 2 n stride bytes with overlap i's query region at 2 i stride
    and its target region (reverse-complemented for '-') at (2 i + 1) stride,
    and the 2 n lengths.  The hook clears the device buffer before the launch
    and the kernel writes nothing outside a region, so the bytes of a slot past
    its region's length are zero."""
    L = load_library()
    q, t = _handles(query_reads, target_reads)
    arr = _overlap_array(overlaps)
    n = len(overlaps)
    seqs = np.zeros(max(2 * n * max(int(stride), 0), 1), np.uint8)
    lens = np.zeros(max(2 * n, 1), np.int32)
    _check(L.gwamd_internal_gather_overlap_regions(q, t, arr, n, int(stride), seqs.ctypes.data_as(C.c_void_p),
                                                   lens.ctypes.data_as(C.c_void_p)))
    return seqs[:2 * n * int(stride)].tobytes(), lens[:2 * n].tolist()


def align_overlaps(overlaps, query_reads, target_reads, num_alignment_engines=1, device_id=0):
    """CIGAR of every overlap (align_overlaps, main.cu:125-175).

    query_reads / target_reads: sequences indexed by the overlaps' read ids, or
    two DeviceReads on the current device (device_id is then not looked at):
    the regions are gathered into the aligner on the device."""
    L = load_library()
    handles = _handles(query_reads, target_reads)
    if handles:
        arr = _overlap_array(overlaps)
        h = C.c_void_p()
        _check(L.gwamd_align_overlaps_resident(*handles, arr, len(overlaps), num_alignment_engines, C.byref(h)))
        return _take(L, h)
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


def read_paf(path_or_text, query_names, target_names, kmer_size=1):
    """(overlaps, cigars) of a PAF file, or of PAF text (anything with a tab or
    a newline in it), the way back from format_paf and the input of
    cudapolish.polish(..., cigars=): one Overlap per non-empty line, its read
    ids the indices of columns 1 and 6 in query_names / target_names,
    num_residues column 10 // kmer_size, and per overlap the ops of its cg:Z:
    tag as a np.uint32 array (cudapolish.cigar_ops; empty without the tag).
    ValueError, with the line's number, for an unknown name, fewer than 12
    columns, a strand other than + and -, start > end and an end beyond the
    read's length in column 2 or 7."""
    from .cudapolish import _read_paf
    return _read_paf(path_or_text, query_names, target_names, kmer_size)


def read_fasta(path, min_sequence_length=0, shuffle=True):
    """(name, sequence) records as io::create_kseq_fasta_parser holds them
    (kseqpp_fasta_parser.cpp:31-72): shorter records dropped, shuffled with
    std::mt19937(0) unless shuffle is False."""
    L = load_library()
    n, s = C.c_void_p(), C.c_void_p()
    _check(L.gwamd_read_fasta(str(path).encode(), int(min_sequence_length), int(bool(shuffle)), C.byref(n),
                              C.byref(s)))
    return list(zip(_take(L, n), _take(L, s)))


def read_fasta_with_qualities(path, min_sequence_length=0, shuffle=True):
    """(records, qualities): read_fasta's records and each one's quality
    string, of its sequence's length for a FASTQ record and "" for a FASTA one."""
    L = load_library()
    n, s, q = C.c_void_p(), C.c_void_p(), C.c_void_p()
    _check(L.gwamd_read_fasta_with_qualities(str(path).encode(), int(min_sequence_length), int(bool(shuffle)),
                                             C.byref(n), C.byref(s), C.byref(q)))
    return list(zip(_take(L, n), _take(L, s))), _take(L, q)


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
        self._download()

    @classmethod
    def _from_handle(cls, handle, allocator=None):
        """An Index around a gwamd_index the library made (IndexHostCopy.copy_index_to_device)."""
        self = cls.__new__(cls)
        self._lib = load_library()
        self._handle = handle
        self._allocator = allocator
        self._download()
        return self

    def _download(self):
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
    one object given for both is uploaded once.  Two DeviceReads on the current
    device (device_id is then not looked at) are read where they lie.  Unlike the reference, which
    runs every round with 100 and 0.9 whatever it is given, extension (0..128)
    and required_similarity are honoured.  Returns a new list of Overlap.
    ValueError for a read id or a position beyond its read, a strand other
    than '+' and '-', an extension out of range and a NaN similarity."""
    L = load_library()
    handles = _handles(query_reads, target_reads)
    arr = _overlap_array(overlaps)
    p, n = C.c_void_p(), C.c_int64()
    if handles:
        _check(L.gwamd_rescue_overlap_ends_resident(*handles, arr, len(overlaps), int(extension),
                                                    float(required_similarity),
                                                    allocator._handle if allocator is not None else None,
                                                    C.byref(p), C.byref(n)))
        return _take_overlaps(L, p, n)
    qb, qo = _pack(query_reads)
    tb, to = (qb, qo) if target_reads is query_reads else _pack(target_reads)
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


def _lengths(reads):
    """A C array of the lengths of reads: sequences, (name, sequence) records or lengths."""
    values = [r if isinstance(r, int) else len(r[1] if isinstance(r, tuple) else r) for r in reads]
    return (C.c_int64 * max(len(values), 1))(*values), len(values)


def index_descriptor_hash(first_read, number_of_reads):
    """IndexDescriptor::get_hash (index_descriptor.cpp:43-59)."""
    return int(load_library().gwamd_index_descriptor_hash(int(first_read), int(number_of_reads)))


def group_reads_into_indices(reads, max_basepairs_per_index=1000000):
    """(first_read, number_of_reads) of the indices the reads are cut into
    (group_reads_into_indices, index_descriptor.cpp:76-109): consecutive reads
    while their basepairs stay within the limit.  reads: sequences, (name,
    sequence) records or lengths.  As in the reference the first descriptor is
    (0, 0) when read 0 alone is over the limit."""
    L = load_library()
    arr, n = _lengths(reads)
    p, count = C.c_void_p(), C.c_int64()
    _check(L.gwamd_group_reads_into_indices(arr, n, int(max_basepairs_per_index), C.byref(p), C.byref(count)))
    try:
        flat = (C.c_uint32 * (2 * count.value)).from_address(p.value) if count.value else []
        return [(flat[2 * i], flat[2 * i + 1]) for i in range(count.value)]
    finally:
        L.gwamd_index_descriptors_free(p)


def generate_batches_of_indices(query_indices_per_host_batch, query_indices_per_device_batch,
                                target_indices_per_host_batch, target_indices_per_device_batch, query_reads,
                                target_reads, query_basepairs_per_index, target_basepairs_per_index,
                                same_query_and_target):
    """generate_batches_of_indices (index_batcher.cu:24-88).  Returns a list of
    host batches, each a dict of "query" and "target" (lists of (first_read,
    number_of_reads)) and "device_batches" (a list of such dicts without
    device batches).  One parser on both sides is one object given for
    query_reads and target_reads.  ValueError for the four mismatches under
    same_query_and_target and for a number of indices per batch below 1."""
    L = load_library()
    q, nq = _lengths(query_reads)
    t, nt = (q, nq) if target_reads is query_reads else _lengths(target_reads)
    p, count = C.c_void_p(), C.c_int64()
    _check(L.gwamd_generate_batches_of_indices(
        int(query_indices_per_host_batch), int(query_indices_per_device_batch), int(target_indices_per_host_batch),
        int(target_indices_per_device_batch), q, nq, t, nt, int(query_basepairs_per_index),
        int(target_basepairs_per_index), int(bool(same_query_and_target)), C.byref(p), C.byref(count)))
    try:
        flat = list((C.c_int64 * count.value).from_address(p.value))
    finally:
        L.gwamd_batches_of_indices_free(p)
    at = [0]

    def take():
        at[0] += 1
        return flat[at[0] - 1]

    def descriptors():
        return [(take(), take()) for _ in range(take())]

    batches = []
    for _ in range(take()):
        batch = {"query": descriptors(), "target": descriptors()}
        batch["device_batches"] = [{"query": descriptors(), "target": descriptors()} for _ in range(take())]
        batches.append(batch)
    assert at[0] == len(flat)
    return batches


class IndexHostCopy:
    """A copy of an Index in host memory (IndexHostCopyBase::create_cache,
    index.hpp:109-182), from which copy_index_to_device makes an Index again
    without building it: equal to the original in every array and getter."""

    def __init__(self, index, first_read_id, kmer_size, window_size):
        self._lib = load_library()
        self._handle = C.c_void_p()
        if not index._handle:
            raise ValueError("index is closed")
        _check(self._lib.gwamd_index_host_copy_create(index._handle, int(first_read_id), int(kmer_size),
                                                      int(window_size), C.byref(self._handle)))
        info, first, k, w = IndexInfo(), C.c_uint32(), C.c_int32(), C.c_int32()
        _check(self._lib.gwamd_index_host_copy_info(self._handle, C.byref(info), C.byref(first), C.byref(k),
                                                    C.byref(w)))
        self.num_elements = int(info.num_elements)
        self.number_of_reads = int(info.number_of_reads)
        self.number_of_basepairs_in_longest_read = int(info.number_of_basepairs_in_longest_read)
        self.first_read_id, self.kmer_size, self.window_size = first.value, k.value, w.value

    def copy_index_to_device(self, device_id=0, allocator=None):
        if not self._handle:
            raise ValueError("host copy is closed")
        h = C.c_void_p()
        _check(self._lib.gwamd_index_host_copy_to_device(self._handle, int(device_id),
                                                         allocator._handle if allocator is not None else None,
                                                         C.byref(h)))
        return Index._from_handle(h, allocator)

    def close(self):
        h, self._handle = self._handle, C.c_void_p()
        if h:
            self._lib.gwamd_index_host_copy_free(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
