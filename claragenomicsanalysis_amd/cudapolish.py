"""cudapolish: the step between cudamapper and cudapoa in a racon-style
polisher, over the C ABI of include/gwamd_polish.h.

window_segments cuts aligned overlaps at the target's window boundaries on the
GPU (racon's find_breaking_points), window_segments_resident aligns the
overlaps on resident reads and cuts them where the aligner leaves its paths on
the device, build_windows groups the pieces into POA windows, and polish runs
targets + reads + overlaps -> polished targets end to end.

Overlaps that already carry CIGARs (cudamapper.align_overlaps, cudamapper -a,
minimap2 -c through cudamapper.read_paf) need no second alignment:
window_segments_cigar cuts them from their runs on the GPU, in the
"genomeworks" or the "sam" convention, without expanding a run to states, and
polish(..., cigars=) takes that route.  cigar_ops turns CIGAR text into the
packed ops (length << 4 | op, BAM numbering) the cut works on.

Path states are AlignmentState values, start -> end: 0 match and 1 mismatch
advance both sequences, 3 (deletion) advances ONLY THE QUERY and 2 (insertion)
ONLY THE TARGET, the reference's convention and the opposite of SAM's I / D.

With device_windows (or qualities) polish names the window sequences as
slices of the reads already resident on the GPU (build_window_slices,
CudaPoaBatch.add_poa_group_resident): no window base is copied on the host or
sent to the device a second time, and base qualities become POA weights on the
device.  Segments of low mean quality are dropped as racon drops them, and
trim_consensus is racon's coverage trimming of a window's consensus ends.

With device_grouping the cut records stay on the device as well:
window_slices_resident cuts and groups them there and returns the windows as a
WindowSlices of flat numpy arrays, build_window_slices_device is that grouping
alone on given segments, and CudaPoaBatch.add_poa_groups_resident adds many
windows per call.

Not done: positional (sub-graph) alignment of a segment within its window, a
native driver for the whole pipeline, a command-line polisher.
"""
import ctypes as C

import numpy as np

from ._lib import load_library
from .cudamapper import DeviceReads, _check, _handles, _overlap_array, _pack

REVERSE, EMPTY, BAD_PATH, NOT_ALIGNED = 1, 2, 4, 8

# gwamd_window_segment
SEGMENT_DTYPE = np.dtype([(n, np.uint32) for n in ("overlap", "window", "q_begin", "q_end", "t_begin", "t_end",
                                                   "flags", "reserved")])


# gwamd_read_slice
SLICE_DTYPE = np.dtype([("set", np.int32), ("read", np.uint32), ("begin", np.uint32), ("end", np.uint32),
                        ("flags", np.uint32)])
SLICE_REVERSE = 1


class _WindowSlicesView(C.Structure):
    """gwamd_window_slices_view."""
    _fields_ = [("num_windows", C.c_int64), ("num_sequences", C.c_int64), ("dropped_by_cap", C.c_int64),
                ("dropped_by_quality", C.c_int64), ("slices", C.c_void_p), ("window_counts", C.c_void_p),
                ("window_target", C.c_void_p), ("window_index", C.c_void_p), ("sequence_overlap", C.c_void_p),
                ("sequence_t_begin", C.c_void_p), ("sequence_t_end", C.c_void_p)]


class _WindowsView(C.Structure):
    """gwamd_windows_view."""
    _fields_ = [("num_windows", C.c_int64), ("num_sequences", C.c_int64), ("num_bases", C.c_int64),
                ("dropped_by_cap", C.c_int64), ("bases", C.c_void_p), ("sequence_offsets", C.c_void_p),
                ("window_counts", C.c_void_p), ("window_target", C.c_void_p), ("window_index", C.c_void_p),
                ("sequence_overlap", C.c_void_p), ("sequence_t_begin", C.c_void_p), ("sequence_t_end", C.c_void_p)]


class _PafView(C.Structure):
    """gwamd_paf_view."""
    _fields_ = [("num_overlaps", C.c_int64), ("num_ops", C.c_int64), ("overlaps", C.c_void_p), ("ops", C.c_void_p),
                ("op_offsets", C.c_void_p)]


def _declare(L):
    vp, i32, i64, u32 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32
    P = C.POINTER
    L.gwamd_window_segments.restype = i32
    L.gwamd_window_segments.argtypes = [vp, i64, vp, vp, i32, i32, vp, P(vp), P(i64)]
    L.gwamd_window_segments_host.restype = i32
    L.gwamd_window_segments_host.argtypes = [vp, vp, i64, i32, u32, P(vp), P(i64)]
    L.gwamd_window_segments_resident.restype = i32
    L.gwamd_window_segments_resident.argtypes = [vp, vp, vp, i32, i32, i32, P(vp), P(i64)]
    L.gwamd_window_segments_cigar.restype = i32
    L.gwamd_window_segments_cigar.argtypes = [vp, i64, vp, vp, i32, i32, i32, vp, P(vp), P(i64)]
    L.gwamd_window_segments_cigar_host.restype = i32
    L.gwamd_window_segments_cigar_host.argtypes = [vp, vp, i64, i32, i32, u32, P(vp), P(i64)]
    L.gwamd_cigar_ops.restype = i32
    L.gwamd_cigar_ops.argtypes = [C.c_char_p, i64, vp, i64, P(i64)]
    L.gwamd_read_paf.restype = i32
    L.gwamd_read_paf.argtypes = [C.c_char_p, C.c_char_p, i64, C.c_char_p, vp, i32, C.c_char_p, vp, i32, i32, P(vp)]
    L.gwamd_paf_get.restype = i32
    L.gwamd_paf_get.argtypes = [vp, P(_PafView)]
    L.gwamd_paf_free.restype = None
    L.gwamd_paf_free.argtypes = [vp]
    L.gwamd_window_segments_free.restype = None
    L.gwamd_window_segments_free.argtypes = [vp]
    L.gwamd_internal_window_segments_strided.restype = i32
    L.gwamd_internal_window_segments_strided.argtypes = [vp, i64, vp, vp, i64, i32, P(vp), P(i64)]
    L.gwamd_build_windows.restype = i32
    L.gwamd_build_windows.argtypes = [C.c_char_p, vp, i32, C.c_char_p, vp, i32, vp, i64, vp, i64, i32, i32, P(vp)]
    L.gwamd_windows_get.restype = i32
    L.gwamd_windows_get.argtypes = [vp, P(_WindowsView)]
    L.gwamd_windows_free.restype = None
    L.gwamd_windows_free.argtypes = [vp]
    L.gwamd_build_window_slices.restype = i32
    L.gwamd_build_window_slices.argtypes = [vp, i32, vp, i32, C.c_char_p, i32, vp, i64, vp, i64, i32, i32, P(vp)]
    L.gwamd_build_window_slices_device.restype = i32
    L.gwamd_build_window_slices_device.argtypes = [vp, i32, vp, i32, vp, i32, vp, i64, vp, i64, i32, i32, i32, vp,
                                                   P(vp)]
    L.gwamd_window_slices_resident.restype = i32
    L.gwamd_window_slices_resident.argtypes = [vp, vp, vp, i32, vp, vp, i32, i32, i32, i32, i32, P(vp)]
    L.gwamd_poa_add_poa_groups_resident.restype = i32
    L.gwamd_poa_add_poa_groups_resident.argtypes = [vp, vp, i32, vp, vp, i32, vp, vp, P(i32)]
    L.gwamd_window_slices_get.restype = i32
    L.gwamd_window_slices_get.argtypes = [vp, P(_WindowSlicesView)]
    L.gwamd_window_slices_free.restype = None
    L.gwamd_window_slices_free.argtypes = [vp]
    L.gwamd_trim_consensus.restype = i32
    L.gwamd_trim_consensus.argtypes = [vp, i32, i32, P(i32), P(i32)]
    L.gwamd_poa_add_poa_group_resident.restype = i32
    L.gwamd_poa_add_poa_group_resident.argtypes = [vp, vp, i32, vp, i32, P(i32)]
    L.gwamd_internal_poa_download_inputs.restype = i32
    L.gwamd_internal_poa_download_inputs.argtypes = [vp, vp, vp]


def _take_segments(L, p, n):
    try:
        out = np.empty(n.value, SEGMENT_DTYPE)
        if n.value:
            C.memmove(out.ctypes.data, p, n.value * SEGMENT_DTYPE.itemsize)
        return out
    finally:
        L.gwamd_window_segments_free(p)


_STATE_OF = {"m": 0, "mm": 1, "i": 2, "d": 3}  # the names CudaAlignment.alignment uses


def _states(path):
    return np.asarray([_STATE_OF[s] if isinstance(s, str) else s for s in path], dtype=np.int64).astype(np.int8)


def _pack_paths(paths):
    offsets = np.zeros(len(paths) + 1, np.int64)
    for i, p in enumerate(paths):
        offsets[i + 1] = offsets[i] + len(p)
    states = np.zeros(max(int(offsets[-1]), 1), np.int8)
    for i, p in enumerate(paths):
        if len(p):
            states[offsets[i]:offsets[i + 1]] = _states(p)
    return states, offsets


def window_segments(overlaps, paths, window_length, device_id=0, allocator=None):
    """The records (a SEGMENT_DTYPE array) of every overlap, in overlap order:
    overlap i owns those of windows target_start // w .. (target_end - 1) // w.

    paths[i]: the AlignmentState values of overlap i, start -> end (or their
    names "m", "mm", "i", "d" as CudaAlignment.alignment has them).  One kernel
    launch; allocator: a cudaaligner.DeviceAllocator whose pool the device
    arrays are counted against during the call.  ValueError for window_length
    <= 0, an overlap with start > end, a path longer than the two spans
    together and more than 2^31 records."""
    L = load_library()
    if len(paths) != len(overlaps):
        raise ValueError("one path per overlap expected")
    arr = _overlap_array(overlaps)
    states, offsets = _pack_paths(paths)
    p, n = C.c_void_p(), C.c_int64()
    _check(L.gwamd_window_segments(arr, len(overlaps), states.ctypes.data_as(C.c_void_p),
                                   offsets.ctypes.data_as(C.c_void_p), int(window_length), int(device_id),
                                   allocator._handle if allocator is not None else None, C.byref(p), C.byref(n)))
    return _take_segments(L, p, n)


def window_segments_host(overlap, path, window_length, overlap_index=0):
    """The same walk for one overlap on the host, without a GPU."""
    L = load_library()
    arr = _overlap_array([overlap])
    states = _states(list(path) + [0])
    p, n = C.c_void_p(), C.c_int64()
    _check(L.gwamd_window_segments_host(arr, states.ctypes.data_as(C.c_void_p), len(path), int(window_length),
                                        int(overlap_index), C.byref(p), C.byref(n)))
    return _take_segments(L, p, n)


def window_segments_resident(overlaps, query_reads, target_reads, window_length, num_alignment_engines=1):
    """The overlaps aligned as cudamapper.align_overlaps aligns them on two
    DeviceReads, and cut on the device from the aligner's own path buffer: only
    the overlaps go up and the records come back.  An overlap beyond the
    aligner's limits gets NOT_ALIGNED records."""
    L = load_library()
    handles = _handles(query_reads, target_reads)
    if not handles:
        raise TypeError("query_reads and target_reads must be DeviceReads")
    arr = _overlap_array(overlaps)
    p, n = C.c_void_p(), C.c_int64()
    _check(L.gwamd_window_segments_resident(*handles, arr, len(overlaps), int(window_length),
                                            int(num_alignment_engines), C.byref(p), C.byref(n)))
    return _take_segments(L, p, n)


CIGAR_CONVENTIONS = {"genomeworks": 0, "sam": 1}  # GWAMD_CIGAR_*
CIGAR_LETTERS = "MIDNSHP=X"  # BAM numbering; the cut takes M, I, D, = and X


def cigar_ops(text):
    """CIGAR text such as "12M3I4D5=1X" as a np.uint32 array of length << 4 |
    op (M 0, I 1, D 2, = 7, X 8; lengths below 2^28).  ValueError for a letter
    without a number, an unknown letter, a length of 2^28 or more and digits
    at the end; "" gives no op."""
    L = load_library()
    data = text.encode() if isinstance(text, str) else bytes(text)
    out = np.zeros(len(data) // 2 + 1, np.uint32)
    n = C.c_int64()
    _check(L.gwamd_cigar_ops(data, len(data), out.ctypes.data_as(C.c_void_p), len(out), C.byref(n)))
    return out[:n.value]


def _convention(name):
    if name not in CIGAR_CONVENTIONS:
        raise ValueError("convention must be one of %s, got %r" % (sorted(CIGAR_CONVENTIONS), name))
    return CIGAR_CONVENTIONS[name]


def _ops(cigar):
    if isinstance(cigar, (str, bytes)):
        return cigar_ops(cigar)
    return np.ascontiguousarray(cigar, dtype=np.uint32)


def _pack_cigars(cigars):
    """(ops, offsets) of CIGARs given as text or as op arrays."""
    if cigars and all(isinstance(c, str) for c in cigars):
        # The texts joined are one CIGAR text whose ops are theirs in order, provided that none ends in
        # digits: one call parses them all, and the letters counted up to each text's end are its ops.
        data = "".join(cigars).encode()
        buf = np.frombuffer(data, np.uint8)
        ends = np.cumsum([len(c) for c in cigars])
        letters = np.concatenate([[0], np.cumsum((buf < 48) | (buf > 57))])
        last = buf[np.maximum(ends - 1, 0)] if len(buf) else np.zeros(len(ends), np.uint8)
        ops = np.zeros(int(letters[-1]) + 1, np.uint32)
        n = C.c_int64()
        if not np.any((last >= 48) & (last <= 57) & (np.diff(ends, prepend=0) > 0)) and \
                load_library().gwamd_cigar_ops(data, len(data), ops.ctypes.data_as(C.c_void_p), len(ops) - 1,
                                               C.byref(n)) == 0 and n.value == len(ops) - 1:
            offsets = np.zeros(len(cigars) + 1, np.int64)
            offsets[1:] = letters[ends]
            return ops, offsets
        # a malformed text: parsed one by one below, which names it
    arrays = [_ops(c) for c in cigars]
    offsets = np.zeros(len(arrays) + 1, np.int64)
    if arrays:
        np.cumsum([len(a) for a in arrays], out=offsets[1:])
    ops = np.concatenate(arrays + [np.zeros(1, np.uint32)])
    return ops, offsets


def window_segments_cigar(overlaps, cigars, window_length, convention="genomeworks", device_id=0, allocator=None):
    """window_segments for overlaps that carry CIGARs: the records of the
    state paths the CIGARs stand for, cut by one kernel launch over the runs
    (no run is expanded, only the ops go up).

    cigars[i]: the CIGAR of overlap i, as text or as ops (cigar_ops).
    convention: "genomeworks" for what align_overlaps and cudamapper -a emit (I
    advances only the target, D only the query; a '-' overlap runs along the
    query and the reverse-complemented target region), "sam" for minimap2's
    PAF and SAM (I only the query, D only the target; '-' runs along the target
    and the reverse-complemented query region).  An op other than M, I, D, =
    and X, and advances that are not the overlap's two spans, give BAD_PATH
    records; ValueError as window_segments, and for an unknown convention."""
    L = load_library()
    if len(cigars) != len(overlaps):
        raise ValueError("one CIGAR per overlap expected")
    code = _convention(convention)
    arr = _overlap_array(overlaps)
    ops, offsets = _pack_cigars(cigars)
    p, n = C.c_void_p(), C.c_int64()
    _check(L.gwamd_window_segments_cigar(arr, len(overlaps), ops.ctypes.data_as(C.c_void_p),
                                         offsets.ctypes.data_as(C.c_void_p), code, int(window_length),
                                         int(device_id), allocator._handle if allocator is not None else None,
                                         C.byref(p), C.byref(n)))
    return _take_segments(L, p, n)


def window_segments_cigar_host(overlap, cigar, window_length, convention="genomeworks", overlap_index=0):
    """The same walk over the runs of one overlap on the host, without a GPU."""
    L = load_library()
    code = _convention(convention)
    arr = _overlap_array([overlap])
    ops = np.concatenate([_ops(cigar), np.zeros(1, np.uint32)])
    p, n = C.c_void_p(), C.c_int64()
    _check(L.gwamd_window_segments_cigar_host(arr, ops.ctypes.data_as(C.c_void_p), len(ops) - 1, code,
                                              int(window_length), int(overlap_index), C.byref(p), C.byref(n)))
    return _take_segments(L, p, n)


def _read_paf(path_or_text, query_names, target_names, kmer_size):
    """cudamapper.read_paf: (overlaps, cigars) over gwamd_read_paf."""
    import os

    from .cudamapper import Overlap
    L = load_library()
    qn, qno = _pack(query_names)
    tn, tno = _pack(target_names)
    text = path_or_text.encode() if isinstance(path_or_text, str) else bytes(path_or_text)
    # PAF text has tabs or is empty; anything else names a file
    is_text = not text or b"\t" in text or b"\n" in text
    if isinstance(path_or_text, os.PathLike):
        text, is_text = os.fsencode(path_or_text), False
    h = C.c_void_p()
    _check(L.gwamd_read_paf(None if is_text else text, text if is_text else None, len(text) if is_text else 0,
                            qn, qno, len(query_names), tn, tno, len(target_names), int(kmer_size), C.byref(h)))
    try:
        v = _PafView()
        _check(L.gwamd_paf_get(h, C.byref(v)))
        raw = _array(v.overlaps, v.num_overlaps * C.sizeof(Overlap), np.uint8).tobytes()
        overlaps = [Overlap.from_buffer_copy(raw, i * C.sizeof(Overlap)) for i in range(v.num_overlaps)]
        ops = _array(v.ops, v.num_ops, np.uint32)
        offsets = _array(v.op_offsets, v.num_overlaps + 1, np.int64)
        cigars = [ops[offsets[i]:offsets[i + 1]].copy() for i in range(v.num_overlaps)]
        return overlaps, cigars
    finally:
        L.gwamd_paf_free(h)


def _window_segments_strided(overlaps, paths, path_lengths, stride, window_length):
    """Test hook: the cut of paths laid out as the aligner leaves them, end ->
    start, path i at paths[i * stride:]; paths is a bytes-like of n * stride."""
    L = load_library()
    arr = _overlap_array(overlaps)
    buf = np.frombuffer(bytes(paths) + b"\0", np.int8).copy()
    lens = np.asarray(list(path_lengths) + [0], dtype=np.int32)
    p, n = C.c_void_p(), C.c_int64()
    _check(L.gwamd_internal_window_segments_strided(arr, len(overlaps), buf.ctypes.data_as(C.c_void_p),
                                                    lens.ctypes.data_as(C.c_void_p), int(stride), int(window_length),
                                                    C.byref(p), C.byref(n)))
    return _take_segments(L, p, n)


def build_windows(targets, queries, overlaps, segments, window_length, max_sequences_per_window=100):
    """(windows, dropped): one window per window_length bases of every target,
    in target then window order, each a dict of "target", "window", "sequences"
    (the backbone first) and per sequence "overlap" (-1: backbone), "t_begin"
    and "t_end" relative to the window's first base.  A segment is kept when it
    is not flagged and (q_end - q_begin) * 50 >= window_length; a REVERSE one
    is reverse-complemented; at most max_sequences_per_window - 1 per window,
    and dropped counts what that cap left out.  Host only."""
    L = load_library()
    tb, to = _pack(targets)
    qb, qo = _pack(queries)
    arr = _overlap_array(overlaps)
    segs = np.ascontiguousarray(segments, dtype=SEGMENT_DTYPE)
    h = C.c_void_p()
    _check(L.gwamd_build_windows(tb, to, len(targets), qb, qo, len(queries), arr, len(overlaps),
                                 segs.ctypes.data_as(C.c_void_p), len(segs), int(window_length),
                                 int(max_sequences_per_window), C.byref(h)))
    try:
        v = _WindowsView()
        _check(L.gwamd_windows_get(h, C.byref(v)))

        bases = C.string_at(v.bases, v.num_bases).decode("latin-1") if v.num_bases else ""
        off = _array(v.sequence_offsets, v.num_sequences + 1, np.int64)
        counts = _array(v.window_counts, v.num_windows, np.int32)
        target = _array(v.window_target, v.num_windows, np.uint32)
        index = _array(v.window_index, v.num_windows, np.uint32)
        overlap = _array(v.sequence_overlap, v.num_sequences, np.int32)
        t_begin = _array(v.sequence_t_begin, v.num_sequences, np.int32)
        t_end = _array(v.sequence_t_end, v.num_sequences, np.int32)
        windows, s = [], 0
        for i in range(v.num_windows):
            c = int(counts[i])
            windows.append({"target": int(target[i]), "window": int(index[i]),
                            "sequences": [bases[off[j]:off[j + 1]] for j in range(s, s + c)],
                            "overlap": overlap[s:s + c].tolist(), "t_begin": t_begin[s:s + c].tolist(),
                            "t_end": t_end[s:s + c].tolist()})
            s += c
        return windows, int(v.dropped_by_cap)
    finally:
        L.gwamd_windows_free(h)


def _array(address, count, dtype):
    if not count:
        return np.zeros(0, dtype)
    return np.frombuffer(C.string_at(address, count * np.dtype(dtype).itemsize), dtype)


def _lengths_offsets(reads):
    offs = (C.c_int64 * (len(reads) + 1))()
    for i, r in enumerate(reads):
        offs[i + 1] = offs[i] + (r if isinstance(r, int) else len(r))
    return offs


def build_window_slices(targets, queries, overlaps, segments, window_length, max_sequences_per_window=100,
                        query_qualities=None, quality_threshold=10.0):
    """(windows, dropped_by_cap, dropped_by_quality): the grouping of
    build_windows without the bases.  Each window is a dict of "target",
    "window", "overlap", "t_begin", "t_end" as build_windows gives them and
    "slices": per sequence (set, read, begin, end, flags) with set 0 the targets
    (the backbone, first) and set 1 the queries, flags & SLICE_REVERSE for a
    reverse-complemented one.  targets / queries: the reads or just their
    lengths.

    query_qualities: one quality string (Phred + 33) per query.  A segment that
    passes the keep rule is then dropped, before the cap, when the mean of
    quality - 33 over its query range is below quality_threshold (racon's
    rule).  The threshold counts in tenths, round(10 * quality_threshold), and
    the test is the integer one: 10 * sum < tenths * length, so a mean equal to
    the threshold keeps the segment.  Host only."""
    L = load_library()
    to, qo = _lengths_offsets(targets), _lengths_offsets(queries)
    quals = None
    if query_qualities is not None:
        if len(query_qualities) != len(queries):
            raise ValueError("%d quality strings for %d queries" % (len(query_qualities), len(queries)))
        for i, q in enumerate(query_qualities):
            if len(q) != qo[i + 1] - qo[i]:
                raise ValueError("query %d has %d quality characters for %d bases" % (i, len(q), qo[i + 1] - qo[i]))
        quals, _ = _pack(query_qualities)
    arr = _overlap_array(overlaps)
    segs = np.ascontiguousarray(segments, dtype=SEGMENT_DTYPE)
    h = C.c_void_p()
    _check(L.gwamd_build_window_slices(to, len(targets), qo, len(queries), quals,
                                       int(round(10 * float(quality_threshold))), arr, len(overlaps),
                                       segs.ctypes.data_as(C.c_void_p), len(segs), int(window_length),
                                       int(max_sequences_per_window), C.byref(h)))
    ws = _take_window_slices(L, h)
    return ws.windows(), ws.dropped_by_cap, ws.dropped_by_quality


class WindowSlices:
    """The windows of every target as flat numpy arrays (gwamd_window_slices_view):
    per sequence, window after window and the backbone first, `slices`
    (SLICE_DTYPE; set 0 the targets, set 1 the queries), `overlap` (-1 for a
    backbone), `t_begin` and `t_end` relative to the window's first base; per
    window `counts` (its sequences), `target` and `index` (k); and the two
    counters dropped_by_cap and dropped_by_quality."""

    def __init__(self, slices, counts, target, index, overlap, t_begin, t_end, dropped_by_cap, dropped_by_quality):
        self.slices, self.counts, self.target, self.index = slices, counts, target, index
        self.overlap, self.t_begin, self.t_end = overlap, t_begin, t_end
        self.dropped_by_cap, self.dropped_by_quality = int(dropped_by_cap), int(dropped_by_quality)

    def __len__(self):
        return len(self.counts)

    def windows(self):
        """The list of dicts build_window_slices returns."""
        slices = self.slices.tolist()  # tuples of ints
        windows, s = [], 0
        for i in range(len(self.counts)):
            c = int(self.counts[i])
            windows.append({"target": int(self.target[i]), "window": int(self.index[i]), "slices": slices[s:s + c],
                            "overlap": self.overlap[s:s + c].tolist(), "t_begin": self.t_begin[s:s + c].tolist(),
                            "t_end": self.t_end[s:s + c].tolist()})
            s += c
        return windows


def _take_window_slices(L, h):
    """The arrays of a gwamd_window_slices handle, copied; the handle is freed."""
    try:
        v = _WindowSlicesView()
        _check(L.gwamd_window_slices_get(h, C.byref(v)))
        return WindowSlices(_array(v.slices, v.num_sequences, SLICE_DTYPE),
                            _array(v.window_counts, v.num_windows, np.int32),
                            _array(v.window_target, v.num_windows, np.uint32),
                            _array(v.window_index, v.num_windows, np.uint32),
                            _array(v.sequence_overlap, v.num_sequences, np.int32),
                            _array(v.sequence_t_begin, v.num_sequences, np.int32),
                            _array(v.sequence_t_end, v.num_sequences, np.int32),
                            v.dropped_by_cap, v.dropped_by_quality)
    finally:
        L.gwamd_window_slices_free(h)


def build_window_slices_device(targets, queries, overlaps, segments, window_length, max_sequences_per_window=100,
                               query_reads=None, quality_threshold=10.0, device_id=0, allocator=None):
    """build_window_slices with the grouping done by kernels on device_id: the
    segments go up, a WindowSlices comes back, equal to the host's in every
    array and both counters.  query_reads: the queries as a DeviceReads; when
    it carries qualities they are read where they are resident and racon's
    mean-quality rule applies as in build_window_slices.  allocator: a
    cudaaligner.DeviceAllocator whose pool the device arrays are counted
    against during the call (RuntimeError when it is too small, with the pool
    as it was).  ValueError, before any device call, for window_length <= 0,
    max_sequences_per_window < 1, a negative threshold and a segment whose
    overlap index, read id, window or query range is out of bounds."""
    L = load_library()
    to, qo = _lengths_offsets(targets), _lengths_offsets(queries)
    handle = None
    if query_reads is not None:
        handle = getattr(query_reads, "_handle", None)
        if not handle:
            raise TypeError("query_reads must be an open DeviceReads")
    arr = _overlap_array(overlaps)
    segs = np.ascontiguousarray(segments, dtype=SEGMENT_DTYPE)
    h = C.c_void_p()
    _check(L.gwamd_build_window_slices_device(to, len(targets), qo, len(queries), handle,
                                              int(round(10 * float(quality_threshold))), arr, len(overlaps),
                                              segs.ctypes.data_as(C.c_void_p), len(segs), int(window_length),
                                              int(max_sequences_per_window), int(device_id),
                                              allocator._handle if allocator is not None else None, C.byref(h)))
    return _take_window_slices(L, h)


def window_slices_resident(overlaps, query_reads, target_reads, window_length, max_sequences_per_window=100,
                           quality_threshold=10.0, num_alignment_engines=1, cigars=None,
                           cigar_convention="genomeworks"):
    """Cut, then group, on the device: what build_window_slices makes of
    window_segments_resident's records (of window_segments_cigar's with
    cigars=, one CIGAR per overlap in cigar_convention), as a WindowSlices,
    without a record on the host: only the overlaps (and the ops) go up and
    only the grouped arrays come back.  The mean-quality rule applies when
    query_reads carries qualities."""
    L = load_library()
    handles = _handles(query_reads, target_reads)
    if not handles:
        raise TypeError("query_reads and target_reads must be DeviceReads")
    arr = _overlap_array(overlaps)
    ops = offsets = None
    code = 0
    if cigars is not None:
        if len(cigars) != len(overlaps):
            raise ValueError("one CIGAR per overlap expected")
        code = _convention(cigar_convention)
        ops_array, offsets_array = _pack_cigars(cigars)
        ops, offsets = ops_array.ctypes.data_as(C.c_void_p), offsets_array.ctypes.data_as(C.c_void_p)
    h = C.c_void_p()
    _check(L.gwamd_window_slices_resident(*handles, arr, len(overlaps), ops, offsets, code, int(window_length),
                                          int(max_sequences_per_window), int(round(10 * float(quality_threshold))),
                                          int(num_alignment_engines), C.byref(h)))
    return _take_window_slices(L, h)


def trim_consensus(consensus, coverage, num_sequences):
    """racon's trimming of a window's consensus by coverage (window.cpp): with
    average = (num_sequences - 1) // 2, num_sequences counting the backbone, the
    consensus from the first to the last index whose coverage is at least
    average, both included.  When no index qualifies, or the first is not before
    the last, the consensus comes back whole (racon warns there).  Host only."""
    L = load_library()
    if len(coverage) != len(consensus):
        raise ValueError("one coverage value per consensus base expected")
    cov = np.ascontiguousarray(list(coverage) + [0], dtype=np.uint16)
    b, e = C.c_int32(), C.c_int32()
    _check(L.gwamd_trim_consensus(cov.ctypes.data_as(C.c_void_p), len(consensus), int(num_sequences), C.byref(b),
                                  C.byref(e)))
    return consensus[b.value:e.value]


_COMPLEMENT = {ord("A"): "T", ord("T"): "A", ord("C"): "G", ord("G"): "C"}


def _slice_text(sets, sl):
    """The bases of a slice, cut from the host strings."""
    text = sets[sl[0]][sl[1]][sl[2]:sl[3]]
    return text[::-1].translate(_COMPLEMENT) if sl[4] & SLICE_REVERSE else text


def _slice_weights(qualities, sl):
    """The weights of a slice: quality - 33 per base, 1 without qualities."""
    if qualities[sl[0]] is None:
        return [1] * (sl[3] - sl[2])
    q = qualities[sl[0]][sl[1]][sl[2]:sl[3]]
    q = q.encode("latin-1") if isinstance(q, str) else bytes(q)
    w = [c - 33 for c in q]
    return w[::-1] if sl[4] & SLICE_REVERSE else w


def polish(targets, queries, overlaps, window_length=500, max_sequences_per_window=100, banded=True,
           band_width=256, scores=(8, -6, -8), num_alignment_engines=1, device_id=0, max_gpu_mem=None,
           return_windows=False, device_windows=False, query_qualities=None, target_qualities=None,
           quality_threshold=10.0, trim=False, cigars=None, cigar_convention="genomeworks", device_grouping=False):
    """Polished targets from targets, reads and overlaps (query = read, target =
    target): the overlaps are aligned and cut on the GPU
    (window_segments_resident), grouped into windows (build_windows) and run
    through CudaPoaBatch.  A window contributes its consensus when it has at
    least three sequences and its POA status is success, its backbone
    otherwise.  scores: (match, mismatch, gap).  max_gpu_mem: the bytes the POA
    batch may take (default: half of the device's free memory); windows beyond
    what it holds at once are processed in rounds.

    device_windows: the windows are named as slices of the two resident read
    sets (build_window_slices) and added with add_poa_group_resident, so the
    POA batch's input is written on the device; the reads stay resident until
    the POA is done.  Same result as the default route.  query_qualities /
    target_qualities: one quality string (Phred + 33) per read; either implies
    device_windows, and the POA then weighs every base of that side with
    quality - 33 (a side without qualities weighs 1).  With query_qualities a
    segment whose mean quality is below quality_threshold is dropped
    (build_window_slices).  trim: every consensus is cut to racon's coverage
    rule (trim_consensus) before it is joined.

    cigars: one CIGAR per overlap (text or ops, in cigar_convention; what
    cudamapper.align_overlaps, cudamapper -a or cudamapper.read_paf give),
    ValueError for another count.  The segments then come from
    window_segments_cigar: the overlaps are not aligned again and no aligner
    is created; everything after the segments is the same.

    device_grouping: implies device_windows.  The cut records stay on the
    device and are grouped there (window_slices_resident): only the grouped
    arrays come back, the windows with at least three sequences are picked and
    sized with numpy on the flat arrays and added with add_poa_groups_resident,
    as many per call as the batch takes.  Per-window lists are built only for
    return_windows.  Same result and stats as device_windows=True.

    Returns (polished, stats); stats counts "windows", "backbone_by_rule"
    (fewer than three sequences), "backbone_by_status", "dropped_by_cap",
    "dropped_by_quality", "trimmed_bases" and carries the "max_sequence_size"
    the POA batch was made for.  With return_windows the windows and each one's
    consensus (None for a backbone by rule; as the POA gave it, untrimmed) and
    status are appended to the result; on the device route a window also
    carries its "slices" and "weights", and its "sequences" are cut from the
    host strings."""
    from .cudapoa import CudaPoaBatch
    import torch

    targets = [t[1] if isinstance(t, tuple) else t for t in targets]
    queries = [q[1] if isinstance(q, tuple) else q for q in queries]
    resident = bool(device_windows) or bool(device_grouping) or query_qualities is not None or \
        target_qualities is not None
    if cigars is not None:
        if len(cigars) != len(overlaps):
            raise ValueError("%d CIGARs for %d overlaps" % (len(cigars), len(overlaps)))
        _convention(cigar_convention)
    with torch.cuda.device(device_id):
        q_reads = DeviceReads(queries, device_id=device_id, qualities=query_qualities)
        try:
            t_reads = DeviceReads(targets, device_id=device_id, qualities=target_qualities)
        except Exception:
            q_reads.close()
            raise
    try:
        with torch.cuda.device(device_id):
            if device_grouping:
                grouped = window_slices_resident(overlaps, q_reads, t_reads, window_length, max_sequences_per_window,
                                                 quality_threshold, num_alignment_engines, cigars, cigar_convention)
            elif cigars is not None:
                segments = window_segments_cigar(overlaps, cigars, window_length, cigar_convention, device_id)
            else:
                segments = window_segments_resident(overlaps, q_reads, t_reads, window_length, num_alignment_engines)
        by_quality = 0
        if device_grouping:
            # everything below works on the flat arrays; per-window lists only for return_windows
            dropped, by_quality = grouped.dropped_by_cap, grouped.dropped_by_quality
            first = np.concatenate([[0], np.cumsum(grouped.counts, dtype=np.int64)])
            seq_len = grouped.slices["end"].astype(np.int64) - grouped.slices["begin"]
            backbone = [_slice_text((targets, queries), sl) for sl in grouped.slices[first[:-1]].tolist()]
            windows = None
            if return_windows:
                windows = grouped.windows()
                for w in windows:
                    w["sequences"] = [_slice_text((targets, queries), sl) for sl in w["slices"]]
                    w["weights"] = [_slice_weights((target_qualities, query_qualities), sl) for sl in w["slices"]]
            num_seqs, window_target = grouped.counts.tolist(), grouped.target.tolist()
            todo = np.nonzero(grouped.counts >= 3)[0]
            in_todo = np.repeat(grouped.counts >= 3, grouped.counts)
            longest = max(int(seq_len[in_todo].max()), 1) if len(todo) else 1
            todo_slices, todo_counts = grouped.slices[in_todo], grouped.counts[todo]
            todo_first = np.concatenate([[0], np.cumsum(todo_counts, dtype=np.int64)])
            todo = todo.tolist()
        elif resident:
            windows, dropped, by_quality = build_window_slices(
                targets, queries, overlaps, segments, window_length, max_sequences_per_window,
                query_qualities=query_qualities, quality_threshold=quality_threshold)
            backbone = [_slice_text((targets, queries), w["slices"][0]) for w in windows]
            lengths = [[sl[3] - sl[2] for sl in w["slices"]] for w in windows]
            if return_windows:
                for w in windows:
                    w["sequences"] = [_slice_text((targets, queries), sl) for sl in w["slices"]]
                    w["weights"] = [_slice_weights((target_qualities, query_qualities), sl) for sl in w["slices"]]
        else:
            q_reads.close()
            t_reads.close()
            windows, dropped = build_windows(targets, queries, overlaps, segments, window_length,
                                             max_sequences_per_window)
            backbone = [w["sequences"][0] for w in windows]
            lengths = [[len(s) for s in w["sequences"]] for w in windows]
        if not device_grouping:
            num_seqs, window_target = [len(n) for n in lengths], [w["target"] for w in windows]
            todo = [i for i, n in enumerate(num_seqs) if n >= 3]
            longest = max([n for i in todo for n in lengths[i]] + [1])
        stats = {"windows": len(num_seqs), "backbone_by_rule": 0, "backbone_by_status": 0, "dropped_by_cap": dropped,
                 "dropped_by_quality": by_quality, "trimmed_bases": 0}
        stats["backbone_by_rule"] = len(num_seqs) - len(todo)
        # a sequence must be shorter than the batch's limit; sizes in steps of 64
        max_sequence_size = (longest + 1 + 63) // 64 * 64
        stats["max_sequence_size"] = max_sequence_size
        consensus = [None] * len(num_seqs)
        coverage = [None] * len(num_seqs)
        status = [None] * len(num_seqs)
        if todo:
            if max_gpu_mem is None:
                max_gpu_mem = int(0.5 * torch.cuda.mem_get_info(device_id)[0])
            batch = CudaPoaBatch(max_sequences_per_window, max_sequence_size, int(max_gpu_mem), device_id=device_id,
                                 gap_score=scores[2], mismatch_score=scores[1], match_score=scores[0],
                                 cuda_banded_alignment=banded, alignment_band_width=band_width)
            held = []

            def add(i):
                if resident:
                    return batch.add_poa_group_resident([t_reads, q_reads], windows[i]["slices"])[0]
                return batch.add_poa_group(windows[i]["sequences"])[0]

            def flush():
                if not held:
                    return
                batch.generate_poa()
                cons, cov, st = batch.get_consensus()
                for j, i in enumerate(held):
                    consensus[i], coverage[i], status[i] = cons[j], cov[j], st[j]
                batch.reset()
                del held[:]

            def add_many(at):
                """As many of todo[at:] as the batch takes, in one call; the index of the first it did not take."""
                added, group_status, _ = batch.add_poa_groups_resident([t_reads, q_reads],
                                                                       todo_slices[todo_first[at]:], todo_counts[at:])
                for i, st in zip(todo[at:at + added], group_status):
                    if st != 0:
                        status[i] = st
                    else:
                        held.append(i)
                return at + added

            if device_grouping:
                at = 0
                while at < len(todo):
                    took = add_many(at)
                    if took < len(todo):  # exceeded_maximum_poas
                        if took == at and not held:  # an empty batch does not hold it either
                            status[todo[took]] = 1
                            took += 1
                        flush()
                    at = took
            else:
                for i in todo:
                    st = add(i)
                    if st == 1:  # exceeded_maximum_poas: process what the batch holds, then add again
                        flush()
                        st = add(i)
                    if st != 0:
                        status[i] = st
                        continue
                    held.append(i)
            flush()
            del batch
    finally:
        q_reads.close()
        t_reads.close()
    polished = ["" for _ in targets]
    for i, target in enumerate(window_target):
        text = backbone[i]
        if consensus[i] is not None and status[i] == 0:
            text = consensus[i]
            if trim:
                text = trim_consensus(text, coverage[i], num_seqs[i])
                stats["trimmed_bases"] += len(consensus[i]) - len(text)
        elif num_seqs[i] >= 3:
            stats["backbone_by_status"] += 1
        polished[target] += text
    if return_windows:
        return polished, stats, windows, consensus, status
    return polished, stats
