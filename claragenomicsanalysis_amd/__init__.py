"""MI355X-native batched POA consensus/MSA, global alignment and cudamapper's
minimizer index, anchor matcher, overlapper, overlap-end rescue, index
batches and reads resident on the device, and cudapolish: aligned overlaps cut
into POA windows on the GPU, from reads and overlaps to a polished target.

Python mirror of the reference's pygenomeworks bindings (genomeworks.cudapoa,
genomeworks.cudaaligner) over the C ABI of libgwamd.so (include/*.h).  All
compute runs in hand-written HIP kernels for gfx950; there is no CPU fallback.
"""
from ._lib import load_library, library_path  # noqa: F401
from .cudamapper import (Index, match_anchors, get_overlaps, match_overlaps, post_process_overlaps,  # noqa: F401
                         rescue_overlap_ends, extend_overlap_by_sequence_similarity, DeviceReads,
                         group_reads_into_indices, generate_batches_of_indices, IndexHostCopy, read_paf)
from .cudapolish import (window_segments, window_segments_host, window_segments_resident,  # noqa: F401
                         window_segments_cigar, window_segments_cigar_host, cigar_ops,
                         build_windows, build_window_slices, trim_consensus, polish)

__all__ = ["load_library", "library_path", "Index", "match_anchors", "get_overlaps", "match_overlaps",
           "post_process_overlaps", "rescue_overlap_ends", "extend_overlap_by_sequence_similarity",
           "DeviceReads", "group_reads_into_indices", "generate_batches_of_indices",
           "IndexHostCopy", "window_segments", "window_segments_host", "window_segments_resident",
           "window_segments_cigar", "window_segments_cigar_host", "cigar_ops", "read_paf", "build_windows", "build_window_slices", "trim_consensus", "polish"]
