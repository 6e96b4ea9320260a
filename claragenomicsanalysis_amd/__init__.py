"""MI355X-native batched POA consensus/MSA, global alignment and cudamapper's
minimizer index, anchor matcher, overlapper and overlap-end rescue.

Python mirror of the reference's pygenomeworks bindings (genomeworks.cudapoa,
genomeworks.cudaaligner) over the C ABI of libgwamd.so (include/*.h).  All
compute runs in hand-written HIP kernels for gfx950; there is no CPU fallback.
"""
from ._lib import load_library, library_path  # noqa: F401
from .cudamapper import (Index, match_anchors, get_overlaps, match_overlaps, post_process_overlaps,  # noqa: F401
                         rescue_overlap_ends, extend_overlap_by_sequence_similarity)

__all__ = ["load_library", "library_path", "Index", "match_anchors", "get_overlaps", "match_overlaps",
           "post_process_overlaps", "rescue_overlap_ends", "extend_overlap_by_sequence_similarity"]
