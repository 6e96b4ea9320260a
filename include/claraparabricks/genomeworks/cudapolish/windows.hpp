// cudapolish: the step between cudamapper and cudapoa in a racon-style
// polisher.  Aligned overlaps are cut at the target's window boundaries on the
// GPU (racon's find_breaking_points) and the pieces grouped into cudapoa
// groups, one per window of every target.  The reference has no such module;
// racon does this step on the host.
//
// Path states are cudaaligner::AlignmentState values, start -> end: match and
// mismatch advance both sequences, deletion (3) advances ONLY THE QUERY and
// insertion (2) ONLY THE TARGET (alignment_impl.cpp:94-103), the opposite of
// SAM's I / D.  The semantics of a record are in include/gwamd_polish.h.
//
// Not done here: quality weights, racon's coverage trimming of consensus ends,
// positional (sub-graph) alignment of a segment within its window.
#pragma once

#include <claraparabricks/genomeworks/cudaaligner/cudaaligner.hpp>
#include <claraparabricks/genomeworks/cudamapper/device_reads.hpp>
#include <claraparabricks/genomeworks/cudamapper/types.hpp>
#include <claraparabricks/genomeworks/cudapoa/batch.hpp>
#include <claraparabricks/genomeworks/io/fasta_parser.hpp>
#include <claraparabricks/genomeworks/utils/allocator.hpp>

#include <cstdint>
#include <vector>

namespace claraparabricks
{
namespace genomeworks
{
namespace cudapolish
{

/// gwamd_window_segment: the piece of one overlap in one target window
struct WindowSegment
{
    enum Flags : uint32_t
    {
        reverse     = 1, ///< the overlap is on the Reverse strand
        empty       = 2, ///< no match or mismatch state in the window
        bad_path    = 4, ///< the path does not fit the overlap
        not_aligned = 8  ///< the overlap is beyond the aligner's limits
    };
    uint32_t overlap; ///< index into the overlaps of the call
    uint32_t window;  ///< k: target positions [k w, (k + 1) w)
    uint32_t q_begin;
    uint32_t q_end;
    uint32_t t_begin;
    uint32_t t_end;
    uint32_t flags;
    uint32_t reserved;
};

/// The records of every overlap, in overlap order: overlap i owns those of
/// windows target_start / w .. (target_end - 1) / w.  paths[i] are the states
/// of overlap i, start -> end.  One kernel launch on the current device; the
/// device arrays are counted against the allocator's pool during the call.
/// Throws std::invalid_argument for window_length <= 0, an overlap with start >
/// end, a path longer than the two spans together and more than 2^31 records.
std::vector<WindowSegment> window_segments(DefaultDeviceAllocator allocator,
                                           const std::vector<cudamapper::Overlap>& overlaps,
                                           const std::vector<std::vector<cudaaligner::AlignmentState>>& paths,
                                           int32_t window_length);

/// The overlaps aligned as cudamapper::align_overlaps aligns them on resident
/// reads, and cut where each aligner leaves its paths on the device: no path
/// and no CIGAR crosses the bus.  An overlap beyond the aligner's limits gets
/// not_aligned records (and align_overlaps' warning).
std::vector<WindowSegment> window_segments(DefaultDeviceAllocator allocator,
                                           const std::vector<cudamapper::Overlap>& overlaps,
                                           const cudamapper::DeviceReads& query_reads,
                                           const cudamapper::DeviceReads& target_reads, int32_t window_length,
                                           int32_t num_alignment_engines);

/// One cudapoa group per window of every target, in target then window order.
struct Windows
{
    struct Sequence
    {
        int32_t overlap; ///< -1 for the backbone
        int32_t t_begin; ///< relative to the window's first base
        int32_t t_end;
    };
    std::vector<cudapoa::Group> groups;          ///< entries point into bases
    std::vector<read_id_t> target;               ///< per group
    std::vector<uint32_t> window;                ///< per group: k
    std::vector<std::vector<Sequence>> sequence; ///< per group, per entry
    std::int64_t dropped_by_cap = 0;             ///< kept segments the cap left out
    std::vector<char> bases;

    Windows()               = default;
    Windows(Windows&&)      = default;
    Windows& operator=(Windows&&) = default;
    Windows(const Windows&) = delete;
    Windows& operator=(const Windows&) = delete;
};

/// Host only.  The backbone target[k w, min((k + 1) w, T)) is the first entry of
/// its group.  A segment is kept when it is not flagged empty, bad_path or
/// not_aligned and (q_end - q_begin) * 50 >= window_length (racon's 2 % rule);
/// kept segments are appended in the order given, a reverse one
/// reverse-complemented (A<->T, C<->G, every position), at most
/// max_sequences_per_window - 1 per group.
Windows build_windows(const io::FastaParser& targets, const io::FastaParser& queries,
                      const std::vector<cudamapper::Overlap>& overlaps, const std::vector<WindowSegment>& segments,
                      int32_t window_length, int32_t max_sequences_per_window = 100);

} // namespace cudapolish
} // namespace genomeworks
} // namespace claraparabricks

namespace claragenomics = claraparabricks::genomeworks;
