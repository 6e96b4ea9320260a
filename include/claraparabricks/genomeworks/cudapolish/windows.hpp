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
// Overlaps that already carry CIGARs (cudamapper -a, align_overlaps, minimap2
// -c) are cut from their runs by window_segments_cigar, without an alignment
// and without expanding a run; read_paf reads them from PAF text.
//
// add_poa_group_resident adds a window to a cudapoa batch as slices of reads
// that are already on the device (cudamapper::DeviceReads), with base qualities
// as weights when the reads carry them; the grouping into slices, racon's
// mean-quality filter and its coverage trimming are in the C ABI
// (gwamd_build_window_slices, gwamd_trim_consensus, include/gwamd_polish.h).
//
// window_slices_resident is the cut and the grouping in one call with the
// records left on the device, build_window_slices_device the grouping alone on
// given segments, add_poa_groups_resident many windows per call.
//
// Not done here: positional (sub-graph) alignment of a segment within its
// window, a native driver for the whole pipeline, a command-line polisher.
#pragma once

#include <claraparabricks/genomeworks/cudaaligner/cudaaligner.hpp>
#include <claraparabricks/genomeworks/cudamapper/device_reads.hpp>
#include <claraparabricks/genomeworks/cudamapper/types.hpp>
#include <claraparabricks/genomeworks/cudapoa/batch.hpp>
#include <claraparabricks/genomeworks/io/fasta_parser.hpp>
#include <claraparabricks/genomeworks/utils/allocator.hpp>

#include <cstdint>
#include <string>
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

/// What I and D mean in a CIGAR and how a Reverse overlap is laid out
/// (GWAMD_CIGAR_*, include/gwamd_polish.h)
enum class CigarConvention : int32_t
{
    genomeworks = 0, ///< align_overlaps, cudamapper -a: I advances only the target, D only the query;
                     ///< Reverse: query forward, target region reverse-complemented
    sam         = 1  ///< minimap2 PAF, SAM: I advances only the query, D only the target;
                     ///< Reverse: target forward, query region reverse-complemented
};

/// CIGAR text such as 12M3I4D5=1X as words length << 4 | op (BAM numbering).
/// Throws std::invalid_argument for a letter without a number, an unknown
/// letter, a length of 2^28 or more and digits at the end.
std::vector<uint32_t> cigar_ops(const std::string& text);

/// window_segments for overlaps that carry CIGARs (cigars[i]: the ops of
/// overlap i): the records of the state paths the CIGARs stand for, cut by one
/// kernel launch over the runs, none of them expanded.  An op other than M, I,
/// D, = and X, and advances that are not the overlap's two spans, make the
/// overlap's records bad_path.
std::vector<WindowSegment> window_segments_cigar(DefaultDeviceAllocator allocator,
                                                 const std::vector<cudamapper::Overlap>& overlaps,
                                                 const std::vector<std::vector<uint32_t>>& cigars,
                                                 int32_t window_length,
                                                 CigarConvention convention = CigarConvention::genomeworks);

/// The same walk over the runs of one overlap on the host
std::vector<WindowSegment> window_segments_cigar_host(const cudamapper::Overlap& overlap,
                                                      const std::vector<uint32_t>& cigar, int32_t window_length,
                                                      CigarConvention convention = CigarConvention::genomeworks,
                                                      uint32_t overlap_index                                    = 0);

/// Overlaps and the ops of their cg:Z: tags (none for a line without one) read
/// from PAF text, as gwamd_read_paf reads it: read ids by name among the
/// parsers' reads, num_residues = column 10 / kmer_size.
struct PafOverlaps
{
    std::vector<cudamapper::Overlap> overlaps;
    std::vector<std::vector<uint32_t>> cigars;
};
PafOverlaps read_paf(const std::string& text, const io::FastaParser& query_parser,
                     const io::FastaParser& target_parser, int32_t kmer_size = 1);

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

/// gwamd_read_slice: bases [begin, end) of read `read` of sets[set],
/// reverse-complemented (A<->T, C<->G, every position) when flags & reverse
struct ReadSlice
{
    enum Flags : uint32_t
    {
        reverse = 1
    };
    int32_t set;
    uint32_t read;
    uint32_t begin;
    uint32_t end;
    uint32_t flags;
};

/// Batch::add_poa_group for sequences that are slices of reads resident on the
/// batch's device: the same group status, per_seq_status, capacity and window
/// order as adding the same sequences from the host, and no base crosses the
/// bus.  generate_poa() writes the bases into the batch's input on the device
/// and, as base weights, quality - 33 of a set created with qualities
/// (reversed, not complemented, for a reverse slice) and 1 of a set without.
/// Host-added and resident groups may be mixed in one batch.  `batch` comes
/// from cudapoa::create_batch.  The read sets must outlive the batch's use of
/// them: until Batch::reset() or the batch's destruction after the last
/// generate_poa() that uses them has completed.  Throws std::invalid_argument,
/// before any device call and with the batch unchanged, for a null set, a set
/// index or read id out of range, begin > end or end beyond the read, and a
/// set on another device than the batch.
cudapoa::StatusType add_poa_group_resident(cudapoa::Batch& batch, std::vector<cudapoa::StatusType>& per_seq_status,
                                           const std::vector<const cudamapper::DeviceReads*>& sets,
                                           const std::vector<ReadSlice>& slices);

/// The windows of every target as slices of the targets (set 0: the backbone,
/// first in its window) and the queries (set 1), window after window: the
/// arrays of gwamd_window_slices_view (include/gwamd_polish.h)
struct WindowSlices
{
    std::vector<ReadSlice> slices;         ///< per sequence
    std::vector<int32_t> window_counts;    ///< sequences per window
    std::vector<read_id_t> window_target;  ///< per window
    std::vector<uint32_t> window_index;    ///< per window: k
    std::vector<int32_t> sequence_overlap; ///< per sequence, -1 for a backbone
    std::vector<int32_t> sequence_t_begin; ///< relative to the window's first base
    std::vector<int32_t> sequence_t_end;
    std::int64_t dropped_by_cap     = 0;
    std::int64_t dropped_by_quality = 0;
};

/// The grouping of build_windows without the bases, done by kernels on the
/// current device (gwamd_build_window_slices_device): `segments` go up, the
/// arrays above come back.  With query_reads that carry qualities a segment
/// whose mean quality - 33 is below quality_threshold_tenths / 10 is dropped
/// before the cap is looked at (racon's rule), its characters read where they
/// are resident.  Device arrays are counted against the allocator's pool.
WindowSlices build_window_slices_device(DefaultDeviceAllocator allocator, const io::FastaParser& targets,
                                        const io::FastaParser& queries,
                                        const std::vector<cudamapper::Overlap>& overlaps,
                                        const std::vector<WindowSegment>& segments, int32_t window_length,
                                        int32_t max_sequences_per_window                  = 100,
                                        const cudamapper::DeviceReads* query_reads        = nullptr,
                                        int32_t quality_threshold_tenths                  = 100);

/// Cut, then group, on the device (gwamd_window_slices_resident): the overlaps
/// are aligned on the resident reads and cut from the aligners' device paths,
/// or, with `cigars` (one per overlap, in `convention`), cut from their runs;
/// the records stay on the device and only the arrays above come back.
WindowSlices window_slices_resident(const std::vector<cudamapper::Overlap>& overlaps,
                                    const cudamapper::DeviceReads& query_reads,
                                    const cudamapper::DeviceReads& target_reads, int32_t window_length,
                                    int32_t max_sequences_per_window = 100, int32_t quality_threshold_tenths = 100,
                                    int32_t num_alignment_engines                    = 1,
                                    const std::vector<std::vector<uint32_t>>* cigars = nullptr,
                                    CigarConvention convention                       = CigarConvention::genomeworks);

/// add_poa_group_resident for many groups in one call: group g is the next
/// group_counts[g] of `slices`.  Equivalent to adding them one by one, in order,
/// up to the first the batch answers exceeded_maximum_poas for; returns the
/// number of groups before that one.  group_status receives one status per
/// group added and per_seq_status one per slice of those groups.  Every slice is
/// checked before the first group is added.
int32_t add_poa_groups_resident(cudapoa::Batch& batch, std::vector<cudapoa::StatusType>& group_status,
                                std::vector<cudapoa::StatusType>& per_seq_status,
                                const std::vector<const cudamapper::DeviceReads*>& sets,
                                const std::vector<ReadSlice>& slices, const std::vector<int32_t>& group_counts);

} // namespace cudapolish
} // namespace genomeworks
} // namespace claraparabricks

namespace claragenomics = claraparabricks::genomeworks;
