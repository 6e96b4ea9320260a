// Overlapper of cudamapper on the MI355X (reference
// cudamapper/include/claraparabricks/genomeworks/cudamapper/overlapper.hpp:60-107).
// get_overlaps, post_process_overlaps, rescue_overlap_ends and
// details::overlapper::extend_overlap_by_sequence_similarity are provided;
// filter_overlaps is declared but never defined in the reference.
//
// One divergence in the rescue: the reference complements a Reverse overlap's
// target through a 26-entry table indexed by (byte - 'A') (overlapper.cpp:94-109),
// which is undefined for a byte outside 'A'..'Z'; here such a byte is left as
// it is, like every letter other than A, C, G and T.
#pragma once

#include <claraparabricks/genomeworks/cudamapper/device_reads.hpp>
#include <claraparabricks/genomeworks/cudamapper/types.hpp>
#include <claraparabricks/genomeworks/io/fasta_parser.hpp>
#include <claraparabricks/genomeworks/types.hpp>
#include <claraparabricks/genomeworks/utils/device_buffer.hpp>

#include <cstdint>
#include <vector>

namespace claraparabricks
{
namespace genomeworks
{
namespace cudamapper
{

namespace details
{
namespace overlapper
{

/// One round of end rescue on the host (overlapper.cpp:254-293).  The head
/// window is the min(query start, target start, extension) bases before the
/// overlap on both reads, the tail window the min(extension, bases left on
/// either read) after it.  An end moves out by its whole window when the
/// windows' similarity is at least required_similarity, both float32.  The
/// similarity is the multiset Jaccard index of the windows' substrings
/// s[i, min(L, 2i + 15)), i = 0 .. L - 15, as the reference cuts them
/// (cudamapper_utils.cpp:114-170); a window shorter than 15 is one string, so
/// two empty windows are similar.  The positions must lie within the sequences.
void extend_overlap_by_sequence_similarity(Overlap& overlap, gw_string_view_t& query_sequence,
                                           gw_string_view_t& target_sequence, std::int32_t extension,
                                           float required_similarity);

} // namespace overlapper
} // namespace details

class Overlapper
{
public:
    virtual ~Overlapper() = default;

    /// Overlaps of anchors sorted by (query_read_id, target_read_id,
    /// query_position_in_read, target_position_in_read), in anchor order.
    /// An overlap is kept when it chains at least min_residues anchors, spans
    /// at least min_overlap_len bases on both reads and fewer than
    /// min_bases_per_residue bases per anchor, joins two different reads, and
    /// its shorter span is more than min_overlap_fraction of its longer one.
    /// Throws std::invalid_argument for a negative or NaN parameter, unsorted
    /// anchors or a position of 2^31 or more.
    virtual void get_overlaps(std::vector<Overlap>& fused_overlaps, const device_buffer<Anchor>& d_anchors,
                              int64_t min_residues, int64_t min_overlap_len, int64_t min_bases_per_residue,
                              float min_overlap_fraction) = 0;

    /// Appends the fusion of every run of neighbouring overlaps that can be
    /// merged (same reads and strand, and gaps that are short, of similar size
    /// or short beside the overlaps); drop_fused_overlaps removes the overlaps
    /// that went into a fusion.
    static void post_process_overlaps(std::vector<Overlap>& overlaps, bool drop_fused_overlaps = false);

    /// Pushes the ends of every overlap out towards the read ends, in place and
    /// on the GPU (the current device): three rounds of
    /// extend_overlap_by_sequence_similarity per overlap, a Reverse overlap
    /// against the reverse complement of its target.  As in the reference
    /// (overlapper.cpp:345) every round runs with an extension of 100 and a
    /// required similarity of 0.9f: the two arguments are ignored.
    /// Throws std::invalid_argument for a read id beyond its parser, a position
    /// beyond its read or a strand that is neither Forward nor Reverse.
    static void rescue_overlap_ends(std::vector<Overlap>& overlaps, const io::FastaParser& query_parser,
                                    const io::FastaParser& target_parser, std::int32_t extension,
                                    float required_similarity);

    /// The same on reads that are resident on the current device
    /// (device_reads.hpp): only the overlaps are uploaded.  Unlike the parser
    /// overload this one honours extension (0..128) and required_similarity.
    /// The same object may stand on both sides.  Throws std::invalid_argument
    /// also for an extension out of range, a NaN similarity and reads on
    /// another device than the current one.
    static void rescue_overlap_ends(std::vector<Overlap>& overlaps, const DeviceReads& query_reads,
                                    const DeviceReads& target_reads, std::int32_t extension,
                                    float required_similarity);
};

} // namespace cudamapper
} // namespace genomeworks
} // namespace claraparabricks

namespace claragenomics = claraparabricks::genomeworks;
