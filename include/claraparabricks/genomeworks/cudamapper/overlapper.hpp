// Overlapper of cudamapper on the MI355X (reference
// cudamapper/include/claraparabricks/genomeworks/cudamapper/overlapper.hpp:60-107).
// get_overlaps and post_process_overlaps are provided; rescue_overlap_ends is
// not, and filter_overlaps is declared but never defined in the reference.
#pragma once

#include <claraparabricks/genomeworks/cudamapper/types.hpp>
#include <claraparabricks/genomeworks/utils/device_buffer.hpp>

#include <cstdint>
#include <vector>

namespace claraparabricks
{
namespace genomeworks
{
namespace cudamapper
{

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
};

} // namespace cudamapper
} // namespace genomeworks
} // namespace claraparabricks

namespace claragenomics = claraparabricks::genomeworks;
