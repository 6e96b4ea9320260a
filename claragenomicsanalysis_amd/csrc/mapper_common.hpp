// Host-side declarations shared by the minimizer index, the matcher, the
// overlapper and the end rescue (mapper_index.hip, mapper_match.hip, mapper_overlap.hip,
// mapper_rescue.hip, mapper_batch.cpp, mapper_rescue_host.cpp).  Reads resident
// on the device and the gather of overlap regions: mapper_reads.hpp.
#pragma once

#include "host_common.hpp"

#include <cstdint>
#include <memory>
#include <utility>
#include <vector>

namespace gwamd
{
namespace mapper
{

using gwamd::host::Budget;
using gwamd::host::DevBuf;

constexpr int kMaxKmerSize   = 32;  // 2 bits per base in a 64-bit representation
constexpr int kMaxWindowSize = 255; // bounds the halo a sketch tile stages in LDS
constexpr int64_t kDefaultMaxAnchors = int64_t(1) << 31;

// cudamapper::Anchor (types.hpp), four u32
struct AnchorRecord
{
    uint32_t query_read_id;
    uint32_t target_read_id;
    uint32_t query_position_in_read;
    uint32_t target_position_in_read;
};

// The six device arrays of an index, ordered by (representation, read_id,
// position_in_read), and its scalars.
struct IndexData
{
    DevBuf<uint64_t> representations;
    DevBuf<uint32_t> read_ids;
    DevBuf<uint32_t> positions_in_reads;
    DevBuf<uint8_t> directions_of_reads;
    DevBuf<uint64_t> unique_representations;
    DevBuf<uint32_t> first_occurrence_of_representations;
    uint32_t number_of_reads                     = 0;
    uint32_t smallest_read_id                    = 0;
    uint32_t largest_read_id                     = 0;
    uint32_t number_of_basepairs_in_longest_read = 0;
    int device_id                                = 0;
};

// Index of the reads [first_read_id, first_read_id + num_reads): read i of the
// range is bases[offsets[i], offsets[i + 1]) (host memory, offsets has
// num_reads + 1 entries).  Arguments are validated by the caller.
void build_index(IndexData& out, const char* bases, const int64_t* offsets, uint32_t first_read_id, uint32_t num_reads,
                 int kmer_size, int window_size, bool hash_representations, double filtering_parameter,
                 const Budget& budget, hipStream_t stream);

// All (query element, target element) pairs of equal representation, sorted by
// (query_read_id, target_read_id, query_position, target_position).  Throws
// std::runtime_error when there are more than max_anchors.
void match_anchors(DevBuf<AnchorRecord>& out, const IndexData& query, const IndexData& target, int64_t max_anchors,
                   const Budget& budget, hipStream_t stream);

// cudamapper::Overlap (types.hpp), nine 32-bit words: the strand character and
// overlap_complete each sit in the low byte of a word of their own
struct OverlapRecord
{
    uint32_t query_read_id;
    uint32_t target_read_id;
    uint32_t query_start;
    uint32_t target_start;
    uint32_t query_end;
    uint32_t target_end;
    uint8_t relative_strand;
    uint32_t num_residues;
    uint8_t overlap_complete;
};
static_assert(sizeof(OverlapRecord) == 36, "OverlapRecord is nine 32-bit words");

// The filter of OverlapperTriggered::get_overlaps; none of the integers is negative.
struct OverlapParams
{
    int64_t min_residues          = 20;
    int64_t min_overlap_len       = 50;
    int64_t min_bases_per_residue = 50;
    float min_overlap_fraction    = 0.9f;
};

// What each level of the overlapper left
struct OverlapCounts
{
    int64_t chains = 0, kept_chains = 0, groups = 0, overlaps = 0;
};

constexpr int kOverlapTile = 2048; // anchors per workgroup of the chain-flag kernel (mapper_overlap.hip)

// Overlaps of n device anchors sorted by (query_read_id, target_read_id,
// query_position, target_position), in anchor order (host memory).  Throws
// std::invalid_argument when an adjacent pair is out of order or a position is
// 2^31 or more; the parameters are validated by the caller.
void get_overlaps(std::vector<OverlapRecord>& out, const AnchorRecord* anchors, int64_t n, const OverlapParams& params,
                  const Budget& budget, hipStream_t stream, OverlapCounts* counts = nullptr);

constexpr int kMaxRescueExtension = 128; // bytes of one window in LDS (mapper_rescue.hip)
constexpr int kRescueRounds       = 3;   // max_rescue_rounds, overlapper.cpp:336
constexpr int kRescueKmer         = 15;  // the kmer_size extend_overlap_by_sequence_similarity passes

// The reads of one side in host memory: read i is bases[offsets[i], offsets[i + 1])
struct ReadSet
{
    const char* bases      = nullptr;
    const int64_t* offsets = nullptr; // num_reads + 1 entries
    int64_t num_reads      = 0;
};

// Overlapper::rescue_overlap_ends on n > 0 host overlaps, in place: kRescueRounds
// rounds of extend_overlap_by_sequence_similarity(extension, required_similarity)
// per overlap.  Two sides with the same pointers are uploaded once.  Arguments
// are validated by the caller: ids, positions and the extension are in range.
void rescue_overlap_ends(OverlapRecord* overlaps, int64_t n, const ReadSet& query, const ReadSet& target,
                         int extension, float required_similarity, const Budget& budget, hipStream_t stream);

} // namespace mapper
} // namespace gwamd
