// (k,w)-minimizer index of cudamapper on the MI355X (reference
// cudamapper/include/claraparabricks/genomeworks/cudamapper/index.hpp:33-107).
// Same accessors and create_index arguments; hipStream_t stands where the
// reference has cudaStream_t.
//
// The sketch elements are ordered by (representation, read_id,
// position_in_read).  A read shorter than window_size + kmer_size - 1
// contributes nothing but keeps its id: in the reference a skipped read shifts
// the ids of the reads after it (index_gpu.cuh:720-734, marked TODO there).
#pragma once

#include <claraparabricks/genomeworks/cudamapper/sketch_element.hpp>
#include <claraparabricks/genomeworks/cudamapper/types.hpp>
#include <claraparabricks/genomeworks/io/fasta_parser.hpp>
#include <claraparabricks/genomeworks/utils/allocator.hpp>
#include <claraparabricks/genomeworks/utils/device_buffer.hpp>

#include <hip/hip_runtime_api.h>

#include <climits>
#include <cstdint>
#include <memory>
#include <vector>

namespace claraparabricks
{
namespace genomeworks
{
namespace cudamapper
{

class Index
{
public:
    virtual ~Index() = default;

    /// Representations of the sketch elements.
    virtual const device_buffer<representation_t>& representations() const = 0;
    /// Read ids of the sketch elements.
    virtual const device_buffer<read_id_t>& read_ids() const = 0;
    /// Positions of the sketch elements in their reads.
    virtual const device_buffer<position_in_read_t>& positions_in_reads() const = 0;
    /// Directions in which the sketch elements were read.
    virtual const device_buffer<SketchElement::DirectionOfRepresentation>& directions_of_reads() const = 0;
    /// Every representation once, sorted.
    virtual const device_buffer<representation_t>& unique_representations() const = 0;
    /// First element of each unique representation, plus a last entry equal to
    /// the number of elements (empty for an empty index).
    virtual const device_buffer<std::uint32_t>& first_occurrence_of_representations() const = 0;

    /// past_the_last_read_id - first_read_id, or 0 when no read is long enough.
    virtual read_id_t number_of_reads() const = 0;
    /// Smallest read id of the index (0 for an empty index).
    virtual read_id_t smallest_read_id() const = 0;
    /// Largest read id of the index (0 for an empty index).
    virtual read_id_t largest_read_id() const = 0;
    /// Length of the longest read that went into the index.
    virtual position_in_read_t number_of_basepairs_in_longest_read() const = 0;

    /// Largest k-mer size: 2 bits per base in a representation_t.
    static std::uint64_t maximum_kmer_size() { return sizeof(representation_t) * CHAR_BIT / 2; }

    /// Index of the reads [first_read_id, past_the_last_read_id) of parser, built on the current device.
    /// filtering_parameter < 1.0 removes every representation that makes up at
    /// least that share of all sketch elements.  Device memory is counted
    /// against the allocator's pool.  Throws std::invalid_argument for
    /// arguments out of range (kmer_size in [1, 32], window_size in [1, 255],
    /// filtering_parameter in [0, 1], read ids within the parser).
    static std::unique_ptr<Index> create_index(DefaultDeviceAllocator allocator, const io::FastaParser& parser,
                                               const read_id_t first_read_id, const read_id_t past_the_last_read_id,
                                               const std::uint64_t kmer_size, const std::uint64_t window_size,
                                               const bool hash_representations  = true,
                                               const double filtering_parameter = 1.0, const hipStream_t stream = 0);
};

/// A copy of an Index in host memory, from which the index is put back on a
/// device without being computed again (reference index.hpp:109-182,
/// cudamapper/src/index_host_copy.cu).
class IndexHostCopyBase
{
public:
    virtual ~IndexHostCopyBase() = default;

    /// An Index on the current device with the arrays and the getters of the
    /// index the copy was made from; Matcher::create_matcher accepts it.  The
    /// device bytes are counted against the allocator's pool, as in create_index.
    virtual std::unique_ptr<Index> copy_index_to_device(DefaultDeviceAllocator allocator,
                                                        const hipStream_t stream = 0) const = 0;

    virtual const std::vector<representation_t>& representations() const = 0;
    virtual const std::vector<read_id_t>& read_ids() const = 0;
    virtual const std::vector<position_in_read_t>& positions_in_reads() const = 0;
    virtual const std::vector<SketchElement::DirectionOfRepresentation>& directions_of_reads() const = 0;
    virtual const std::vector<representation_t>& unique_representations() const = 0;
    virtual const std::vector<std::uint32_t>& first_occurrence_of_representations() const = 0;
    virtual read_id_t number_of_reads() const = 0;
    virtual position_in_read_t number_of_basepairs_in_longest_read() const = 0;
    /// the first_read_id given to create_cache
    virtual read_id_t first_read_id() const = 0;
    virtual std::uint64_t kmer_size() const = 0;
    virtual std::uint64_t window_size() const = 0;

    /// Copies the six arrays and the scalars of an index made by
    /// Index::create_index (std::invalid_argument for any other) to the host.
    static std::unique_ptr<IndexHostCopyBase> create_cache(const Index& index, const read_id_t first_read_id,
                                                           const std::uint64_t kmer_size,
                                                           const std::uint64_t window_size,
                                                           const hipStream_t stream = 0);
};

} // namespace cudamapper
} // namespace genomeworks
} // namespace claraparabricks

namespace claragenomics = claraparabricks::genomeworks;
