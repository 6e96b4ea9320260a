// IndexDescriptor and group_reads_into_indices of cudamapper (reference
// cudamapper/src/index_descriptor.hpp:25-87, index_descriptor.cpp:24-109): the
// range of reads one index is built from, and the cut of a parser's reads into
// such ranges by a limit of basepairs.
#pragma once

#include <claraparabricks/genomeworks/io/fasta_parser.hpp>
#include <claraparabricks/genomeworks/types.hpp>

#include <cstddef>
#include <cstdint>
#include <vector>

namespace claraparabricks
{
namespace genomeworks
{
namespace cudamapper
{

/// The reads [first_read, first_read + number_of_reads) of a parser.
class IndexDescriptor
{
public:
    IndexDescriptor(read_id_t first_read, number_of_reads_t number_of_reads)
        : first_read_(first_read)
        , number_of_reads_(number_of_reads)
        , hash_(std::size_t(first_read) | std::size_t(number_of_reads) << 32)
    {
        static_assert(sizeof(std::size_t) == 8, "the hash holds two 32-bit values");
    }
    read_id_t first_read() const { return first_read_; }
    number_of_reads_t number_of_reads() const { return number_of_reads_; }
    /// first_read in the lower 32 bits, number_of_reads in the upper
    std::size_t get_hash() const { return hash_; }

private:
    read_id_t first_read_;
    number_of_reads_t number_of_reads_;
    std::size_t hash_;
};

inline bool operator==(const IndexDescriptor& lhs, const IndexDescriptor& rhs)
{
    return lhs.first_read() == rhs.first_read() && lhs.number_of_reads() == rhs.number_of_reads();
}
inline bool operator!=(const IndexDescriptor& lhs, const IndexDescriptor& rhs) { return !(lhs == rhs); }

struct IndexDescriptorHash
{
    std::size_t operator()(const IndexDescriptor& index_descriptor) const { return index_descriptor.get_hash(); }
};

/// Consecutive reads are put into one index while their basepairs stay within
/// max_basepairs_per_index; a read that is longer gets an index of its own.
/// As in the reference the current index is closed before it is known to hold
/// a read, so the first descriptor is the empty {0, 0} when read 0 alone is
/// over the limit, and a parser without reads gives the one descriptor {0, 0}.
std::vector<IndexDescriptor> group_reads_into_indices(const io::FastaParser& parser,
                                                      number_of_basepairs_t max_basepairs_per_index = 1000000);

} // namespace cudamapper
} // namespace genomeworks
} // namespace claraparabricks

namespace claragenomics = claraparabricks::genomeworks;
