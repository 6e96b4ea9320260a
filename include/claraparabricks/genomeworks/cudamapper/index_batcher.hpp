// Batches of indices of cudamapper (reference cudamapper/src/index_batcher.cuh:29-132,
// index_batcher.cu): the indices of the query and of the target are cut into
// host batches, the sections kept in host memory together, and every host
// batch into device batches, the sections kept in device memory together.
#pragma once

#include <claraparabricks/genomeworks/cudamapper/index_descriptor.hpp>
#include <claraparabricks/genomeworks/io/fasta_parser.hpp>
#include <claraparabricks/genomeworks/types.hpp>

#include <cstdint>
#include <memory>
#include <vector>

namespace claraparabricks
{
namespace genomeworks
{
namespace cudamapper
{

/// One section of query indices and one of target indices, of a host or of a device batch.
struct IndexBatch
{
    std::vector<IndexDescriptor> query_indices;
    std::vector<IndexDescriptor> target_indices;
};

/// A host batch and the device batches it is worked through in.
struct BatchOfIndices
{
    IndexBatch host_batch;
    std::vector<IndexBatch> device_batches;
};

using number_of_indices_t = std::int32_t;

/// Every section of *_indices_per_host_batch query indices is paired with
/// every such section of target indices, and within a host batch every section
/// of *_indices_per_device_batch indices with every other.  With
/// same_query_and_target only the upper triangle is made: a target section is
/// paired with the query sections that do not come after it, since (a, b)
/// covers (b, a).  The device batches of a host batch are a triangle only when
/// that batch's query and target sections are equal.
/// Throws std::invalid_argument when same_query_and_target holds and the two
/// sides differ in indices per host batch, in indices per device batch, in the
/// parser or in basepairs per index; and, where the reference would not
/// return, for a number of indices per batch below 1.
std::vector<BatchOfIndices> generate_batches_of_indices(number_of_indices_t query_indices_per_host_batch,
                                                        number_of_indices_t query_indices_per_device_batch,
                                                        number_of_indices_t target_indices_per_host_batch,
                                                        number_of_indices_t target_indices_per_device_batch,
                                                        std::shared_ptr<const io::FastaParser> query_parser,
                                                        std::shared_ptr<const io::FastaParser> target_parser,
                                                        number_of_basepairs_t query_basepairs_per_index,
                                                        number_of_basepairs_t target_basepairs_per_index,
                                                        bool same_query_and_target);

namespace details
{
namespace index_batcher
{

/// The pairs of sections described at generate_batches_of_indices, for one level.
std::vector<IndexBatch> group_into_batches(const std::vector<IndexDescriptor>& query_indices,
                                           const std::vector<IndexDescriptor>& target_indices,
                                           number_of_indices_t query_indices_per_batch,
                                           number_of_indices_t target_indices_per_batch,
                                           bool same_query_and_target);

} // namespace index_batcher
} // namespace details

} // namespace cudamapper
} // namespace genomeworks
} // namespace claraparabricks

namespace claragenomics = claraparabricks::genomeworks;
