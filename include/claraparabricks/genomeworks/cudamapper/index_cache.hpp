// Caches of indices of cudamapper (reference cudamapper/src/index_cache.cuh:43-213,
// index_cache.cu).  IndexCacheHost builds the indices of a host batch once and
// keeps them in host memory; IndexCacheDevice holds those of the device batch
// at work, fetched from the host cache.  One object of each serves the query
// side and the target side; with same_query_and_target an index that the other
// side already holds is shared, not built or copied again.
#pragma once

#include <claraparabricks/genomeworks/cudamapper/index.hpp>
#include <claraparabricks/genomeworks/cudamapper/index_descriptor.hpp>
#include <claraparabricks/genomeworks/io/fasta_parser.hpp>
#include <claraparabricks/genomeworks/utils/allocator.hpp>

#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <memory>
#include <unordered_map>
#include <vector>

namespace claraparabricks
{
namespace genomeworks
{
namespace cudamapper
{

class IndexCacheHost
{
public:
    IndexCacheHost(bool same_query_and_target, DefaultDeviceAllocator allocator,
                   std::shared_ptr<io::FastaParser> query_parser, std::shared_ptr<io::FastaParser> target_parser,
                   std::uint64_t kmer_size, std::uint64_t window_size, bool hash_representations = true,
                   double filtering_parameter = 1.0, hipStream_t stream = 0);
    IndexCacheHost(const IndexCacheHost&) = delete;
    IndexCacheHost& operator=(const IndexCacheHost&) = delete;

    /// Replaces the content of the query (target) cache by the indices of the
    /// descriptors.  An index the cache held before is kept, not built again;
    /// with same_query_and_target one the other side holds is shared.  The
    /// indices named in descriptors_of_indices_to_keep_on_device also stay on
    /// the device until they are fetched once.  skip_copy_to_host, for when
    /// both lists are the same, makes no host copy at all.
    void generate_query_cache_content(const std::vector<IndexDescriptor>& descriptors_of_indices_to_cache,
                                      const std::vector<IndexDescriptor>& descriptors_of_indices_to_keep_on_device = {},
                                      bool skip_copy_to_host = false);
    void generate_target_cache_content(const std::vector<IndexDescriptor>& descriptors_of_indices_to_cache,
                                       const std::vector<IndexDescriptor>& descriptors_of_indices_to_keep_on_device = {},
                                       bool skip_copy_to_host = false);

    /// The index on the device: the one kept there, handed out once, or else a
    /// copy of the host's.  Throws std::out_of_range for a descriptor that is not cached.
    std::shared_ptr<Index> get_index_from_query_cache(const IndexDescriptor& descriptor_of_index_to_cache);
    std::shared_ptr<Index> get_index_from_target_cache(const IndexDescriptor& descriptor_of_index_to_cache);

private:
    using cache_type_t = std::unordered_map<IndexDescriptor, std::shared_ptr<const IndexHostCopyBase>, IndexDescriptorHash>;
    using device_cache_type_t = std::unordered_map<IndexDescriptor, std::shared_ptr<Index>, IndexDescriptorHash>;

    void generate_cache_content(const std::vector<IndexDescriptor>& to_cache,
                                const std::vector<IndexDescriptor>& to_keep_on_device, bool skip_copy_to_host,
                                bool query_side);
    std::shared_ptr<Index> get_index_from_cache(const IndexDescriptor& descriptor, bool query_side);

    cache_type_t query_cache_, target_cache_;
    device_cache_type_t query_temp_device_cache_, target_temp_device_cache_;
    const bool same_query_and_target_;
    DefaultDeviceAllocator allocator_;
    std::shared_ptr<io::FastaParser> query_parser_, target_parser_;
    const std::uint64_t kmer_size_, window_size_;
    const bool hash_representations_;
    const double filtering_parameter_;
    const hipStream_t stream_;
};

class IndexCacheDevice
{
public:
    IndexCacheDevice(bool same_query_and_target, std::shared_ptr<IndexCacheHost> index_cache_host);
    IndexCacheDevice(const IndexCacheDevice&) = delete;
    IndexCacheDevice& operator=(const IndexCacheDevice&) = delete;

    /// Replaces the content of the query (target) cache by the indices of the
    /// descriptors: kept when held before, shared with the other side under
    /// same_query_and_target, else fetched from the host cache.
    void generate_query_cache_content(const std::vector<IndexDescriptor>& descriptors_of_indices_to_cache);
    void generate_target_cache_content(const std::vector<IndexDescriptor>& descriptors_of_indices_to_cache);

    /// Throws std::out_of_range for a descriptor that is not cached.
    std::shared_ptr<Index> get_index_from_query_cache(const IndexDescriptor& descriptor_of_index_to_cache);
    std::shared_ptr<Index> get_index_from_target_cache(const IndexDescriptor& descriptor_of_index_to_cache);

private:
    using cache_type_t = std::unordered_map<IndexDescriptor, std::shared_ptr<Index>, IndexDescriptorHash>;
    void generate_cache_content(const std::vector<IndexDescriptor>& to_cache, bool query_side);

    cache_type_t query_cache_, target_cache_;
    const bool same_query_and_target_;
    std::shared_ptr<IndexCacheHost> index_cache_host_;
};

} // namespace cudamapper
} // namespace genomeworks
} // namespace claraparabricks

namespace claragenomics = claraparabricks::genomeworks;
