// Index descriptors and batches of indices (reference
// cudamapper/src/index_descriptor.cpp:76-109, index_batcher.cu) and their C ABI
// (include/gwamd_cudamapper.h).  Host code only.
#include <claraparabricks/genomeworks/cudamapper/index_batcher.hpp>
#include <claraparabricks/genomeworks/cudamapper/index_descriptor.hpp>

#include "mapper_capi.hpp"

#include <algorithm>
#include <memory>
#include <stdexcept>
#include <vector>

namespace cm = claraparabricks::genomeworks::cudamapper;

namespace
{

// group_reads_into_indices on the reads' lengths
template <typename LengthOf>
std::vector<cm::IndexDescriptor> group_lengths(uint32_t total_number_of_reads, uint64_t max_basepairs_per_index,
                                               LengthOf length_of)
{
    std::vector<cm::IndexDescriptor> descriptors;
    uint32_t first_read = 0, reads = 0;
    uint64_t basepairs  = 0;
    for (uint32_t read_id = 0; read_id < total_number_of_reads; read_id++)
    {
        const uint64_t in_this_read = length_of(read_id);
        if (in_this_read + basepairs > max_basepairs_per_index)
        {
            // the current index is closed whether or not it holds a read (read 0 over the limit: {0, 0})
            descriptors.emplace_back(first_read, reads);
            first_read = read_id;
            reads      = 1;
            basepairs  = in_this_read;
        }
        else
        {
            basepairs += in_this_read;
            reads++;
        }
    }
    descriptors.emplace_back(first_read, reads);
    return descriptors;
}

void check_same_sides(bool same, int32_t q_host, int32_t q_device, int32_t t_host, int32_t t_device, bool same_parser,
                      uint64_t q_basepairs, uint64_t t_basepairs)
{
    if (!same)
        return;
    if (q_host != t_host)
        throw std::invalid_argument("generate_batches_of_indices: same query and target, but their indices per host batch differ");
    if (q_device != t_device)
        throw std::invalid_argument("generate_batches_of_indices: same query and target, but their indices per device batch differ");
    if (!same_parser)
        throw std::invalid_argument("generate_batches_of_indices: same query and target, but two parsers");
    if (q_basepairs != t_basepairs)
        throw std::invalid_argument("generate_batches_of_indices: same query and target, but their basepairs per index differ");
}

std::vector<cm::BatchOfIndices> batches_of(const std::vector<cm::IndexDescriptor>& query_descriptors,
                                           const std::vector<cm::IndexDescriptor>& target_descriptors, int32_t q_host,
                                           int32_t q_device, int32_t t_host, int32_t t_device, bool same)
{
    std::vector<cm::IndexBatch> host_batches =
        cm::details::index_batcher::group_into_batches(query_descriptors, target_descriptors, q_host, t_host, same);
    std::vector<cm::BatchOfIndices> all;
    for (cm::IndexBatch& batch : host_batches)
    {
        // the device batches are a triangle only when the batch's two sections are the same
        const bool same_in_batch = same && batch.query_indices == batch.target_indices;
        std::vector<cm::IndexBatch> device_batches = cm::details::index_batcher::group_into_batches(
            batch.query_indices, batch.target_indices, q_device, t_device, same_in_batch);
        all.push_back({std::move(batch), std::move(device_batches)});
    }
    return all;
}

} // namespace

namespace claraparabricks
{
namespace genomeworks
{
namespace cudamapper
{

std::vector<IndexDescriptor> group_reads_into_indices(const io::FastaParser& parser,
                                                      const number_of_basepairs_t max_basepairs_per_index)
{
    return group_lengths(parser.get_num_seqences(), max_basepairs_per_index,
                         [&](uint32_t id) { return uint64_t(parser.get_sequence_by_id(id).seq.size()); });
}

std::vector<BatchOfIndices> generate_batches_of_indices(const number_of_indices_t query_indices_per_host_batch,
                                                        const number_of_indices_t query_indices_per_device_batch,
                                                        const number_of_indices_t target_indices_per_host_batch,
                                                        const number_of_indices_t target_indices_per_device_batch,
                                                        const std::shared_ptr<const io::FastaParser> query_parser,
                                                        const std::shared_ptr<const io::FastaParser> target_parser,
                                                        const number_of_basepairs_t query_basepairs_per_index,
                                                        const number_of_basepairs_t target_basepairs_per_index,
                                                        const bool same_query_and_target)
{
    check_same_sides(same_query_and_target, query_indices_per_host_batch, query_indices_per_device_batch,
                     target_indices_per_host_batch, target_indices_per_device_batch, query_parser == target_parser,
                     query_basepairs_per_index, target_basepairs_per_index);
    if (!query_parser || !target_parser)
        throw std::invalid_argument("generate_batches_of_indices: parser is null");
    return batches_of(group_reads_into_indices(*query_parser, query_basepairs_per_index),
                      group_reads_into_indices(*target_parser, target_basepairs_per_index),
                      query_indices_per_host_batch, query_indices_per_device_batch, target_indices_per_host_batch,
                      target_indices_per_device_batch, same_query_and_target);
}

namespace details
{
namespace index_batcher
{

std::vector<IndexBatch> group_into_batches(const std::vector<IndexDescriptor>& query_indices,
                                           const std::vector<IndexDescriptor>& target_indices,
                                           const number_of_indices_t query_indices_per_batch,
                                           const number_of_indices_t target_indices_per_batch,
                                           const bool same_query_and_target)
{
    if (same_query_and_target && query_indices_per_batch != target_indices_per_batch)
        throw std::invalid_argument("group_into_batches: same query and target, but their indices per batch differ");
    // (the reference's loops do not end on a step below 1)
    if (query_indices_per_batch < 1 || target_indices_per_batch < 1)
        throw std::invalid_argument("group_into_batches: indices per batch must be at least 1");
    std::vector<IndexBatch> batches;
    const size_t nq = query_indices.size(), nt = target_indices.size();
    for (size_t q = 0; q < nq; q += size_t(query_indices_per_batch))
    {
        // same query and target: the upper triangle of the query x target matrix only
        for (size_t t = same_query_and_target ? q : 0; t < nt; t += size_t(target_indices_per_batch))
        {
            const size_t q_end = std::min(q + size_t(query_indices_per_batch), nq);
            const size_t t_end = std::min(t + size_t(target_indices_per_batch), nt);
            batches.push_back({{query_indices.begin() + q, query_indices.begin() + q_end},
                               {target_indices.begin() + t, target_indices.begin() + t_end}});
        }
    }
    return batches;
}

} // namespace index_batcher
} // namespace details

} // namespace cudamapper
} // namespace genomeworks
} // namespace claraparabricks

// ---- C ABI ------------------------------------------------------------------

namespace
{

void check_lengths(const char* side, const int64_t* lengths, int32_t n, int64_t max_basepairs)
{
    if (n < 0 || (n > 0 && !lengths))
        throw std::invalid_argument(std::string(side) + ": a negative number of reads, or lengths is NULL");
    for (int32_t i = 0; i < n; i++)
        if (lengths[i] < 0 || lengths[i] >= (int64_t(1) << 31))
            throw std::invalid_argument(std::string(side) + ": read lengths must be between 0 and 2^31");
    if (max_basepairs < 0 || max_basepairs >= (int64_t(1) << 32))
        throw std::invalid_argument(std::string(side) + ": basepairs per index must be between 0 and 2^32");
}

std::vector<cm::IndexDescriptor> group(const int64_t* lengths, int32_t n, int64_t max_basepairs)
{
    return group_lengths(uint32_t(n), uint64_t(max_basepairs), [&](uint32_t id) { return uint64_t(lengths[id]); });
}

void flatten(std::vector<int64_t>& out, const std::vector<cm::IndexDescriptor>& descriptors)
{
    out.push_back(int64_t(descriptors.size()));
    for (const cm::IndexDescriptor& d : descriptors)
    {
        out.push_back(d.first_read());
        out.push_back(d.number_of_reads());
    }
}

} // namespace

extern "C" {

int32_t gwamd_group_reads_into_indices(const int64_t* lengths, int32_t n, int64_t max_basepairs,
                                       gwamd_index_descriptor** descriptors, int64_t* count)
{
    if (descriptors)
        *descriptors = nullptr;
    if (count)
        *count = 0;
    return gwamd::mapper::guarded_map([&] {
        if (!descriptors || !count)
            throw std::invalid_argument("descriptors or count is NULL");
        check_lengths("reads", lengths, n, max_basepairs);
        const std::vector<cm::IndexDescriptor> found = group(lengths, n, max_basepairs);
        std::unique_ptr<gwamd_index_descriptor[]> h(new gwamd_index_descriptor[found.size()]);
        for (size_t i = 0; i < found.size(); i++)
            h[i] = gwamd_index_descriptor{found[i].first_read(), found[i].number_of_reads()};
        *count       = int64_t(found.size());
        *descriptors = h.release();
        return int32_t(0);
    });
}

void gwamd_index_descriptors_free(gwamd_index_descriptor* descriptors) { delete[] descriptors; }

uint64_t gwamd_index_descriptor_hash(uint32_t first_read, uint32_t number_of_reads)
{
    return uint64_t(cm::IndexDescriptorHash()(cm::IndexDescriptor(first_read, number_of_reads)));
}

int32_t gwamd_generate_batches_of_indices(int32_t query_indices_per_host_batch, int32_t query_indices_per_device_batch,
                                          int32_t target_indices_per_host_batch,
                                          int32_t target_indices_per_device_batch, const int64_t* query_lengths,
                                          int32_t num_queries, const int64_t* target_lengths, int32_t num_targets,
                                          int64_t query_basepairs_per_index, int64_t target_basepairs_per_index,
                                          int32_t same_query_and_target, int64_t** batches, int64_t* count)
{
    if (batches)
        *batches = nullptr;
    if (count)
        *count = 0;
    return gwamd::mapper::guarded_map([&] {
        if (!batches || !count)
            throw std::invalid_argument("batches or count is NULL");
        check_lengths("queries", query_lengths, num_queries, query_basepairs_per_index);
        check_lengths("targets", target_lengths, num_targets, target_basepairs_per_index);
        // one parser on both sides: the same array of lengths
        check_same_sides(same_query_and_target != 0, query_indices_per_host_batch, query_indices_per_device_batch,
                         target_indices_per_host_batch, target_indices_per_device_batch,
                         query_lengths == target_lengths && num_queries == num_targets,
                         uint64_t(query_basepairs_per_index), uint64_t(target_basepairs_per_index));
        const std::vector<cm::BatchOfIndices> all =
            batches_of(group(query_lengths, num_queries, query_basepairs_per_index),
                       group(target_lengths, num_targets, target_basepairs_per_index), query_indices_per_host_batch,
                       query_indices_per_device_batch, target_indices_per_host_batch,
                       target_indices_per_device_batch, same_query_and_target != 0);
        std::vector<int64_t> flat;
        flat.push_back(int64_t(all.size()));
        for (const cm::BatchOfIndices& b : all)
        {
            flatten(flat, b.host_batch.query_indices);
            flatten(flat, b.host_batch.target_indices);
            flat.push_back(int64_t(b.device_batches.size()));
            for (const cm::IndexBatch& d : b.device_batches)
            {
                flatten(flat, d.query_indices);
                flatten(flat, d.target_indices);
            }
        }
        std::unique_ptr<int64_t[]> h(new int64_t[flat.size()]);
        std::copy(flat.begin(), flat.end(), h.get());
        *count   = int64_t(flat.size());
        *batches = h.release();
        return int32_t(0);
    });
}

void gwamd_batches_of_indices_free(int64_t* batches) { delete[] batches; }

} // extern "C"
