// The host copy of an index and the two caches of indices (reference
// cudamapper/src/index_host_copy.cu, index_cache.cu:29-294) with the C ABI of
// the host copy (include/gwamd_cudamapper.h).  Copies only: no kernel.
#include <claraparabricks/genomeworks/cudamapper/index.hpp>
#include <claraparabricks/genomeworks/cudamapper/index_cache.hpp>

#include "allocator_handle.hpp"
#include "mapper_capi.hpp"
#include "mapper_index_impl.hpp"

#include <unordered_set>

namespace gm = gwamd::mapper;

namespace claraparabricks
{
namespace genomeworks
{
namespace cudamapper
{
namespace
{

template <typename T, typename D>
void to_host(std::vector<T>& h, const gm::DevBuf<D>& d, hipStream_t stream)
{
    static_assert(sizeof(T) == sizeof(D), "copied as bytes");
    h.resize(d.size());
    if (d.size() > 0)
        GWAMD_HIP_CHECK(hipMemcpyAsync(h.data(), d.data(), d.size() * sizeof(D), hipMemcpyDeviceToHost, stream));
}

template <typename T, typename D>
void to_device(gm::DevBuf<D>& d, const std::vector<T>& h, const gm::Budget& budget, hipStream_t stream)
{
    static_assert(sizeof(T) == sizeof(D), "copied as bytes");
    d.alloc(h.size(), budget);
    if (!h.empty())
        GWAMD_HIP_CHECK(hipMemcpyAsync(d.data(), h.data(), h.size() * sizeof(D), hipMemcpyHostToDevice, stream));
}

class IndexHostCopy : public IndexHostCopyBase
{
public:
    using Direction = SketchElement::DirectionOfRepresentation;

    IndexHostCopy(const IndexHip& index, read_id_t first_read_id, std::uint64_t kmer_size, std::uint64_t window_size,
                  hipStream_t stream)
        : number_of_reads_(index.data.number_of_reads)
        , smallest_read_id_(index.data.smallest_read_id)
        , largest_read_id_(index.data.largest_read_id)
        , longest_read_(index.data.number_of_basepairs_in_longest_read)
        , first_read_id_(first_read_id)
        , kmer_size_(kmer_size)
        , window_size_(window_size)
    {
        gwamd::host::ScopedDevice dev(index.data.device_id);
        to_host(representations_, index.data.representations, stream);
        to_host(read_ids_, index.data.read_ids, stream);
        to_host(positions_in_reads_, index.data.positions_in_reads, stream);
        to_host(directions_, index.data.directions_of_reads, stream);
        to_host(unique_, index.data.unique_representations, stream);
        to_host(first_occurrence_, index.data.first_occurrence_of_representations, stream);
        GWAMD_HIP_CHECK(hipStreamSynchronize(stream));
    }

    std::unique_ptr<Index> copy_index_to_device(DefaultDeviceAllocator allocator, const hipStream_t stream) const override
    {
        auto index          = std::make_unique<IndexHip>();
        gm::IndexData& data = index->data;
        // (an empty index touches no device, like the one create_index makes)
        if (!representations_.empty() || !first_occurrence_.empty())
            GWAMD_HIP_CHECK(hipGetDevice(&data.device_id));
        const gm::Budget budget = allocator.budget();
        to_device(data.representations, representations_, budget, stream);
        to_device(data.read_ids, read_ids_, budget, stream);
        to_device(data.positions_in_reads, positions_in_reads_, budget, stream);
        to_device(data.directions_of_reads, directions_, budget, stream);
        to_device(data.unique_representations, unique_, budget, stream);
        to_device(data.first_occurrence_of_representations, first_occurrence_, budget, stream);
        data.number_of_reads                     = number_of_reads_;
        data.smallest_read_id                    = smallest_read_id_;
        data.largest_read_id                     = largest_read_id_;
        data.number_of_basepairs_in_longest_read = longest_read_;
        if (!representations_.empty() || !first_occurrence_.empty())
            GWAMD_HIP_CHECK(hipStreamSynchronize(stream)); // the copy may be freed once this returns
        index->refresh_views();
        return index;
    }

    const std::vector<representation_t>& representations() const override { return representations_; }
    const std::vector<read_id_t>& read_ids() const override { return read_ids_; }
    const std::vector<position_in_read_t>& positions_in_reads() const override { return positions_in_reads_; }
    const std::vector<Direction>& directions_of_reads() const override { return directions_; }
    const std::vector<representation_t>& unique_representations() const override { return unique_; }
    const std::vector<std::uint32_t>& first_occurrence_of_representations() const override
    {
        return first_occurrence_;
    }
    read_id_t number_of_reads() const override { return number_of_reads_; }
    position_in_read_t number_of_basepairs_in_longest_read() const override { return longest_read_; }
    read_id_t first_read_id() const override { return first_read_id_; }
    std::uint64_t kmer_size() const override { return kmer_size_; }
    std::uint64_t window_size() const override { return window_size_; }
    // (not part of the reference's interface: what the Index that comes back reports)
    read_id_t smallest_read_id() const { return smallest_read_id_; }
    read_id_t largest_read_id() const { return largest_read_id_; }

private:
    std::vector<representation_t> representations_, unique_;
    std::vector<read_id_t> read_ids_;
    std::vector<position_in_read_t> positions_in_reads_;
    std::vector<Direction> directions_;
    std::vector<std::uint32_t> first_occurrence_;
    read_id_t number_of_reads_, smallest_read_id_, largest_read_id_;
    position_in_read_t longest_read_;
    read_id_t first_read_id_;
    std::uint64_t kmer_size_, window_size_;
};

} // namespace

std::unique_ptr<IndexHostCopyBase> IndexHostCopyBase::create_cache(const Index& index, const read_id_t first_read_id,
                                                                   const std::uint64_t kmer_size,
                                                                   const std::uint64_t window_size,
                                                                   const hipStream_t stream)
{
    const auto* impl = dynamic_cast<const IndexHip*>(&index);
    if (!impl)
        throw std::invalid_argument("create_cache takes an index made by Index::create_index");
    return std::make_unique<IndexHostCopy>(*impl, first_read_id, kmer_size, window_size, stream);
}

// ---- IndexCacheHost ---------------------------------------------------------------

IndexCacheHost::IndexCacheHost(const bool same_query_and_target, DefaultDeviceAllocator allocator,
                               std::shared_ptr<io::FastaParser> query_parser,
                               std::shared_ptr<io::FastaParser> target_parser, const std::uint64_t kmer_size,
                               const std::uint64_t window_size, const bool hash_representations,
                               const double filtering_parameter, const hipStream_t stream)
    : same_query_and_target_(same_query_and_target)
    , allocator_(allocator)
    , query_parser_(std::move(query_parser))
    , target_parser_(std::move(target_parser))
    , kmer_size_(kmer_size)
    , window_size_(window_size)
    , hash_representations_(hash_representations)
    , filtering_parameter_(filtering_parameter)
    , stream_(stream)
{
}

void IndexCacheHost::generate_query_cache_content(const std::vector<IndexDescriptor>& to_cache,
                                                  const std::vector<IndexDescriptor>& to_keep_on_device,
                                                  const bool skip_copy_to_host)
{
    generate_cache_content(to_cache, to_keep_on_device, skip_copy_to_host, true);
}

void IndexCacheHost::generate_target_cache_content(const std::vector<IndexDescriptor>& to_cache,
                                                   const std::vector<IndexDescriptor>& to_keep_on_device,
                                                   const bool skip_copy_to_host)
{
    generate_cache_content(to_cache, to_keep_on_device, skip_copy_to_host, false);
}

std::shared_ptr<Index> IndexCacheHost::get_index_from_query_cache(const IndexDescriptor& descriptor)
{
    return get_index_from_cache(descriptor, true);
}

std::shared_ptr<Index> IndexCacheHost::get_index_from_target_cache(const IndexDescriptor& descriptor)
{
    return get_index_from_cache(descriptor, false);
}

void IndexCacheHost::generate_cache_content(const std::vector<IndexDescriptor>& to_cache,
                                            const std::vector<IndexDescriptor>& to_keep_on_device,
                                            const bool skip_copy_to_host, const bool query_side)
{
    // without a host copy an index that is not kept on the device would be built and lost
    if (skip_copy_to_host && !(to_cache == to_keep_on_device))
        throw std::invalid_argument("skip_copy_to_host needs every cached index kept on the device");
    cache_type_t& mine                     = query_side ? query_cache_ : target_cache_;
    const cache_type_t& other              = query_side ? target_cache_ : query_cache_;
    device_cache_type_t& mine_on_device    = query_side ? query_temp_device_cache_ : target_temp_device_cache_;
    const device_cache_type_t& other_on_device = query_side ? target_temp_device_cache_ : query_temp_device_cache_;
    const io::FastaParser& parser          = query_side ? *query_parser_ : *target_parser_;
    const std::unordered_set<IndexDescriptor, IndexDescriptorHash> keep(to_keep_on_device.begin(),
                                                                        to_keep_on_device.end());
    cache_type_t new_cache;
    mine_on_device.clear();
    for (const IndexDescriptor& descriptor : to_cache)
    {
        const bool keep_on_device = keep.count(descriptor) != 0;
        std::shared_ptr<const IndexHostCopyBase> on_host;
        std::shared_ptr<Index> on_device;
        if (same_query_and_target_)
        {
            // the other side's copy is this side's too
            const auto held = other.find(descriptor);
            if (held != other.end())
            {
                on_host = held->second;
                if (keep_on_device)
                {
                    const auto held_on_device = other_on_device.find(descriptor);
                    on_device = held_on_device != other_on_device.end()
                                    ? held_on_device->second
                                    : std::shared_ptr<Index>(on_host->copy_index_to_device(allocator_, stream_));
                }
            }
        }
        if (!on_host)
        {
            const auto held = mine.find(descriptor);
            if (held != mine.end())
            {
                on_host = held->second;
                if (keep_on_device)
                    on_device = on_host->copy_index_to_device(allocator_, stream_);
            }
            else
            {
                on_device = Index::create_index(allocator_, parser, descriptor.first_read(),
                                                descriptor.first_read() + descriptor.number_of_reads(), kmer_size_,
                                                window_size_, hash_representations_, filtering_parameter_, stream_);
                if (!skip_copy_to_host)
                    on_host = IndexHostCopyBase::create_cache(*on_device, descriptor.first_read(), kmer_size_,
                                                              window_size_, stream_);
            }
        }
        if (!skip_copy_to_host)
            new_cache[descriptor] = on_host;
        if (keep_on_device)
            mine_on_device[descriptor] = on_device;
    }
    std::swap(new_cache, mine);
}

std::shared_ptr<Index> IndexCacheHost::get_index_from_cache(const IndexDescriptor& descriptor, const bool query_side)
{
    const cache_type_t& host_cache = query_side ? query_cache_ : target_cache_;
    device_cache_type_t& on_device = query_side ? query_temp_device_cache_ : target_temp_device_cache_;
    const auto kept                = on_device.find(descriptor);
    if (kept != on_device.end())
    {
        // an index kept on the device is handed out once
        std::shared_ptr<Index> index = kept->second;
        on_device.erase(kept);
        return index;
    }
    return host_cache.at(descriptor)->copy_index_to_device(allocator_, stream_);
}

// ---- IndexCacheDevice -------------------------------------------------------------

IndexCacheDevice::IndexCacheDevice(const bool same_query_and_target, std::shared_ptr<IndexCacheHost> index_cache_host)
    : same_query_and_target_(same_query_and_target)
    , index_cache_host_(std::move(index_cache_host))
{
}

void IndexCacheDevice::generate_query_cache_content(const std::vector<IndexDescriptor>& to_cache)
{
    generate_cache_content(to_cache, true);
}

void IndexCacheDevice::generate_target_cache_content(const std::vector<IndexDescriptor>& to_cache)
{
    generate_cache_content(to_cache, false);
}

std::shared_ptr<Index> IndexCacheDevice::get_index_from_query_cache(const IndexDescriptor& descriptor)
{
    return query_cache_.at(descriptor);
}

std::shared_ptr<Index> IndexCacheDevice::get_index_from_target_cache(const IndexDescriptor& descriptor)
{
    return target_cache_.at(descriptor);
}

void IndexCacheDevice::generate_cache_content(const std::vector<IndexDescriptor>& to_cache, const bool query_side)
{
    cache_type_t& mine        = query_side ? query_cache_ : target_cache_;
    const cache_type_t& other = query_side ? target_cache_ : query_cache_;
    cache_type_t new_cache;
    for (const IndexDescriptor& descriptor : to_cache)
    {
        std::shared_ptr<Index> index;
        if (same_query_and_target_)
        {
            const auto held = other.find(descriptor);
            if (held != other.end())
                index = held->second;
        }
        if (!index)
        {
            const auto held = mine.find(descriptor);
            if (held != mine.end())
                index = held->second;
            else
                index = query_side ? index_cache_host_->get_index_from_query_cache(descriptor)
                                   : index_cache_host_->get_index_from_target_cache(descriptor);
        }
        new_cache[descriptor] = index;
    }
    std::swap(new_cache, mine);
}

} // namespace cudamapper
} // namespace genomeworks
} // namespace claraparabricks

// ---- C ABI ------------------------------------------------------------------

namespace cm = claraparabricks::genomeworks::cudamapper;

struct gwamd_index_host_copy
{
    std::unique_ptr<cm::IndexHostCopyBase> copy;
};

extern "C" {

int32_t gwamd_index_host_copy_create(const gwamd_index* index, uint32_t first_read_id, int32_t kmer_size,
                                     int32_t window_size, gwamd_index_host_copy** out)
{
    if (out)
        *out = nullptr;
    return gm::guarded_map([&] {
        if (!out || !index)
            throw std::invalid_argument("index or out is NULL");
        if (kmer_size < 1 || kmer_size > gm::kMaxKmerSize || window_size < 1 || window_size > gm::kMaxWindowSize)
            throw std::invalid_argument("kmer_size or window_size out of range");
        auto h  = std::make_unique<gwamd_index_host_copy>();
        h->copy = cm::IndexHostCopyBase::create_cache(*index->impl, first_read_id, uint64_t(kmer_size),
                                                      uint64_t(window_size), nullptr);
        *out    = h.release();
        return int32_t(0);
    });
}

int32_t gwamd_index_host_copy_to_device(const gwamd_index_host_copy* copy, int32_t device_id,
                                        gwamd_device_allocator* allocator_or_null, gwamd_index** out)
{
    if (out)
        *out = nullptr;
    return gm::guarded_map([&] {
        if (!out || !copy)
            throw std::invalid_argument("copy or out is NULL");
        if (device_id < 0)
            throw std::invalid_argument("device_id must not be negative");
        gwamd::host::ScopedDevice dev(device_id);
        std::unique_ptr<cm::Index> index = copy->copy->copy_index_to_device(
            allocator_or_null ? allocator_or_null->alloc : claraparabricks::genomeworks::DefaultDeviceAllocator(),
            nullptr);
        auto h = std::make_unique<gwamd_index>();
        h->impl.reset(static_cast<cm::IndexHip*>(index.release()));
        h->impl->data.device_id = device_id;
        *out                    = h.release();
        return int32_t(0);
    });
}

int32_t gwamd_index_host_copy_info(const gwamd_index_host_copy* copy, gwamd_index_info_t* info,
                                   uint32_t* first_read_id, int32_t* kmer_size, int32_t* window_size)
{
    return gm::guarded_map([&] {
        if (!copy || !info)
            throw std::invalid_argument("copy or info is NULL");
        const auto& c = static_cast<const cm::IndexHostCopy&>(*copy->copy); // the only implementation
        info->num_elements                       = int64_t(c.representations().size());
        info->num_unique_representations         = int64_t(c.unique_representations().size());
        info->number_of_reads                    = c.number_of_reads();
        info->smallest_read_id                   = c.smallest_read_id();
        info->largest_read_id                    = c.largest_read_id();
        info->number_of_basepairs_in_longest_read = c.number_of_basepairs_in_longest_read();
        if (first_read_id)
            *first_read_id = c.first_read_id();
        if (kmer_size)
            *kmer_size = int32_t(c.kmer_size());
        if (window_size)
            *window_size = int32_t(c.window_size());
        return int32_t(0);
    });
}

void gwamd_index_host_copy_free(gwamd_index_host_copy* copy) { delete copy; }

} // extern "C"
