// Reads resident on the device (mapper_reads.hpp): the upload, the one check
// of a read set and the one check of overlaps against their reads that every
// entry point of the mapper and of cudapolish forwards to, a parser packed
// into bases and offsets, the C++ class
// cudamapper::DeviceReads with the Overlapper::rescue_overlap_ends overload on
// it, and their C ABI (include/gwamd_cudamapper.h).  Every argument is checked
// here, on the host copy of the offsets, before any device call, so that no
// kernel forms an address outside the arrays it is given.
#include <claraparabricks/genomeworks/cudamapper/device_reads.hpp>
#include <claraparabricks/genomeworks/cudamapper/overlapper.hpp>

#include "allocator_handle.hpp"
#include "mapper_capi.hpp"
#include "mapper_reads.hpp"

#include <cstring>
#include <string>
#include <vector>

namespace gm = gwamd::mapper;
namespace cm = claraparabricks::genomeworks::cudamapper;

namespace gwamd
{
namespace mapper
{

void check_read_set(const char* side, const ReadSet& reads)
{
    if (reads.num_reads < 0)
        throw std::invalid_argument(std::string("the number of ") + side + " reads must not be negative");
    if (reads.num_reads >= (int64_t(1) << 31))
        throw std::invalid_argument(std::string("the number of ") + side + " reads must be below 2^31");
    if (reads.num_reads > 0 && !reads.offsets)
        throw std::invalid_argument(std::string(side) + " offsets is NULL");
    check_read_lengths(reads.offsets, reads.num_reads);
    if (reads.num_reads > 0 && !reads.bases && reads.offsets[reads.num_reads] > 0)
        throw std::invalid_argument(std::string(side) + " bases is NULL");
}

void check_qualities(const ReadSet& reads, const char* qualities)
{
    if (reads.num_reads == 0)
        return;
    const int64_t first = reads.offsets[0], last = reads.offsets[reads.num_reads];
    if (!qualities && last > first)
        throw std::invalid_argument("qualities is NULL");
    for (int64_t i = first; i < last; i++)
        if (qualities[i] < 33 || qualities[i] > 126)
            throw std::invalid_argument("quality character " + std::to_string(int(uint8_t(qualities[i]))) +
                                        " at base " + std::to_string(i - first) + " is outside 33..126");
}

void check_overlap_count(const void* overlaps, int64_t n)
{
    if (n < 0 || n >= (int64_t(1) << 31))
        throw std::invalid_argument("the number of overlaps must be between 0 and 2^31, got " + std::to_string(n));
    if (n > 0 && !overlaps)
        throw std::invalid_argument("overlaps is NULL");
}

void check_overlaps(const int64_t* query_offsets, int64_t num_queries, const int64_t* target_offsets,
                    int64_t num_targets, const OverlapRecord* overlaps, int64_t n)
{
    check_overlap_count(overlaps, n);
    for (int64_t i = 0; i < n; i++)
    {
        const OverlapRecord& o  = overlaps[i];
        const std::string which = "overlap " + std::to_string(i);
        if (int64_t(o.query_read_id) >= num_queries || int64_t(o.target_read_id) >= num_targets)
            throw std::invalid_argument(which + ": read id beyond the reads");
        const int64_t query_length  = query_offsets[size_t(o.query_read_id) + 1] - query_offsets[o.query_read_id];
        const int64_t target_length = target_offsets[size_t(o.target_read_id) + 1] - target_offsets[o.target_read_id];
        if (o.query_start > o.query_end || int64_t(o.query_end) > query_length)
            throw std::invalid_argument(which + ": query positions are not start <= end <= read length");
        if (o.target_start > o.target_end || int64_t(o.target_end) > target_length)
            throw std::invalid_argument(which + ": target positions are not start <= end <= read length");
        if (o.relative_strand != '+' && o.relative_strand != '-')
            throw std::invalid_argument(which + ": relative_strand is neither '+' nor '-'");
    }
}

void check_on_current_device(const DeviceReads& query, const DeviceReads& target)
{
    int current = -1;
    GWAMD_HIP_CHECK(hipGetDevice(&current));
    if (query.device_id != current || target.device_id != current)
        throw std::invalid_argument("the reads are on device " + std::to_string(query.device_id) + " and " +
                                    std::to_string(target.device_id) + ", the current device is " +
                                    std::to_string(current));
}

PackedReads::PackedReads(const claraparabricks::genomeworks::io::FastaParser& parser)
    : PackedReads(parser, 0, parser.get_num_seqences())
{
}

PackedReads::PackedReads(const claraparabricks::genomeworks::io::FastaParser& parser, uint32_t first,
                         uint32_t past_the_last)
    : offsets(size_t(past_the_last - first) + 1, 0)
{
    const uint32_t n = past_the_last - first;
    for (uint32_t i = 0; i < n; i++)
        offsets[i + 1] = offsets[i] + int64_t(parser.get_sequence_by_id(first + i).seq.size());
    bases.reserve(size_t(offsets[n]));
    for (uint32_t i = 0; i < n; i++)
        bases += parser.get_sequence_by_id(first + i).seq;
}

void PackedReads::pack_qualities(const claraparabricks::genomeworks::io::FastaParser& parser)
{
    const uint32_t n = uint32_t(offsets.size() - 1);
    qualities.clear();
    qualities.reserve(bases.size());
    for (uint32_t i = 0; i < n; i++)
    {
        const std::string& q = parser.get_quality_by_id(i);
        if (int64_t(q.size()) != offsets[i + 1] - offsets[i])
            throw std::invalid_argument("read " + std::to_string(i) + " has " + std::to_string(q.size()) +
                                        " quality characters for " + std::to_string(offsets[i + 1] - offsets[i]) +
                                        " bases");
        qualities += q;
    }
}

namespace
{

// kReadsPad zero bytes, `total` bytes of src, zeros up to a multiple of 16, kReadsPad zero bytes
void upload_padded(DevBuf<uint8_t>& storage, const char* src, size_t total, const Budget& budget, hipStream_t stream)
{
    const size_t padded = (total + 15) / 16 * 16;
    // padded at both ends: the gather kernels read whole aligned words (kReadsPad)
    storage.alloc(kReadsPad + padded + kReadsPad, budget);
    GWAMD_HIP_CHECK(hipMemsetAsync(storage.data(), 0, kReadsPad, stream));
    GWAMD_HIP_CHECK(hipMemsetAsync(storage.data() + kReadsPad + total, 0, padded - total + kReadsPad, stream));
    if (total > 0)
        GWAMD_HIP_CHECK(hipMemcpyAsync(storage.data() + kReadsPad, src, total, hipMemcpyHostToDevice, stream));
}

} // namespace

std::unique_ptr<DeviceReads> make_device_reads(const ReadSet& reads, const char* qualities, int device_id,
                                               const Budget& budget, hipStream_t stream)
{
    auto d       = std::make_unique<DeviceReads>();
    d->device_id = device_id;
    d->offsets.assign(size_t(reads.num_reads) + 1, 0);
    if (reads.num_reads > 0)
        std::memcpy(d->offsets.data(), reads.offsets, d->offsets.size() * sizeof(int64_t));
    // offsets may begin anywhere in the caller's array: the handle's begin at 0
    const int64_t first = d->offsets.front();
    for (int64_t& o : d->offsets)
        o -= first;
    const size_t total = size_t(d->offsets.back());
    upload_padded(d->storage, reads.bases + first, total, budget, stream);
    if (qualities)
    {
        upload_padded(d->qual_storage, qualities + first, total, budget, stream);
        d->has_qualities = true;
    }
    d->d_offsets.alloc(d->offsets.size(), budget);
    GWAMD_HIP_CHECK(hipMemcpyAsync(d->d_offsets.data(), d->offsets.data(), d->offsets.size() * sizeof(int64_t),
                                   hipMemcpyHostToDevice, stream));
    GWAMD_HIP_CHECK(hipStreamSynchronize(stream)); // the caller's arrays may go
    return d;
}

} // namespace mapper
} // namespace gwamd

namespace
{

void rescue_resident(const gm::DeviceReads& query, const gm::DeviceReads& target, gm::OverlapRecord* records,
                     int64_t n, int32_t extension, float required_similarity, const gm::Budget& budget)
{
    gm::check_overlaps(query, target, records, n);
    gm::check_rescue_numbers(extension, required_similarity);
    if (n == 0)
        return;
    gm::check_on_current_device(query, target);
    gm::rescue_overlap_ends(records, n, query, target, extension, required_similarity, budget, nullptr);
}

} // namespace

namespace claraparabricks
{
namespace genomeworks
{
namespace cudamapper
{

DeviceReads::DeviceReads() = default;
DeviceReads::~DeviceReads() = default;

std::unique_ptr<DeviceReads> DeviceReads::create(DefaultDeviceAllocator allocator, const io::FastaParser& parser,
                                                 hipStream_t stream)
{
    const gm::PackedReads packed(parser);
    const gm::ReadSet reads = packed.view();
    gm::check_read_set("parser", reads);
    int device_id = 0;
    GWAMD_HIP_CHECK(hipGetDevice(&device_id));
    std::unique_ptr<DeviceReads> out(new DeviceReads());
    out->impl_        = std::make_unique<Impl>();
    out->impl_->reads = gm::make_device_reads(reads, device_id, allocator.budget(), stream);
    return out;
}

std::unique_ptr<DeviceReads> DeviceReads::create(DefaultDeviceAllocator allocator, const io::FastaParser& parser,
                                                 with_qualities_t, hipStream_t stream)
{
    gm::PackedReads packed(parser);
    packed.pack_qualities(parser);
    const gm::ReadSet reads = packed.view();
    gm::check_read_set("parser", reads);
    gm::check_qualities(reads, packed.qualities.data());
    int device_id = 0;
    GWAMD_HIP_CHECK(hipGetDevice(&device_id));
    std::unique_ptr<DeviceReads> out(new DeviceReads());
    out->impl_        = std::make_unique<Impl>();
    out->impl_->reads = gm::make_device_reads(reads, packed.qualities.data(), device_id, allocator.budget(), stream);
    return out;
}

bool DeviceReads::has_qualities() const { return impl_->reads->has_qualities; }
number_of_reads_t DeviceReads::number_of_reads() const { return number_of_reads_t(impl_->reads->num_reads()); }
std::int64_t DeviceReads::number_of_basepairs() const { return impl_->reads->num_bases(); }
std::int32_t DeviceReads::device_id() const { return impl_->reads->device_id; }

void Overlapper::rescue_overlap_ends(std::vector<Overlap>& overlaps, const DeviceReads& query_reads,
                                     const DeviceReads& target_reads, const std::int32_t extension,
                                     const float required_similarity)
{
    std::vector<gm::OverlapRecord> records = gm::to_records(overlaps.data(), int64_t(overlaps.size()));
    rescue_resident(*query_reads.impl().reads, *target_reads.impl().reads, records.data(), int64_t(records.size()),
                    extension, required_similarity, nullptr);
    gm::from_records(records, overlaps.data());
}

} // namespace cudamapper
} // namespace genomeworks
} // namespace claraparabricks

// ---- C ABI ------------------------------------------------------------------

namespace
{

int32_t create_device_reads(const char* bases, const char* qualities, bool with_qualities, const int64_t* offsets,
                            int32_t num_reads, int32_t device_id, gwamd_device_allocator* allocator_or_null,
                            gwamd_device_reads** out)
{
    if (out)
        *out = nullptr;
    return gm::guarded_map([&] {
        if (!out)
            throw std::invalid_argument("out is NULL");
        if (device_id < 0)
            throw std::invalid_argument("device_id must not be negative");
        const gm::ReadSet reads{bases, offsets, num_reads};
        gm::check_read_set("device", reads);
        static const char none = 0; // a set without a base has no quality to point at
        if (with_qualities)
        {
            gm::check_qualities(reads, qualities);
            if (!qualities)
                qualities = &none;
        }
        gwamd::host::ScopedDevice dev(device_id);
        auto h   = std::make_unique<gwamd_device_reads>();
        h->reads = gm::make_device_reads(reads, with_qualities ? qualities : nullptr, device_id,
                                         allocator_or_null ? allocator_or_null->alloc.budget() : nullptr, nullptr);
        *out     = h.release();
        return int32_t(0);
    });
}

} // namespace

extern "C" {

int32_t gwamd_device_reads_create(const char* bases, const int64_t* offsets, int32_t num_reads, int32_t device_id,
                                  gwamd_device_allocator* allocator_or_null, gwamd_device_reads** out)
{
    return create_device_reads(bases, nullptr, false, offsets, num_reads, device_id, allocator_or_null, out);
}

int32_t gwamd_device_reads_create_with_qualities(const char* bases, const char* qualities, const int64_t* offsets,
                                                 int32_t num_reads, int32_t device_id,
                                                 gwamd_device_allocator* allocator_or_null, gwamd_device_reads** out)
{
    return create_device_reads(bases, qualities, true, offsets, num_reads, device_id, allocator_or_null, out);
}

int32_t gwamd_device_reads_has_qualities(const gwamd_device_reads* reads)
{
    return gm::guarded_map([&] {
        if (!reads)
            throw std::invalid_argument("reads is NULL");
        return int32_t(reads->reads->has_qualities ? 1 : 0);
    });
}

void gwamd_device_reads_free(gwamd_device_reads* reads)
{
    if (!reads)
        return;
    try
    {
        gwamd::host::ScopedDevice dev(reads->reads->device_id);
        delete reads;
    }
    catch (const std::exception&)
    {
        delete reads;
    }
}

int32_t gwamd_device_reads_info(const gwamd_device_reads* reads, int64_t* num_reads, int64_t* num_bases,
                                int32_t* device_id)
{
    return gm::guarded_map([&] {
        if (!reads)
            throw std::invalid_argument("reads is NULL");
        if (num_reads)
            *num_reads = reads->reads->num_reads();
        if (num_bases)
            *num_bases = reads->reads->num_bases();
        if (device_id)
            *device_id = reads->reads->device_id;
        return int32_t(0);
    });
}

int32_t gwamd_rescue_overlap_ends_resident(const gwamd_device_reads* query_reads,
                                           const gwamd_device_reads* target_reads, const gwamd_overlap* overlaps,
                                           int64_t n, int32_t extension, float required_similarity,
                                           gwamd_device_allocator* allocator_or_null, gwamd_overlap** out,
                                           int64_t* num_out)
{
    gm::clear_overlap_outputs(out, num_out);
    return gm::guarded_map([&] {
        if (!out || !num_out)
            throw std::invalid_argument("out or num_out is NULL");
        if (!query_reads || !target_reads)
            throw std::invalid_argument("query_reads or target_reads is NULL");
        gm::check_overlap_count(overlaps, n);
        std::vector<gm::OverlapRecord> records = gm::to_records(overlaps, n);
        rescue_resident(*query_reads->reads, *target_reads->reads, records.data(), n, extension, required_similarity,
                        allocator_or_null ? allocator_or_null->alloc.budget() : nullptr);
        gm::hand_over(records, out, num_out);
        return int32_t(0);
    });
}

int32_t gwamd_internal_gather_overlap_regions(const gwamd_device_reads* query_reads,
                                              const gwamd_device_reads* target_reads, const gwamd_overlap* overlaps,
                                              int64_t n, int64_t stride, char* seqs_out, int32_t* lens_out)
{
    return gm::guarded_map([&] {
        if (!query_reads || !target_reads)
            throw std::invalid_argument("query_reads or target_reads is NULL");
        gm::check_overlap_count(overlaps, n);
        if (n > 0 && (!seqs_out || !lens_out))
            throw std::invalid_argument("seqs_out or lens_out is NULL");
        if (stride < 1 || stride >= (int64_t(1) << 31) || 2 * n * stride >= (int64_t(1) << 31))
            throw std::invalid_argument("stride must be at least 1 and 2 n stride below 2^31");
        const gm::DeviceReads& query  = *query_reads->reads;
        const gm::DeviceReads& target = *target_reads->reads;
        const std::vector<gm::OverlapRecord> records = gm::to_records(overlaps, n);
        gm::check_overlaps(query, target, records.data(), n);
        for (int64_t i = 0; i < n; i++)
            if (int64_t(records[size_t(i)].query_end - records[size_t(i)].query_start) > stride ||
                int64_t(records[size_t(i)].target_end - records[size_t(i)].target_start) > stride)
                throw std::invalid_argument("overlap " + std::to_string(i) + ": a region is longer than stride");
        if (n == 0)
            return int32_t(0);
        gm::check_on_current_device(query, target);
        gm::DevBuf<gm::OverlapRecord> d_records(size_t(n), nullptr);
        gm::DevBuf<char> d_seqs(size_t(2 * n * stride), nullptr);
        gm::DevBuf<int32_t> d_lens(size_t(2 * n), nullptr);
        GWAMD_HIP_CHECK(hipMemcpyAsync(d_records.data(), records.data(), size_t(n) * sizeof(gm::OverlapRecord),
                                       hipMemcpyHostToDevice, nullptr));
        GWAMD_HIP_CHECK(hipMemsetAsync(d_seqs.data(), 0, d_seqs.size(), nullptr));
        gm::gather_overlap_regions(d_seqs.data(), d_lens.data(), d_records.data(), n, stride, query, target, nullptr);
        GWAMD_HIP_CHECK(hipMemcpyAsync(seqs_out, d_seqs.data(), d_seqs.size(), hipMemcpyDeviceToHost, nullptr));
        GWAMD_HIP_CHECK(hipMemcpyAsync(lens_out, d_lens.data(), size_t(2 * n) * sizeof(int32_t),
                                       hipMemcpyDeviceToHost, nullptr));
        GWAMD_HIP_CHECK(hipStreamSynchronize(nullptr));
        return int32_t(0);
    });
}

} // extern "C"
