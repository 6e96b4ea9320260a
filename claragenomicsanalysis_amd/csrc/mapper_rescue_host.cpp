// Host side of the overlap-end rescue: the reference's
// Overlapper::rescue_overlap_ends and
// details::overlapper::extend_overlap_by_sequence_similarity
// (cudamapper/src/overlapper.cpp:254-365) and their C ABI
// (include/gwamd_cudamapper.h).  The rescue of a list of overlaps runs in
// mapper_rescue.hip; the single round on one overlap is host code.  Every
// argument is checked here, before any device call, so that the kernel never
// forms an address outside the arrays it is given.
#include <claraparabricks/genomeworks/cudamapper/overlapper.hpp>

#include "allocator_handle.hpp"
#include "mapper_capi.hpp"

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <memory>
#include <string>
#include <string_view>
#include <vector>

namespace gm = gwamd::mapper;
namespace cm = claraparabricks::genomeworks::cudamapper;

namespace
{

// sequence_jaccard_similarity(a, b, 15, 1) >= required_similarity for two
// windows of one length (cudamapper_utils.cpp:114-170).  Substring i is
// s[i, min(L, 2i + 15)); only substrings i and n - 1 - i have its length, so
// it is counted into the multiset intersection when its rank among its own
// window's copies is below its number of copies in the other window.
bool similar(std::string_view a, std::string_view b, float required_similarity)
{
    const size_t len = a.size();
    size_t n = 1, shared = 0;
    if (len < size_t(gm::kRescueKmer))
        shared = a == b;
    else
    {
        n = len - gm::kRescueKmer + 1;
        for (size_t i = 0; i < n; i++)
        {
            const size_t j   = n - 1 - i;
            const size_t sub = std::min(i + gm::kRescueKmer, len - i);
            const std::string_view s = a.substr(i, sub);
            const int in_b = int(s == b.substr(i, sub)) + int(j != i && s == b.substr(j, sub));
            const int rank = j < i && s == a.substr(j, sub);
            shared += rank < in_b;
        }
    }
    return float(shared) / float(2 * n - shared) >= required_similarity;
}

void check_reads(const char* side, const gm::ReadSet& reads)
{
    if (reads.num_reads < 0)
        throw std::invalid_argument(std::string("the number of ") + side + " reads must not be negative");
    if (reads.num_reads > 0 && !reads.offsets)
        throw std::invalid_argument(std::string(side) + " offsets is NULL");
    gm::check_read_lengths(reads.offsets, reads.num_reads);
    if (reads.num_reads > 0 && !reads.bases && reads.offsets[reads.num_reads] > 0)
        throw std::invalid_argument(std::string(side) + " bases is NULL");
}

// everything gm::rescue_overlap_ends relies on; Record is gwamd_overlap or gm::OverlapRecord
template <typename Record>
void check_rescue_arguments(const gm::ReadSet& query, const gm::ReadSet& target, const Record* overlaps, int64_t n,
                            int32_t extension, float required_similarity)
{
    if (n < 0 || n >= (int64_t(1) << 31))
        throw std::invalid_argument("the number of overlaps must be between 0 and 2^31, got " + std::to_string(n));
    if (n > 0 && !overlaps)
        throw std::invalid_argument("overlaps is NULL");
    check_reads("query", query);
    check_reads("target", target);
    if (extension < 0 || extension > gm::kMaxRescueExtension)
        throw std::invalid_argument("extension must be between 0 and " + std::to_string(gm::kMaxRescueExtension) +
                                    ", got " + std::to_string(extension));
    if (required_similarity != required_similarity)
        throw std::invalid_argument("required_similarity is not a number");
    for (int64_t i = 0; i < n; i++)
    {
        const Record& o            = overlaps[i];
        const std::string which    = "overlap " + std::to_string(i);
        if (int64_t(o.query_read_id) >= query.num_reads || int64_t(o.target_read_id) >= target.num_reads)
            throw std::invalid_argument(which + ": read id beyond the reads");
        const int64_t query_length  = query.offsets[o.query_read_id + 1] - query.offsets[o.query_read_id];
        const int64_t target_length = target.offsets[o.target_read_id + 1] - target.offsets[o.target_read_id];
        if (o.query_start > o.query_end || int64_t(o.query_end) > query_length)
            throw std::invalid_argument(which + ": query positions are not start <= end <= read length");
        if (o.target_start > o.target_end || int64_t(o.target_end) > target_length)
            throw std::invalid_argument(which + ": target positions are not start <= end <= read length");
        if (o.relative_strand != '+' && o.relative_strand != '-')
            throw std::invalid_argument(which + ": relative_strand is neither '+' nor '-'");
    }
}

struct PackedReads
{
    std::string bases;
    std::vector<int64_t> offsets;
    explicit PackedReads(const claraparabricks::genomeworks::io::FastaParser& parser)
        : offsets(size_t(parser.get_num_seqences()) + 1, 0)
    {
        const uint32_t n = parser.get_num_seqences();
        for (uint32_t i = 0; i < n; i++)
            offsets[i + 1] = offsets[i] + int64_t(parser.get_sequence_by_id(i).seq.size());
        bases.reserve(size_t(offsets[n]));
        for (uint32_t i = 0; i < n; i++)
            bases += parser.get_sequence_by_id(i).seq;
    }
    gm::ReadSet view() const { return {bases.data(), offsets.data(), int64_t(offsets.size()) - 1}; }
};

static_assert(sizeof(cm::Overlap) == sizeof(gm::OverlapRecord) && sizeof(gwamd_overlap) == sizeof(gm::OverlapRecord),
              "overlaps are copied as bytes (field offsets: mapper_batch.cpp)");

int32_t rescue(const gm::ReadSet& query, const gm::ReadSet& target, const gwamd_overlap* overlaps, int64_t n,
               int32_t extension, float required_similarity, int32_t device_id, const gm::Budget& budget,
               gwamd_overlap** out, int64_t* num_out)
{
    gm::clear_overlap_outputs(out, num_out);
    return gm::guarded_map([&] {
        if (!out || !num_out)
            throw std::invalid_argument("out or num_out is NULL");
        if (device_id < 0)
            throw std::invalid_argument("device_id must not be negative");
        check_rescue_arguments(query, target, overlaps, n, extension, required_similarity);
        if (n == 0)
            return int32_t(0);
        std::vector<gm::OverlapRecord> records(static_cast<size_t>(n));
        std::memcpy(static_cast<void*>(records.data()), overlaps, size_t(n) * sizeof(gwamd_overlap));
        gwamd::host::ScopedDevice dev(device_id);
        gm::rescue_overlap_ends(records.data(), n, query, target, extension, required_similarity, budget, nullptr);
        gm::hand_over(records, out, num_out);
        return int32_t(0);
    });
}

} // namespace

namespace claraparabricks
{
namespace genomeworks
{
namespace cudamapper
{

void details::overlapper::extend_overlap_by_sequence_similarity(Overlap& overlap, gw_string_view_t& query_sequence,
                                                                gw_string_view_t& target_sequence,
                                                                const std::int32_t extension,
                                                                const float required_similarity)
{
    // the reference converts the extension to an unsigned position
    const position_in_read_t reach = static_cast<position_in_read_t>(extension);
    position_in_read_t& qs         = overlap.query_start_position_in_read_;
    position_in_read_t& qe         = overlap.query_end_position_in_read_;
    position_in_read_t& ts         = overlap.target_start_position_in_read_;
    position_in_read_t& te         = overlap.target_end_position_in_read_;
    const position_in_read_t head  = std::min({qs, ts, reach});
    if (similar(query_sequence.substr(qs - head, head), target_sequence.substr(ts - head, head), required_similarity))
    {
        qs -= head;
        ts -= head;
    }
    const position_in_read_t tail = std::min({reach, position_in_read_t(query_sequence.size()) - qe,
                                              position_in_read_t(target_sequence.size()) - te});
    if (similar(query_sequence.substr(qe, tail), target_sequence.substr(te, tail), required_similarity))
    {
        qe += tail;
        te += tail;
    }
}

void Overlapper::rescue_overlap_ends(std::vector<Overlap>& overlaps, const io::FastaParser& query_parser,
                                     const io::FastaParser& target_parser, const std::int32_t /*extension*/,
                                     const float /*required_similarity*/)
{
    if (overlaps.empty())
        return;
    const PackedReads query(query_parser);
    std::unique_ptr<PackedReads> other; // one parser on both sides is packed, and uploaded, once
    if (&target_parser != &query_parser)
        other = std::make_unique<PackedReads>(target_parser);
    const gm::ReadSet query_reads  = query.view();
    const gm::ReadSet target_reads = other ? other->view() : query_reads;
    std::vector<gm::OverlapRecord> records(overlaps.size());
    std::memcpy(static_cast<void*>(records.data()), overlaps.data(), overlaps.size() * sizeof(Overlap));
    // what the reference passes to every round, whatever it is given (overlapper.cpp:345)
    const std::int32_t extension    = 100;
    const float required_similarity = 0.9f;
    check_rescue_arguments(query_reads, target_reads, records.data(), int64_t(records.size()), extension,
                           required_similarity);
    gm::rescue_overlap_ends(records.data(), int64_t(records.size()), query_reads, target_reads, extension,
                            required_similarity, nullptr, nullptr);
    std::memcpy(static_cast<void*>(overlaps.data()), records.data(), overlaps.size() * sizeof(Overlap));
}

} // namespace cudamapper
} // namespace genomeworks
} // namespace claraparabricks

// ---- C ABI ------------------------------------------------------------------

extern "C" {

int32_t gwamd_rescue_overlap_ends(const char* query_bases, const int64_t* query_offsets, int32_t num_queries,
                                  const char* target_bases, const int64_t* target_offsets, int32_t num_targets,
                                  const gwamd_overlap* overlaps, int64_t n, int32_t extension,
                                  float required_similarity, int32_t device_id, gwamd_overlap** out, int64_t* num_out)
{
    return rescue({query_bases, query_offsets, num_queries}, {target_bases, target_offsets, num_targets}, overlaps, n,
                  extension, required_similarity, device_id, nullptr, out, num_out);
}

int32_t gwamd_rescue_overlap_ends_with_allocator(const char* query_bases, const int64_t* query_offsets,
                                                 int32_t num_queries, const char* target_bases,
                                                 const int64_t* target_offsets, int32_t num_targets,
                                                 const gwamd_overlap* overlaps, int64_t n, int32_t extension,
                                                 float required_similarity, int32_t device_id,
                                                 gwamd_device_allocator* allocator, gwamd_overlap** out,
                                                 int64_t* num_out)
{
    if (!allocator)
        return gm::allocator_is_null(out, num_out);
    return rescue({query_bases, query_offsets, num_queries}, {target_bases, target_offsets, num_targets}, overlaps, n,
                  extension, required_similarity, device_id, allocator->alloc.budget(), out, num_out);
}

int32_t gwamd_extend_overlap_by_sequence_similarity(gwamd_overlap* overlap, const char* query, int64_t query_len,
                                                    const char* target, int64_t target_len, int32_t extension,
                                                    float required_similarity)
{
    return gm::guarded_map([&] {
        if (!overlap)
            throw std::invalid_argument("overlap is NULL");
        const int64_t offsets[4] = {0, query_len, 0, target_len};
        const gm::ReadSet query_read{query, offsets, 1}, target_read{target, offsets + 2, 1};
        gm::OverlapRecord record;
        std::memcpy(static_cast<void*>(&record), overlap, sizeof(record));
        record.query_read_id = record.target_read_id = 0;
        record.relative_strand                       = '+'; // a round does not look at the strand
        check_rescue_arguments(query_read, target_read, &record, 1, 0, required_similarity);
        cm::Overlap o;
        std::memcpy(static_cast<void*>(&o), overlap, sizeof(o));
        std::string_view query_view(query ? query : "", size_t(query_len));
        std::string_view target_view(target ? target : "", size_t(target_len));
        cm::details::overlapper::extend_overlap_by_sequence_similarity(o, query_view, target_view, extension,
                                                                       required_similarity);
        std::memcpy(static_cast<void*>(overlap), &o, sizeof(o));
        return int32_t(0);
    });
}

} // extern "C"
