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
#include "mapper_reads.hpp"

#include <algorithm>
#include <cstddef>
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

// The n overlaps as records, after the checks of everything gm::rescue_overlap_ends
// relies on: the count, the two read sets, the two numbers, then each overlap
template <typename T>
std::vector<gm::OverlapRecord> checked_records(const gm::ReadSet& query, const gm::ReadSet& target, const T* overlaps,
                                               int64_t n, int32_t extension, float required_similarity)
{
    gm::check_overlap_count(overlaps, n);
    gm::check_read_set("query", query);
    gm::check_read_set("target", target);
    gm::check_rescue_numbers(extension, required_similarity);
    std::vector<gm::OverlapRecord> records = gm::to_records(overlaps, n);
    gm::check_overlaps(query, target, records.data(), n);
    return records;
}

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
        std::vector<gm::OverlapRecord> records =
            checked_records(query, target, overlaps, n, extension, required_similarity);
        if (n == 0)
            return int32_t(0);
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
    const gm::PackedReads query(query_parser);
    std::unique_ptr<gm::PackedReads> other; // one parser on both sides is packed, and uploaded, once
    if (&target_parser != &query_parser)
        other = std::make_unique<gm::PackedReads>(target_parser);
    const gm::ReadSet query_reads  = query.view();
    const gm::ReadSet target_reads = other ? other->view() : query_reads;
    // what the reference passes to every round, whatever it is given (overlapper.cpp:345)
    const std::int32_t extension    = 100;
    const float required_similarity = 0.9f;
    std::vector<gm::OverlapRecord> records = checked_records(query_reads, target_reads, overlaps.data(),
                                                             int64_t(overlaps.size()), extension, required_similarity);
    gm::rescue_overlap_ends(records.data(), int64_t(records.size()), query_reads, target_reads, extension,
                            required_similarity, nullptr, nullptr);
    gm::from_records(records, overlaps.data());
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
        gm::OverlapRecord record = gm::overlap_as<gm::OverlapRecord>(*overlap);
        record.query_read_id = record.target_read_id = 0;
        record.relative_strand                       = '+'; // a round does not look at the strand
        gm::check_read_set("query", query_read);
        gm::check_read_set("target", target_read);
        gm::check_rescue_numbers(0, required_similarity);
        gm::check_overlaps(query_read, target_read, &record, 1);
        cm::Overlap o = gm::overlap_as<cm::Overlap>(*overlap);
        std::string_view query_view(query ? query : "", size_t(query_len));
        std::string_view target_view(target ? target : "", size_t(target_len));
        cm::details::overlapper::extend_overlap_by_sequence_similarity(o, query_view, target_view, extension,
                                                                       required_similarity);
        *overlap = gm::overlap_as<gwamd_overlap>(o);
        return int32_t(0);
    });
}

} // extern "C"
