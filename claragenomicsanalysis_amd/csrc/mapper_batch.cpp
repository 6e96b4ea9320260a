// Host side of cudamapper's minimizer index, anchor matcher and overlapper:
// the reference's C++ API (Index::create_index, Matcher::create_matcher,
// OverlapperTriggered::get_overlaps, Overlapper::post_process_overlaps;
// cudamapper/src/index.cu, matcher.cu, overlapper_triggered.cu, overlapper.cpp)
// and the C ABI of include/gwamd_cudamapper.h.  Device work is in
// mapper_index.hip, mapper_match.hip and mapper_overlap.hip.  Every argument
// is checked here, before any device call.
#include <claraparabricks/genomeworks/cudamapper/index.hpp>
#include <claraparabricks/genomeworks/cudamapper/matcher.hpp>
#include <claraparabricks/genomeworks/cudamapper/overlapper_triggered.hpp>

#include "allocator_handle.hpp"
#include "mapper_capi.hpp"
#include "mapper_index_impl.hpp"
#include "mapper_reads.hpp"

#include <cstddef>
#include <vector>

namespace gm = gwamd::mapper;
using gm::allocator_is_null;
using gm::check_read_lengths;
using gm::clear_overlap_outputs;
using gm::guarded_map;
using gm::hand_over;

namespace
{

void check_index_arguments(int64_t num_reads, int64_t first_read_id, int64_t past_the_last_read_id, uint64_t kmer_size,
                           uint64_t window_size, double filtering_parameter)
{
    if (kmer_size < 1 || kmer_size > uint64_t(gm::kMaxKmerSize))
        throw std::invalid_argument("kmer_size must be between 1 and " + std::to_string(gm::kMaxKmerSize) + ", got " +
                                    std::to_string(kmer_size));
    if (window_size < 1 || window_size > uint64_t(gm::kMaxWindowSize))
        throw std::invalid_argument("window_size must be between 1 and " + std::to_string(gm::kMaxWindowSize) +
                                    ", got " + std::to_string(window_size));
    if (!(filtering_parameter >= 0.0 && filtering_parameter <= 1.0))
        throw std::invalid_argument("filtering_parameter must be between 0 and 1");
    if (num_reads < 0 || first_read_id < 0 || first_read_id > past_the_last_read_id ||
        past_the_last_read_id > num_reads)
        throw std::invalid_argument("read range [" + std::to_string(first_read_id) + ", " +
                                    std::to_string(past_the_last_read_id) + ") is not within the " +
                                    std::to_string(num_reads) + " reads");
}

gm::OverlapParams check_overlap_parameters(int64_t min_residues, int64_t min_overlap_len,
                                           int64_t min_bases_per_residue, float min_overlap_fraction)
{
    // the reference converts the three integers to size_t
    if (min_residues < 0 || min_overlap_len < 0 || min_bases_per_residue < 0)
        throw std::invalid_argument("min_residues, min_overlap_len and min_bases_per_residue must not be negative");
    if (min_overlap_fraction != min_overlap_fraction)
        throw std::invalid_argument("min_overlap_fraction is not a number");
    return gm::OverlapParams{min_residues, min_overlap_len, min_bases_per_residue, min_overlap_fraction};
}

void check_anchor_count(int64_t n)
{
    if (n < 0 || n > gm::kDefaultMaxAnchors)
        throw std::invalid_argument("the number of anchors must be between 0 and 2^31, got " + std::to_string(n));
}

} // namespace

namespace claraparabricks
{
namespace genomeworks
{
namespace cudamapper
{
namespace
{

class MatcherHip : public Matcher
{
public:
    static_assert(sizeof(Anchor) == sizeof(gm::AnchorRecord), "Anchor is four u32");
    gm::DevBuf<gm::AnchorRecord> data;
    device_buffer<Anchor> view;
    device_buffer<Anchor>& anchors() override { return view; }
};

std::unique_ptr<IndexHip> make_index(const char* bases, const int64_t* offsets, uint32_t first_read_id,
                                     uint32_t num_reads, int kmer_size, int window_size, bool hash_representations,
                                     double filtering_parameter, const gm::Budget& budget, hipStream_t stream)
{
    auto index = std::make_unique<IndexHip>();
    if (num_reads > 0)
    {
        GWAMD_HIP_CHECK(hipGetDevice(&index->data.device_id));
        gm::build_index(index->data, bases, offsets, first_read_id, num_reads, kmer_size, window_size,
                        hash_representations, filtering_parameter, budget, stream);
    }
    index->refresh_views();
    return index;
}

} // namespace

std::unique_ptr<Index> Index::create_index(DefaultDeviceAllocator allocator, const io::FastaParser& parser,
                                           const read_id_t first_read_id, const read_id_t past_the_last_read_id,
                                           const std::uint64_t kmer_size, const std::uint64_t window_size,
                                           const bool hash_representations, const double filtering_parameter,
                                           const hipStream_t stream)
{
    check_index_arguments(parser.get_num_seqences(), first_read_id, past_the_last_read_id, kmer_size, window_size,
                          filtering_parameter);
    const uint32_t n = past_the_last_read_id - first_read_id;
    const gm::PackedReads packed(parser, first_read_id, past_the_last_read_id);
    check_read_lengths(packed.offsets.data(), n);
    return make_index(packed.bases.data(), packed.offsets.data(), first_read_id, n, int(kmer_size), int(window_size),
                      hash_representations, filtering_parameter, allocator.budget(), stream);
}

std::unique_ptr<Matcher> Matcher::create_matcher(DefaultDeviceAllocator allocator, const Index& query_index,
                                                 const Index& target_index, const hipStream_t stream)
{
    const auto* q = dynamic_cast<const IndexHip*>(&query_index);
    const auto* t = dynamic_cast<const IndexHip*>(&target_index);
    if (!q || !t)
        throw std::invalid_argument("create_matcher takes indices made by Index::create_index");
    auto m = std::make_unique<MatcherHip>();
    gm::match_anchors(m->data, q->data, t->data, gm::kDefaultMaxAnchors, allocator.budget(), stream);
    m->view = {reinterpret_cast<Anchor*>(m->data.data()), std::ptrdiff_t(m->data.size())};
    return m;
}

OverlapperTriggered::OverlapperTriggered(DefaultDeviceAllocator allocator, const hipStream_t stream)
    : allocator_(allocator)
    , stream_(stream)
{
}

void OverlapperTriggered::get_overlaps(std::vector<Overlap>& fused_overlaps, const device_buffer<Anchor>& d_anchors,
                                       int64_t min_residues, int64_t min_overlap_len, int64_t min_bases_per_residue,
                                       float min_overlap_fraction)
{
    const gm::OverlapParams params =
        check_overlap_parameters(min_residues, min_overlap_len, min_bases_per_residue, min_overlap_fraction);
    check_anchor_count(d_anchors.size());
    std::vector<gm::OverlapRecord> records;
    gm::get_overlaps(records, reinterpret_cast<const gm::AnchorRecord*>(d_anchors.data()), d_anchors.size(), params,
                     allocator_.budget(), stream_);
    fused_overlaps.resize(records.size());
    gm::from_records(records, fused_overlaps.data());
}

namespace
{

int32_t abs_of(uint32_t difference) // abs(int) of a difference of two positions
{
    const int32_t d = int32_t(difference);
    return d < 0 ? int32_t(0u - difference) : d;
}

// whether overlap b can be fused to its predecessor a (overlaps_mergable, overlapper.cpp:29-91)
bool mergeable(const Overlap& a, const Overlap& b)
{
    const bool forward = a.relative_strand == RelativeStrand::Forward && b.relative_strand == RelativeStrand::Forward;
    const bool reverse = a.relative_strand == RelativeStrand::Reverse && b.relative_strand == RelativeStrand::Reverse;
    if (!forward && !reverse)
        return false;
    if (a.query_read_id_ != b.query_read_id_ || a.target_read_id_ != b.target_read_id_)
        return false;
    const int32_t query_gap = abs_of(b.query_start_position_in_read_ - a.query_end_position_in_read_);
    // on the reverse strand the target positions fall while the query positions rise
    const int32_t target_gap = reverse ? abs_of(a.target_start_position_in_read_ - b.target_end_position_in_read_)
                                       : abs_of(b.target_start_position_in_read_ - a.target_end_position_in_read_);
    if (query_gap < 500 && target_gap < 500)
        return true;
    // float32 quotients compared with double constants, as the reference writes them
    const float gap_ratio = float(std::min(query_gap, target_gap)) / float(std::max(query_gap, target_gap));
    if (gap_ratio > 0.8)
        return true;
    const uint32_t query_length = (a.query_end_position_in_read_ - a.query_start_position_in_read_) +
                                  (b.query_end_position_in_read_ - b.query_start_position_in_read_);
    const uint32_t target_length = (a.target_end_position_in_read_ - a.target_start_position_in_read_) +
                                   (b.target_end_position_in_read_ - b.target_start_position_in_read_);
    return float(query_gap) / float(query_length) < 0.2 && float(target_gap) / float(target_length) < 0.2;
}

} // namespace

void Overlapper::post_process_overlaps(std::vector<Overlap>& overlaps, const bool drop_fused_overlaps)
{
    const size_t n = overlaps.size();
    std::vector<bool> fused(drop_fused_overlaps ? n : 0);
    std::vector<Overlap> added;
    bool in_fuse = false;
    Overlap fusion{}; // the overlap before the current one, with the fusion's span and residues
    uint32_t query_start = 0, query_end = 0, target_start = 0, target_end = 0, residues = 0;
    const auto close = [&] {
        fusion.query_start_position_in_read_  = query_start;
        fusion.query_end_position_in_read_    = query_end;
        fusion.target_start_position_in_read_ = target_start;
        fusion.target_end_position_in_read_   = target_end;
        fusion.num_residues_                  = residues;
        added.push_back(fusion);
    };
    for (size_t i = 1; i < n; i++)
    {
        const Overlap& prev = overlaps[i - 1];
        const Overlap& cur  = overlaps[i];
        // the reference copies the other fields of a fusion from the overlap
        // before the last one it looked at: the fusion's last overlap when the
        // next one ends it, its last but one when the list ends in it
        fusion = prev;
        if (mergeable(prev, cur))
        {
            if (drop_fused_overlaps)
                fused[i] = fused[i - 1] = true;
            const bool is_forward = cur.relative_strand == RelativeStrand::Forward;
            if (!in_fuse)
            {
                in_fuse      = true;
                residues     = prev.num_residues_ + cur.num_residues_;
                query_start  = prev.query_start_position_in_read_;
                query_end    = cur.query_end_position_in_read_;
                target_start = is_forward ? prev.target_start_position_in_read_ : cur.target_start_position_in_read_;
                target_end   = is_forward ? cur.target_end_position_in_read_ : prev.target_end_position_in_read_;
            }
            else
            {
                residues += cur.num_residues_;
                query_end = cur.query_end_position_in_read_;
                if (is_forward)
                    target_end = cur.target_end_position_in_read_;
                else
                    target_start = cur.target_start_position_in_read_;
            }
        }
        else if (in_fuse)
        {
            in_fuse = false;
            close();
        }
    }
    if (in_fuse)
        close();
    if (drop_fused_overlaps)
    {
        // drop_overlaps_by_mask: the mask covers the overlaps that came in
        size_t kept = 0;
        for (size_t i = 0; i < n; i++)
            if (!fused[i])
                overlaps[kept++] = overlaps[i];
        overlaps.resize(kept);
    }
    overlaps.insert(overlaps.end(), added.begin(), added.end());
}

} // namespace cudamapper
} // namespace genomeworks
} // namespace claraparabricks

// ---- C ABI ------------------------------------------------------------------

namespace cm = claraparabricks::genomeworks::cudamapper;

static_assert(sizeof(gwamd_anchor) == sizeof(gm::AnchorRecord), "gwamd_anchor must match cudamapper::Anchor");

namespace
{

int32_t index_create(const char* bases, const int64_t* offsets, int32_t num_reads, int32_t first_read_id,
                     int32_t past_the_last_read_id, int32_t kmer_size, int32_t window_size,
                     int32_t hash_representations, double filtering_parameter, int32_t device_id,
                     const gm::Budget& budget, gwamd_index** out)
{
    if (out)
        *out = nullptr;
    return guarded_map([&] {
        if (!out)
            throw std::invalid_argument("out is NULL");
        if (kmer_size < 0 || window_size < 0)
            throw std::invalid_argument("kmer_size and window_size must be positive");
        check_index_arguments(num_reads, first_read_id, past_the_last_read_id, uint64_t(kmer_size),
                              uint64_t(window_size), filtering_parameter);
        if (num_reads > 0 && (!offsets || (!bases && offsets[num_reads] > 0)))
            throw std::invalid_argument("bases or offsets is NULL");
        if (device_id < 0)
            throw std::invalid_argument("device_id must not be negative");
        check_read_lengths(offsets, num_reads);
        auto h           = std::make_unique<gwamd_index>();
        const uint32_t n = uint32_t(past_the_last_read_id - first_read_id);
        if (n == 0)
        {
            h->impl = std::make_unique<cm::IndexHip>();
            h->impl->data.device_id = device_id;
        }
        else
        {
            gwamd::host::ScopedDevice dev(device_id);
            h->impl = cm::make_index(bases, offsets + first_read_id, uint32_t(first_read_id), n, kmer_size,
                                     window_size, hash_representations != 0, filtering_parameter, budget, nullptr);
        }
        *out = h.release();
        return int32_t(0);
    });
}

int32_t match(const gwamd_index* query_index, const gwamd_index* target_index, int64_t max_anchors,
              const gm::Budget& budget, gwamd_anchor** anchors, int64_t* num_anchors)
{
    if (anchors)
        *anchors = nullptr;
    if (num_anchors)
        *num_anchors = 0;
    return guarded_map([&] {
        if (!query_index || !target_index || !anchors || !num_anchors)
            throw std::invalid_argument("index, anchors or num_anchors is NULL");
        if (max_anchors < -1)
            throw std::invalid_argument("max_anchors must be -1 (the default of 2^31) or not negative");
        const gm::IndexData& q = query_index->impl->data;
        const gm::IndexData& t = target_index->impl->data;
        if (q.representations.size() == 0 || t.representations.size() == 0)
            return int32_t(0);
        if (q.device_id != t.device_id)
            throw std::invalid_argument("the two indices are on different devices");
        gwamd::host::ScopedDevice dev(q.device_id);
        gm::DevBuf<gm::AnchorRecord> d;
        gm::match_anchors(d, q, t, max_anchors < 0 ? gm::kDefaultMaxAnchors : max_anchors, budget, nullptr);
        hand_over(d.data(), d.size(), anchors, num_anchors, true);
        return int32_t(0);
    });
}

int32_t overlaps_of_anchors(const gwamd_anchor* anchors, int64_t n, int64_t min_residues, int64_t min_overlap_len,
                            int64_t min_bases_per_residue, float min_overlap_fraction, int32_t device_id,
                            const gm::Budget& budget, gwamd_overlap** overlaps, int64_t* num_overlaps)
{
    clear_overlap_outputs(overlaps, num_overlaps);
    return guarded_map([&] {
        if (!overlaps || !num_overlaps)
            throw std::invalid_argument("overlaps or num_overlaps is NULL");
        const gm::OverlapParams params =
            check_overlap_parameters(min_residues, min_overlap_len, min_bases_per_residue, min_overlap_fraction);
        check_anchor_count(n);
        if (n > 0 && !anchors)
            throw std::invalid_argument("anchors is NULL");
        if (device_id < 0)
            throw std::invalid_argument("device_id must not be negative");
        if (n == 0)
            return int32_t(0);
        gwamd::host::ScopedDevice dev(device_id);
        gm::DevBuf<gm::AnchorRecord> d(size_t(n), budget);
        GWAMD_HIP_CHECK(hipMemcpy(d.data(), anchors, size_t(n) * sizeof(gwamd_anchor), hipMemcpyHostToDevice));
        std::vector<gm::OverlapRecord> records;
        gm::get_overlaps(records, d.data(), n, params, budget, nullptr);
        hand_over(records, overlaps, num_overlaps);
        return int32_t(0);
    });
}

int32_t match_overlaps(const gwamd_index* query_index, const gwamd_index* target_index, int64_t max_anchors,
                       int64_t min_residues, int64_t min_overlap_len, int64_t min_bases_per_residue,
                       float min_overlap_fraction, const gm::Budget& budget, gwamd_overlap** overlaps,
                       int64_t* num_overlaps, int64_t* num_anchors)
{
    clear_overlap_outputs(overlaps, num_overlaps, num_anchors);
    return guarded_map([&] {
        if (!query_index || !target_index || !overlaps || !num_overlaps)
            throw std::invalid_argument("index, overlaps or num_overlaps is NULL");
        if (max_anchors < -1)
            throw std::invalid_argument("max_anchors must be -1 (the default of 2^31) or not negative");
        const gm::OverlapParams params =
            check_overlap_parameters(min_residues, min_overlap_len, min_bases_per_residue, min_overlap_fraction);
        const gm::IndexData& q = query_index->impl->data;
        const gm::IndexData& t = target_index->impl->data;
        if (q.representations.size() == 0 || t.representations.size() == 0)
            return int32_t(0);
        if (q.device_id != t.device_id)
            throw std::invalid_argument("the two indices are on different devices");
        gwamd::host::ScopedDevice dev(q.device_id);
        gm::DevBuf<gm::AnchorRecord> d;
        gm::match_anchors(d, q, t, max_anchors < 0 ? gm::kDefaultMaxAnchors : max_anchors, budget, nullptr);
        std::vector<gm::OverlapRecord> records;
        gm::get_overlaps(records, d.data(), int64_t(d.size()), params, budget, nullptr);
        hand_over(records, overlaps, num_overlaps);
        if (num_anchors)
            *num_anchors = int64_t(d.size());
        return int32_t(0);
    });
}

template <typename T>
void copy_out(T* dst, const gm::DevBuf<T>& src)
{
    if (dst && src.size() > 0)
        GWAMD_HIP_CHECK(hipMemcpy(dst, src.data(), src.size() * sizeof(T), hipMemcpyDeviceToHost));
}

} // namespace

extern "C" {

int32_t gwamd_index_create(const char* bases, const int64_t* offsets, int32_t num_reads, int32_t first_read_id,
                           int32_t past_the_last_read_id, int32_t kmer_size, int32_t window_size,
                           int32_t hash_representations, double filtering_parameter, int32_t device_id,
                           gwamd_index** out)
{
    return index_create(bases, offsets, num_reads, first_read_id, past_the_last_read_id, kmer_size, window_size,
                        hash_representations, filtering_parameter, device_id, nullptr, out);
}

int32_t gwamd_index_create_with_allocator(const char* bases, const int64_t* offsets, int32_t num_reads,
                                          int32_t first_read_id, int32_t past_the_last_read_id, int32_t kmer_size,
                                          int32_t window_size, int32_t hash_representations,
                                          double filtering_parameter, int32_t device_id,
                                          gwamd_device_allocator* allocator, gwamd_index** out)
{
    if (!allocator)
    {
        if (out)
            *out = nullptr;
        gwamd::host::last_error() = "allocator is NULL";
        return GWAMD_E_INVALID_ARGUMENT;
    }
    return index_create(bases, offsets, num_reads, first_read_id, past_the_last_read_id, kmer_size, window_size,
                        hash_representations, filtering_parameter, device_id, allocator->alloc.budget(), out);
}

void gwamd_index_free(gwamd_index* index) { delete index; }

int32_t gwamd_index_info(const gwamd_index* index, gwamd_index_info_t* info)
{
    return guarded_map([&] {
        if (!index || !info)
            throw std::invalid_argument("index or info is NULL");
        const gm::IndexData& d                    = index->impl->data;
        info->num_elements                        = int64_t(d.representations.size());
        info->num_unique_representations          = int64_t(d.unique_representations.size());
        info->number_of_reads                     = d.number_of_reads;
        info->smallest_read_id                    = d.smallest_read_id;
        info->largest_read_id                     = d.largest_read_id;
        info->number_of_basepairs_in_longest_read = d.number_of_basepairs_in_longest_read;
        return int32_t(0);
    });
}

int32_t gwamd_index_copy(const gwamd_index* index, uint64_t* representations, uint32_t* read_ids,
                         uint32_t* positions_in_reads, uint8_t* directions_of_reads,
                         uint64_t* unique_representations, uint32_t* first_occurrence_of_representations)
{
    return guarded_map([&] {
        if (!index)
            throw std::invalid_argument("index is NULL");
        const gm::IndexData& d = index->impl->data;
        if (d.representations.size() == 0)
            return int32_t(0);
        gwamd::host::ScopedDevice dev(d.device_id);
        copy_out(representations, d.representations);
        copy_out(read_ids, d.read_ids);
        copy_out(positions_in_reads, d.positions_in_reads);
        copy_out(directions_of_reads, d.directions_of_reads);
        copy_out(unique_representations, d.unique_representations);
        copy_out(first_occurrence_of_representations, d.first_occurrence_of_representations);
        return int32_t(0);
    });
}

int32_t gwamd_match_anchors(const gwamd_index* query_index, const gwamd_index* target_index, int64_t max_anchors,
                            gwamd_anchor** anchors, int64_t* num_anchors)
{
    return match(query_index, target_index, max_anchors, nullptr, anchors, num_anchors);
}

int32_t gwamd_match_anchors_with_allocator(const gwamd_index* query_index, const gwamd_index* target_index,
                                           int64_t max_anchors, gwamd_device_allocator* allocator,
                                           gwamd_anchor** anchors, int64_t* num_anchors)
{
    if (!allocator)
    {
        if (anchors)
            *anchors = nullptr;
        if (num_anchors)
            *num_anchors = 0;
        gwamd::host::last_error() = "allocator is NULL";
        return GWAMD_E_INVALID_ARGUMENT;
    }
    return match(query_index, target_index, max_anchors, allocator->alloc.budget(), anchors, num_anchors);
}

void gwamd_anchors_free(gwamd_anchor* anchors) { delete[] anchors; }

int32_t gwamd_get_overlaps(const gwamd_anchor* anchors, int64_t n, int64_t min_residues, int64_t min_overlap_len,
                           int64_t min_bases_per_residue, float min_overlap_fraction, int32_t device_id,
                           gwamd_overlap** overlaps, int64_t* num_overlaps)
{
    return overlaps_of_anchors(anchors, n, min_residues, min_overlap_len, min_bases_per_residue,
                               min_overlap_fraction, device_id, nullptr, overlaps, num_overlaps);
}

int32_t gwamd_get_overlaps_with_allocator(const gwamd_anchor* anchors, int64_t n, int64_t min_residues,
                                          int64_t min_overlap_len, int64_t min_bases_per_residue,
                                          float min_overlap_fraction, int32_t device_id,
                                          gwamd_device_allocator* allocator, gwamd_overlap** overlaps,
                                          int64_t* num_overlaps)
{
    if (!allocator)
        return allocator_is_null(overlaps, num_overlaps);
    return overlaps_of_anchors(anchors, n, min_residues, min_overlap_len, min_bases_per_residue,
                               min_overlap_fraction, device_id, allocator->alloc.budget(), overlaps, num_overlaps);
}

int32_t gwamd_match_overlaps(const gwamd_index* query_index, const gwamd_index* target_index, int64_t max_anchors,
                             int64_t min_residues, int64_t min_overlap_len, int64_t min_bases_per_residue,
                             float min_overlap_fraction, gwamd_overlap** overlaps, int64_t* num_overlaps,
                             int64_t* num_anchors)
{
    return match_overlaps(query_index, target_index, max_anchors, min_residues, min_overlap_len,
                          min_bases_per_residue, min_overlap_fraction, nullptr, overlaps, num_overlaps, num_anchors);
}

int32_t gwamd_match_overlaps_with_allocator(const gwamd_index* query_index, const gwamd_index* target_index,
                                            int64_t max_anchors, int64_t min_residues, int64_t min_overlap_len,
                                            int64_t min_bases_per_residue, float min_overlap_fraction,
                                            gwamd_device_allocator* allocator, gwamd_overlap** overlaps,
                                            int64_t* num_overlaps, int64_t* num_anchors)
{
    if (!allocator)
        return allocator_is_null(overlaps, num_overlaps, num_anchors);
    return match_overlaps(query_index, target_index, max_anchors, min_residues, min_overlap_len,
                          min_bases_per_residue, min_overlap_fraction, allocator->alloc.budget(), overlaps,
                          num_overlaps, num_anchors);
}

int32_t gwamd_post_process_overlaps(const gwamd_overlap* in, int64_t n, int32_t drop_fused_overlaps,
                                    gwamd_overlap** out, int64_t* num_out)
{
    clear_overlap_outputs(out, num_out);
    return guarded_map([&] {
        if (!out || !num_out)
            throw std::invalid_argument("out or num_out is NULL");
        if (n < 0)
            throw std::invalid_argument("the number of overlaps must not be negative");
        if (n > 0 && !in)
            throw std::invalid_argument("in is NULL");
        std::vector<cm::Overlap> overlaps(static_cast<size_t>(n));
        gm::from_records(gm::to_records(in, n), overlaps.data());
        cm::Overlapper::post_process_overlaps(overlaps, drop_fused_overlaps != 0);
        hand_over(overlaps, out, num_out);
        return int32_t(0);
    });
}

void gwamd_overlaps_free(gwamd_overlap* overlaps) { delete[] overlaps; }

} // extern "C"
