// Overlap-alignment caller of the global aligner (reference
// cudamapper/src/main.cu:48-175): the alignment engines (overlap_engines.hpp)
// and the four entry points that align overlaps into CIGARs, on reads in host
// memory and on reads resident on the device, in C++ and in the C ABI.
//
// Engines: num_alignment_engines host threads, each with its own HIP stream and
// aligner, pull [start, start + batch) ranges of the overlap list from a shared
// counter, add the overlap regions (target reverse-complemented for Reverse
// overlaps), align, and store the CIGARs at the overlaps' indices, so the
// output order is the overlap order whatever the thread interleaving.
#include <claraparabricks/genomeworks/cudaaligner/aligner.hpp>
#include <claraparabricks/genomeworks/cudamapper/overlap_alignment.hpp>

#include "../../include/gwamd_cudaaligner.h"
#include "mapper_capi.hpp"
#include "mapper_reads.hpp"
#include "overlap_engines.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <exception>
#include <iostream>
#include <mutex>
#include <thread>

namespace gwamd
{
namespace aln
{

namespace ca = claraparabricks::genomeworks::cudaaligner;

std::vector<int32_t> pairs_within_limits(const std::vector<PairLengths>& lengths)
{
    int32_t lim_q = 0, lim_t = 0;
    gwamd_aligner_max_lengths(GWAMD_ALIGNER_HIRSCHBERG_MYERS, &lim_q, &lim_t);
    const int32_t n = int32_t(lengths.size());
    std::vector<int32_t> kept;
    kept.reserve(lengths.size());
    for (int32_t i = 0; i < n; i++)
        if (lengths[size_t(i)].query <= lim_q && lengths[size_t(i)].target <= lim_t)
            kept.push_back(i);
    if (int32_t(kept.size()) != n)
        std::cerr << "align_overlaps: " << n - int32_t(kept.size())
                  << " overlap(s) longer than the aligner's limits (query " << lim_q << ", target " << lim_t
                  << " bases) left without a CIGAR" << std::endl;
    return kept;
}

int64_t engine_batch_size(int32_t n, int32_t max_query_size, int32_t max_target_size, int32_t num_alignment_engines,
                          size_t free_bytes)
{
    // Bound on the host staging of one engine's batch (the aligner keeps pinned
    // copies of every pair it holds)
    constexpr int64_t kMaxStagingBytes = int64_t(1) << 30;
    const float memory_per_base        = 0.03f;
    const float memory_per_alignment = std::max(1.0f, memory_per_base * float(max_query_size) * float(max_target_size));
    const size_t max_alignments      = size_t((float(free_bytes) * 85 / 100) / memory_per_alignment);
    int64_t batch_size = std::min<int64_t>(n, int64_t(std::min<size_t>(max_alignments, INT32_MAX))) /
                         num_alignment_engines;
    const int64_t per_pair = 2 * int64_t(std::max(max_query_size, max_target_size)) + max_query_size +
                             max_target_size + 16;
    batch_size = std::min<int64_t>(batch_size, std::max<int64_t>(1, kMaxStagingBytes / per_pair));
    // the reference loops forever on a zero batch size (fewer overlaps than engines)
    return std::max<int64_t>(batch_size, 1);
}

void run_engines(const std::vector<PairLengths>& lengths, const std::vector<int32_t>& kept,
                 int32_t num_alignment_engines, const EngineJob& job)
{
    if (num_alignment_engines < 1)
        throw std::runtime_error("num_alignment_engines must be at least 1");
    const int32_t n = int32_t(kept.size());
    if (n == 0)
        return;
    int32_t max_query_size = 0, max_target_size = 0;
    for (int32_t i : kept)
    {
        max_query_size  = std::max(max_query_size, lengths[size_t(i)].query);
        max_target_size = std::max(max_target_size, lengths[size_t(i)].target);
    }
    int device_id = 0;
    GWAMD_HIP_CHECK(hipGetDevice(&device_id));
    size_t free_mem = 0, total_mem = 0;
    GWAMD_HIP_CHECK(hipMemGetInfo(&free_mem, &total_mem));
    const int64_t batch_size =
        engine_batch_size(n, max_query_size, max_target_size, num_alignment_engines, free_mem);
    std::cerr << "Aligning " << n << " overlaps (" << max_query_size << "x" << max_target_size
              << ") with batch size " << batch_size << std::endl;

    std::mutex idx_mtx;
    int32_t next = 0;
    std::vector<std::exception_ptr> errors(static_cast<size_t>(num_alignment_engines));
    auto engine = [&](int32_t e) {
        try
        {
            gwamd::host::ScopedDevice dev(device_id);
            gwamd::host::OwnedStream stream;
            auto aligner = ca::create_aligner(max_query_size, max_target_size, int32_t(batch_size),
                                              ca::AlignmentType::global_alignment,
                                              claraparabricks::genomeworks::DefaultDeviceAllocator(), stream,
                                              device_id);
            if (job.keep_paths_on_device)
                keep_paths_on_device(*aligner, true);
            while (true)
            {
                int32_t start = 0, end = 0;
                {
                    std::lock_guard<std::mutex> lk(idx_mtx);
                    if (next == n)
                        break;
                    start = next;
                    end   = int32_t(std::min<int64_t>(int64_t(start) + batch_size, n));
                    next  = end;
                }
                job.add(*aligner, start, end);
                aligner->align_all();
                job.finish(*aligner, start, end);
                aligner->reset();
            }
        }
        catch (...)
        {
            errors[size_t(e)] = std::current_exception();
            std::lock_guard<std::mutex> lk(idx_mtx);
            next = n; // stop the other engines
        }
    };
    std::vector<std::thread> threads;
    for (int32_t e = 0; e < num_alignment_engines; e++)
        threads.emplace_back(engine, e);
    for (auto& t : threads)
        t.join();
    for (auto& ep : errors)
        if (ep)
            std::rethrow_exception(ep);
}

ResidentOverlaps::ResidentOverlaps(const gwamd::mapper::OverlapRecord* overlaps, int32_t n)
    : lengths(static_cast<size_t>(n))
{
    for (int32_t i = 0; i < n; i++)
        lengths[size_t(i)] = {int32_t(overlaps[i].query_end - overlaps[i].query_start),
                              int32_t(overlaps[i].target_end - overlaps[i].target_start)};
    kept = pairs_within_limits(lengths);
    kept_records.reserve(kept.size());
    for (int32_t i : kept)
        kept_records.push_back(overlaps[i]);
}

RangeFn ResidentOverlaps::add(const gwamd::mapper::DeviceReads& query, const gwamd::mapper::DeviceReads& target) const
{
    return [this, &query, &target](ca::Aligner& aligner, int32_t start, int32_t end) {
        check_added(add_device_overlaps(aligner, query, target, kept_records.data() + start, end - start));
    };
}

} // namespace aln
} // namespace gwamd

namespace gm = gwamd::mapper;
namespace ga = gwamd::aln;

namespace
{

namespace ca = claraparabricks::genomeworks::cudaaligner;

// One overlap's two regions in host memory
struct Region
{
    const char* query;
    const char* target;
    bool reverse;
};

// finish: the CIGAR of the pair kept[k] to cigars[kept[k]]
ga::RangeFn store_cigars(const std::vector<int32_t>& kept, std::vector<std::string>& cigars)
{
    return [&kept, &cigars](ca::Aligner& aligner, int32_t start, int32_t) {
        aligner.sync_alignments();
        const auto& alignments = aligner.get_alignments();
        for (size_t i = 0; i < alignments.size(); i++)
            cigars[size_t(kept[size_t(start) + i])] = alignments[i]->convert_to_cigar();
    };
}

// n overlaps whose regions are in host memory, added to the aligners one by one
void align_regions(const std::vector<Region>& regions, const std::vector<ga::PairLengths>& lengths,
                   int32_t num_alignment_engines, std::vector<std::string>& cigars)
{
    const std::vector<int32_t> kept = ga::pairs_within_limits(lengths);
    cigars.assign(lengths.size(), std::string());
    const ga::RangeFn add = [&](ca::Aligner& aligner, int32_t start, int32_t end) {
        for (int32_t k = start; k < end; k++)
        {
            const size_t i = size_t(kept[size_t(k)]);
            ga::check_added(aligner.add_alignment(regions[i].query, lengths[i].query, regions[i].target,
                                                  lengths[i].target, false, regions[i].reverse));
        }
    };
    ga::run_engines(lengths, kept, num_alignment_engines, {add, store_cigars(kept, cigars), false});
}

// align_overlaps on n checked records whose reads are resident on the current device
void align_resident(const gm::DeviceReads& query, const gm::DeviceReads& target, const gm::OverlapRecord* records,
                    int32_t n, int32_t num_alignment_engines, std::vector<std::string>& cigars)
{
    const ga::ResidentOverlaps pairs(records, n);
    cigars.assign(size_t(n), std::string());
    ga::run_engines(pairs.lengths, pairs.kept, num_alignment_engines,
                    {pairs.add(query, target), store_cigars(pairs.kept, cigars), false});
}

void check_range(uint32_t start, uint32_t end, size_t length, const char* what)
{
    if (start > end || end > length)
        throw std::invalid_argument(std::string("overlap ") + what + " range outside its read");
}

} // namespace

namespace claraparabricks
{
namespace genomeworks
{
namespace cudamapper
{

// This entry keeps a check of its own: it neither looks at the strand (anything
// but Reverse is aligned forward) nor at the ids (the parser's concern).
void align_overlaps(DefaultDeviceAllocator /*allocator*/, std::vector<Overlap>& overlaps,
                    const io::FastaParser& query_parser, const io::FastaParser& target_parser,
                    int32_t num_alignment_engines, std::vector<std::string>& cigars)
{
    if (overlaps.size() > size_t(INT32_MAX))
        throw std::invalid_argument("too many overlaps for one call");
    std::vector<Region> regions;
    std::vector<ga::PairLengths> lengths;
    regions.reserve(overlaps.size());
    lengths.reserve(overlaps.size());
    for (const Overlap& o : overlaps)
    {
        const std::string& q = query_parser.get_sequence_by_id(o.query_read_id_).seq;
        const std::string& t = target_parser.get_sequence_by_id(o.target_read_id_).seq;
        check_range(o.query_start_position_in_read_, o.query_end_position_in_read_, q.size(), "query");
        check_range(o.target_start_position_in_read_, o.target_end_position_in_read_, t.size(), "target");
        regions.push_back({q.data() + o.query_start_position_in_read_, t.data() + o.target_start_position_in_read_,
                           o.relative_strand == RelativeStrand::Reverse});
        lengths.push_back({int32_t(o.query_end_position_in_read_ - o.query_start_position_in_read_),
                           int32_t(o.target_end_position_in_read_ - o.target_start_position_in_read_)});
    }
    align_regions(regions, lengths, num_alignment_engines, cigars);
}

void align_overlaps(DefaultDeviceAllocator /*allocator*/, std::vector<Overlap>& overlaps,
                    const DeviceReads& query_reads, const DeviceReads& target_reads, int32_t num_alignment_engines,
                    std::vector<std::string>& cigars)
{
    if (overlaps.size() > size_t(INT32_MAX))
        throw std::invalid_argument("too many overlaps for one call");
    const gm::DeviceReads& query  = *query_reads.impl().reads;
    const gm::DeviceReads& target = *target_reads.impl().reads;
    const std::vector<gm::OverlapRecord> records = gm::to_records(overlaps.data(), int64_t(overlaps.size()));
    gm::check_overlaps(query, target, records.data(), int64_t(records.size()));
    if (num_alignment_engines < 1)
        throw std::runtime_error("num_alignment_engines must be at least 1");
    cigars.clear();
    if (records.empty())
        return;
    gm::check_on_current_device(query, target);
    align_resident(query, target, records.data(), int32_t(records.size()), num_alignment_engines, cigars);
}

} // namespace cudamapper
} // namespace genomeworks
} // namespace claraparabricks

// ---- C ABI ------------------------------------------------------------------

extern "C" {

// The reads are checked by check_offsets, not check_read_set: this entry takes
// reads of 2^31 bases and more, and NULL bases, as it always has.
int32_t gwamd_align_overlaps(const char* query_bases, const int64_t* query_offsets, int32_t num_queries,
                             const char* target_bases, const int64_t* target_offsets, int32_t num_targets,
                             const gwamd_overlap* overlaps, int32_t num_overlaps, int32_t num_alignment_engines,
                             int32_t device_id, gwamd_text_list** cigars)
{
    *cigars = nullptr;
    return gm::guarded_map([&] {
        gm::check_offsets(query_offsets, num_queries, "queries");
        gm::check_offsets(target_offsets, num_targets, "targets");
        const std::vector<gm::OverlapRecord> records = gm::to_records(overlaps, std::max(num_overlaps, 0));
        gm::check_overlaps(query_offsets, num_queries, target_offsets, num_targets, records.data(),
                           int64_t(records.size()));
        auto list = std::make_unique<gwamd_text_list>();
        if (num_overlaps == 0)
        {
            *cigars = list.release();
            return 0;
        }
        gwamd::host::ScopedDevice dev(device_id);
        if (num_overlaps < 0) // GWAMD_E_RUNTIME here, after the device is set, not an invalid argument
            throw std::runtime_error("the number of overlaps must not be negative");
        std::vector<Region> regions;
        std::vector<ga::PairLengths> lengths;
        for (const gm::OverlapRecord& o : records)
        {
            regions.push_back({query_bases + query_offsets[o.query_read_id] + o.query_start,
                               target_bases + target_offsets[o.target_read_id] + o.target_start,
                               o.relative_strand == '-'});
            lengths.push_back({int32_t(o.query_end - o.query_start), int32_t(o.target_end - o.target_start)});
        }
        align_regions(regions, lengths, num_alignment_engines, list->items);
        *cigars = list.release();
        return 0;
    });
}

int32_t gwamd_align_overlaps_resident(const gwamd_device_reads* query_reads, const gwamd_device_reads* target_reads,
                                      const gwamd_overlap* overlaps, int32_t n, int32_t num_alignment_engines,
                                      gwamd_text_list** cigars)
{
    if (cigars)
        *cigars = nullptr;
    return gm::guarded_map([&] {
        if (!cigars)
            throw std::invalid_argument("cigars is NULL");
        if (!query_reads || !target_reads)
            throw std::invalid_argument("query_reads or target_reads is NULL");
        gm::check_overlap_count(overlaps, n);
        const std::vector<gm::OverlapRecord> records = gm::to_records(overlaps, n);
        gm::check_overlaps(*query_reads->reads, *target_reads->reads, records.data(), n);
        if (num_alignment_engines < 1)
            throw std::runtime_error("num_alignment_engines must be at least 1");
        auto list = std::make_unique<gwamd_text_list>();
        if (n > 0)
        {
            gm::check_on_current_device(*query_reads->reads, *target_reads->reads);
            align_resident(*query_reads->reads, *target_reads->reads, records.data(), n, num_alignment_engines,
                           list->items);
        }
        *cigars = list.release();
        return 0;
    });
}

} // extern "C"
