// The alignment engines of the overlap-alignment caller (overlap_align.cpp;
// reference cudamapper/src/main.cu:48-175), for its own entry points and for
// cudapolish's cut on the aligner's device paths (polish_windows_host.cpp).
//
// num_alignment_engines host threads, each with its own stream and aligner,
// pull [start, start + batch) ranges of the pairs within the aligner's limits
// from a shared counter and hand each range to a job: add() puts the pairs into
// the aligner, align_all() runs, finish() takes the results.  The first
// exception stops every engine and is rethrown by run_engines.
#pragma once

#include <claraparabricks/genomeworks/cudaaligner/aligner.hpp>

#include "aligner_resident.hpp"

#include <cstdint>
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>

namespace gwamd
{
namespace aln
{

struct PairLengths
{
    int32_t query;
    int32_t target;
};

// One of the two steps of a job on the pairs kept[start, end) and the aligner
// of the engine that drew them.  Engines call it concurrently, on ranges that
// do not meet.
using RangeFn = std::function<void(claraparabricks::genomeworks::cudaaligner::Aligner&, int32_t start, int32_t end)>;

struct EngineJob
{
    RangeFn add;
    // after align_all(): with keep_paths_on_device it reads device_paths()
    // and no sync_alignments() is called, otherwise it calls it itself
    RangeFn finish;
    bool keep_paths_on_device = false;
};

// The indices of the pairs within the aligner's limits
// (gwamd_aligner_max_lengths; the reference has none), ascending.  The others
// are left unaligned, with a warning on stderr, so that one long overlap does
// not fail the whole call.
std::vector<int32_t> pairs_within_limits(const std::vector<PairLengths>& lengths);

// Pairs per engine batch (main.cu:150-156): 0.03 B per cell of the largest
// pair against 85 % of the free device memory, split among the engines, capped
// so that an engine stages at most 1 GiB on the host, and at least 1.  The
// batch size has no effect on results.
int64_t engine_batch_size(int32_t n, int32_t max_query_size, int32_t max_target_size, int32_t num_alignment_engines,
                          size_t free_bytes);

// Runs the job over kept (from pairs_within_limits(lengths)) on the current
// device, with aligners sized for the longest kept pair (main.cu:125-175).
// Throws std::runtime_error for num_alignment_engines < 1.
void run_engines(const std::vector<PairLengths>& lengths, const std::vector<int32_t>& kept,
                 int32_t num_alignment_engines, const EngineJob& job);

inline void check_added(claraparabricks::genomeworks::cudaaligner::StatusType status)
{
    if (status != claraparabricks::genomeworks::cudaaligner::StatusType::success)
        throw std::runtime_error("Experienced error type " + std::to_string(int(status)));
}

// The overlaps of a call on resident reads (checked by the caller): the
// lengths of all n, the indices of those within the aligner's limits and
// their records, contiguous, which is what add() hands ranges of to
// add_device_overlaps.
struct ResidentOverlaps
{
    std::vector<PairLengths> lengths;
    std::vector<int32_t> kept;
    std::vector<gwamd::mapper::OverlapRecord> kept_records;

    ResidentOverlaps(const gwamd::mapper::OverlapRecord* overlaps, int32_t n);
    // (the three outlive the job)
    RangeFn add(const gwamd::mapper::DeviceReads& query, const gwamd::mapper::DeviceReads& target) const;
};

} // namespace aln
} // namespace gwamd
