// The aligner host's plan: length limits, the LDS and workspace-slot layouts
// the kernels index by, the slot count and what each launch runs, as pure
// functions of the capacities, the device's facts and the tuning switches.
// No HIP in here (aligner_plan.cpp), so a plan can be examined, and sanitized,
// on the host: gwamd_internal_aligner_plan.
#pragma once

#include "aligner_common.hpp"
#include "aligner_tuning.hpp"

#include <cstdint>

namespace gwamd
{
namespace aln
{

// Algorithms (GWAMD_ALIGNER_* of include/gwamd_cudaaligner.h)
constexpr int kAlgoHm = 0, kAlgoMyers = 1, kAlgoBanded = 2, kAlgoUkkonen = 3;

// long mode: target letter codes in LDS up to kHmLdsTarget bases, in HBM beyond
constexpr int32_t kHmMaxQuery  = 1 << 24;
constexpr int32_t kHmMaxTarget = 1 << 24;
constexpr int32_t kHmLdsTarget = 131072;
// full Myers: one pair's (word, column) state (0.375 B per cell) per slot
constexpr int64_t kMyersMaxSlot   = int64_t(32) << 30;
constexpr int64_t kMyersWorkspace = int64_t(64) << 30; // resident slots within 64 GiB of the 288 GB HBM
// Hirschberg-Myers takes the LDS-resident kernel (hm_kernel<false>, patterns in
// LDS, register-resident sweeps of up to 4 blocks per half) up to these sizes
constexpr int32_t kHmShortQuery  = 16384;
constexpr int32_t kHmShortTarget = 65535;
constexpr int64_t kHmWorkspace   = int64_t(16) << 30; // resident slots within 16 GiB of the 288 GB HBM
constexpr int kMaxStages         = 8;    // pipeline stages of align_all(), at most
constexpr int kLongBandQuery     = 8192; // banded Myers: longer queries run 8 waves per pair
constexpr int kMaxSpecSweeps     = 8;    // banded Myers sweeps run ahead, at most
constexpr int kDefaultSpecSweeps = 5;    // est x 1 .. x 16
constexpr int kLdsPerCu          = 163840;

// Which kernel: the key of the kernel table (aligner_kernels.hip, aligner_banded.hip)
struct KernelKey
{
    int32_t algo;
    int32_t long_mode;  // Hirschberg-Myers, full Myers: hm_kernel<true>, myers_kernel<true>
    int32_t band_waves; // banded Myers: myers_banded_kernel<1 | 4 | 8 | 16>
    int32_t uk_threads; // Ukkonen: > 0 is ukkonen_wide_kernel with this many threads
};
struct KernelRef
{
    const void* fn; // nullptr: the table has no such kernel
    int threads;
};

// What the plan needs to know of the device
struct DeviceFacts
{
    int32_t cus         = 1;
    int32_t per_cu      = 1; // resident workgroups per CU of AlignerPlan::occupancy_key at args.lds_bytes
    int32_t wide_per_cu = 1; // of ukkonen_wide_kernel (1,024 threads, uk_wide_lds), asked when AlignerPlan::uk_wide
    int64_t free_bytes  = 0; // free device memory
};

struct AlignerPlan
{
    int32_t algo = 0;
    Args args{};              // every field but the pointers and n: the layout the kernels index by
    int64_t slot_bytes  = 0;  // one workspace slot (args.ws_slot_bytes)
    int64_t fixed_bytes = 0;  // sequences, lengths, paths, counters: every device array but the workspace
    int32_t uk_wide_lds = 0;  // Ukkonen: LDS image of ukkonen_wide_kernel (args.lds_bytes is ukkonen_kernel's)
    bool uk_wide        = false; // Ukkonen: the widest allowed band needs ukkonen_wide_kernel
    bool band_waves_forced = false; // GWAMD_BAND_WAVES
    int32_t spec_forced = -1; // GWAMD_BAND_SPEC (banded Myers), -1: not given
    KernelKey occupancy_key{}; // the kernel whose occupancy decides the grid
};

struct SlotPlan
{
    int32_t slots    = 1; // workspace slots = workgroups of the persistent grid
    int32_t resident = 1; // banded aligners: workgroups resident at once
    int32_t cus      = 1;
};

struct LaunchPlan
{
    KernelKey key{};
    // what this launch changes in the plan's Args
    int32_t uk_threads = 0, lds_bytes = 0, lds_tile_off = 0, tile_bytes = 0, band_waves = 1;
    int32_t spec_sweeps = 0; // > 0: two launches (spec_phase 1 on grid[0], spec_phase 2 on grid[1])
    int32_t grid[2]     = {0, 0};
};

// Length limits of this implementation (include/gwamd_cudaaligner.h)
struct AlignerLimits
{
    int32_t max_query, max_target;
};
AlignerLimits aligner_limits(int algo);
// Why an aligner of these capacities cannot be built ("" when it can): the
// length limits, the Ukkonen band bound and the full-Myers slot bound.
std::string aligner_limit_error(int algo, int32_t max_q, int32_t max_t);
inline bool aligner_pair_fits(int algo, int32_t max_q, int32_t max_t)
{
    return aligner_limit_error(algo, max_q, max_t).empty();
}
// ukkonen_max_score_matrix_size (ukkonen_gpu.cu:313-324): band rows for a length difference
inline int32_t ukkonen_band_rows(int32_t diff) { return (1 + diff + 2 * kUkkonenP + 1) / 2; }
// aligner_global_ukkonen.cpp:23,32: float 0.1 times max_target_length, truncated
inline int32_t ukkonen_max_difference(int32_t max_t) { return int32_t(float(max_t) * 0.1f); }

// Workspace slot of the full Myers aligner; the offsets may be null.
int64_t myers_slot_layout(int32_t max_q, int32_t max_t, int64_t* hbuf_off, int64_t* pat_off, int64_t* tcod_off);

// Everything of the plan that needs no device.  Throws std::invalid_argument
// for capacities past the limits, an LDS image that does not fit, and switches
// of this algorithm that are out of range.
AlignerPlan plan_layout(int algo, int32_t max_q, int32_t max_t, int32_t max_n, const AlignerTuning& tuning);
// Slots: what is resident, within the workspace caps, then GWAMD_ALIGNER_GRID, then at most max_n.
SlotPlan plan_slots(const AlignerPlan& plan, const DeviceFacts& facts, int32_t max_n, const AlignerTuning& tuning);
// banded Myers with more than one wave planned: the launch depends on the longest query of its pairs
inline bool launch_needs_max_query(const AlignerPlan& p)
{
    return p.algo == kAlgoBanded && p.args.band_waves > 1 && !p.band_waves_forced;
}
// One launch of `count` pairs on `nslots` slots: max_query_in_range is the
// longest query among them (read only when launch_needs_max_query), max_diff
// the batch's largest |query - target|.
LaunchPlan plan_launch(const AlignerPlan& plan, const SlotPlan& sp, int32_t count, int32_t nslots,
                       int32_t max_query_in_range, int32_t max_diff);
// Pipeline stages of align_all() for n pairs: as many (up to kMaxStages) as
// keep each stage's half of the slots busy four times over; 1 = one stage.
int pipeline_stages(int32_t slots, int32_t n, const AlignerTuning& tuning);

} // namespace aln
} // namespace gwamd
