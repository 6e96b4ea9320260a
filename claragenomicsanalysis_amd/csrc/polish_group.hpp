// Internal declarations of cudapolish's window grouping on the device
// (polish_group.hip: the kernels and their launch; polish_group_host.cpp: the
// checks, the upload of given segments, the fused cut-then-group route and the
// C ABI).  The grouping is group_slices' (polish_windows_host.cpp), array for
// array.
#pragma once

#include "polish_windows.hpp"

#include <cstdint>
#include <vector>

// The handle of gwamd_build_window_slices, gwamd_build_window_slices_device and
// gwamd_window_slices_resident: the arrays of gwamd_window_slices_view
struct gwamd_window_slices
{
    std::vector<gwamd_read_slice> slices;
    std::vector<int32_t> window_counts;
    std::vector<uint32_t> window_target, window_index;
    std::vector<int32_t> sequence_overlap, sequence_t_begin, sequence_t_end;
    int64_t dropped_by_cap = 0, dropped_by_quality = 0;
};

namespace gwamd
{
namespace polish
{

// What the grouping reads, all of it on the device.  Two kinds of record array:
//
//   completed  records as gwamd_window_segment defines them, in any order:
//              overlap, window and flags are read from the record itself
//              (record_base, status and status_slot are null);
//   raw        records as the cut kernels leave them, where plan_records puts
//              them: overlap i owns records [record_base[i], record_base[i + 1])
//              of windows target_start / w upwards, and contributes nothing
//              when status_slot[i] is kNotAligned or status[status_slot[i]] is
//              not 0.  A record no state touched has q_end == 0.
struct GroupInput
{
    const gwamd_window_segment* records = nullptr;
    int64_t num_records                 = 0;
    const OverlapRecord* overlaps       = nullptr;
    int64_t num_overlaps                = 0;
    const uint32_t* record_base         = nullptr; // num_overlaps + 1, raw records only
    const uint32_t* status              = nullptr; // raw records only
    const uint32_t* status_slot         = nullptr; // num_overlaps, raw records only
    const int64_t* target_offsets       = nullptr; // num_targets + 1
    const uint32_t* window_first        = nullptr; // num_targets + 1: the first window of every target
    int64_t num_targets                 = 0;
    int64_t num_windows                 = 0;       // window_first[num_targets], below 2^31
    const int64_t* query_offsets        = nullptr; // num_queries + 1; read with qualities only
    const uint8_t* query_qualities      = nullptr; // DeviceReads::qualities(), or null: no filter
    int32_t quality_threshold_tenths    = 0;
    int32_t window_length               = 0;
    int32_t max_sequences_per_window    = 0;
};

constexpr uint32_t kNotAligned = 0xffffffffu;

using GroupOutput = ::gwamd_window_slices;

// The windows of the input, grouped on the current device: the scratch arrays
// are counted against budget, only the grouped arrays come back.  Returns after
// the stream has been synchronized.  The caller has checked every argument:
// the kernels trust ids, windows and query ranges of the records that count.
void group_on_device(const GroupInput& in, GroupOutput& out, const Budget& budget, hipStream_t stream);

} // namespace polish
} // namespace gwamd
