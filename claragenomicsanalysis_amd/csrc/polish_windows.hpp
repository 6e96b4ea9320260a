// Internal declarations of cudapolish's window cut (polish_windows.hip: the
// kernel and its launch; polish_windows_host.cpp: the checks, the record
// layout, the host walk, the one cut launch, the cut on the aligner's device
// paths through the engines of overlap_engines.hpp, the grouping and the C ABI).
#pragma once

#include "../../include/gwamd_polish.h"
#include "mapper_common.hpp"

#include <cstdint>
#include <vector>

namespace gwamd
{
namespace mapper
{
struct DeviceReads;
}
namespace polish
{

using gwamd::mapper::Budget;
using gwamd::mapper::OverlapRecord;

constexpr int kCutWaves      = 4;    // waves per workgroup, one overlap each
constexpr int kCutTileStates = 1024; // states a wave covers in one step: 64 lanes x 16 bytes

// Where the kernel finds path i of a launch: bytes [A, A + lengths[i]) of
// paths with A = offsets ? offsets[i] : (first + i) * stride.  paths is
// 16-byte aligned and paths_bytes its allocation: a 16-byte chunk that would
// cross its end is read as the 32-bit words that lie inside it.
struct PathSource
{
    const int8_t* paths      = nullptr; // device
    int64_t paths_bytes      = 0;
    const int64_t* offsets   = nullptr; // device, or null for strided paths
    int64_t stride           = 0;
    int64_t first            = 0;
    const int32_t* lengths   = nullptr; // device
    int32_t max_length       = 0;       // a longer (or negative) length is a path that does not fit
    bool end_to_start        = false;   // the aligner's order
};

// n = the number of overlaps of the launch; d_overlaps their records,
// d_record_base[i] the index of overlap i's first record in d_records (8
// words each, zeroed by the caller), d_status[i] receives 0 or 1 (the path
// does not fit).  The kernel stores q_begin, q_end, t_begin, t_end of the
// windows that hold a match or mismatch state; complete_records does the
// rest on the host.  Asynchronous on stream.
void launch_window_cut(const PathSource& source, const OverlapRecord* d_overlaps, const uint32_t* d_record_base,
                       gwamd_window_segment* d_records, uint32_t* d_status, int64_t n, int32_t window_length,
                       hipStream_t stream);

// The layout of a call's records: counts per overlap and their exclusive sum
struct RecordLayout
{
    std::vector<uint32_t> base; // n + 1 entries
    int64_t total() const { return int64_t(base.back()); }
};

// Throws std::invalid_argument for window_length <= 0 and for more than 2^31 records.
RecordLayout plan_records(const OverlapRecord* overlaps, int64_t n, int32_t window_length);

// The `count` records of one overlap as the kernel left them, completed on the
// host: overlap, window, flags and the reserved word; a record no state
// touched becomes empty.  With flag != 0 (GWAMD_SEGMENT_BAD_PATH or
// GWAMD_SEGMENT_NOT_ALIGNED) every record becomes empty with that flag.
void complete_records(gwamd_window_segment* records, uint32_t count, uint32_t index, const OverlapRecord& overlap,
                      int32_t window_length, uint32_t flag);

// The records of one overlap from its states (start -> end), on the host
void walk_on_host(gwamd_window_segment* records, uint32_t count, uint32_t index, const OverlapRecord& overlap,
                  const int8_t* states, int64_t num_states, int32_t window_length);

// The checked overlaps aligned on resident reads by num_alignment_engines
// engines (overlap_engines.hpp) and cut on each aligner's stream from its
// device paths; out receives every record, completed.
void window_segments_resident(const gwamd::mapper::DeviceReads& query, const gwamd::mapper::DeviceReads& target,
                              const OverlapRecord* overlaps, int32_t n, int32_t window_length,
                              int32_t num_alignment_engines, std::vector<gwamd_window_segment>& out);

} // namespace polish
} // namespace gwamd
