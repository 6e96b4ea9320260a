// Internal declarations of cudapolish's window cut (polish_windows.hip: the
// kernel on state paths and its launch; polish_cigar.hip: the kernel on CIGAR
// runs and its launch; polish_windows_host.cpp: the checks, the record
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

constexpr int kCigarTileOps           = 64; // CIGAR ops a wave covers in one step: a lane one op
constexpr uint32_t kCigarOwnCrossings = 2;  // window boundaries inside a match run its own lane walks

// Where the CIGAR kernel (polish_cigar.hip) finds the ops of overlap i of a
// launch: words [offsets[i], offsets[i + 1]) of ops, each length << 4 | op in
// BAM numbering, normalised to this project's convention and to path order
// (normalised_op).  num_ops is the allocation in words.
struct CigarSource
{
    const uint32_t* ops    = nullptr; // device
    int64_t num_ops        = 0;
    const int64_t* offsets = nullptr; // device, n + 1 entries
};

// launch_window_cut for CIGAR runs in place of states: the same records, status and stream order
void launch_window_cut_cigar(const CigarSource& source, const OverlapRecord* d_overlaps, const uint32_t* d_record_base,
                             gwamd_window_segment* d_records, uint32_t* d_status, int64_t n, int32_t window_length,
                             hipStream_t stream);

// Op j of the `count` ops of an overlap as the walks take it: a SAM CIGAR
// (GWAMD_CIGAR_SAM) has I and D exchanged and, for a '-' overlap, its order reversed.
inline uint32_t normalised_op(const uint32_t* ops, int64_t count, int64_t j, bool sam, bool reverse)
{
    if (!sam)
        return ops[j];
    const uint32_t op   = ops[reverse ? count - 1 - j : j];
    const uint32_t code = op & 15;
    return code == 1 || code == 2 ? op ^ 3 : op;
}

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

// The records of one overlap from its CIGAR ops in either convention, on the
// host: a walk over runs and the windows they cross, never over bases
void walk_cigar_on_host(gwamd_window_segment* records, uint32_t count, uint32_t index, const OverlapRecord& overlap,
                        const uint32_t* ops, int64_t num_ops, bool sam, int32_t window_length);

// The checked overlaps aligned on resident reads by num_alignment_engines
// engines (overlap_engines.hpp) and cut on each aligner's stream from its
// device paths; out receives every record, completed.
void window_segments_resident(const gwamd::mapper::DeviceReads& query, const gwamd::mapper::DeviceReads& target,
                              const OverlapRecord* overlaps, int32_t n, int32_t window_length,
                              int32_t num_alignment_engines, std::vector<gwamd_window_segment>& out);

} // namespace polish
} // namespace gwamd
