// What the C ABI entry points of include/gwamd_cudamapper.h share
// (mapper_batch.cpp, mapper_rescue_host.cpp, mapper_reads.cpp, mapper_batcher.cpp,
// mapper_index_cache.cpp): the error convention, the checks of
// packed reads and the hand-over of overlaps in a library-owned array.
#pragma once

#include "../../include/gwamd_cudamapper.h"
#include "mapper_common.hpp"

#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

namespace gwamd
{
namespace mapper
{

// 0 or f's result; std::invalid_argument becomes GWAMD_E_INVALID_ARGUMENT,
// anything else GWAMD_E_HIP or GWAMD_E_RUNTIME, with the message kept
template <typename F>
int32_t guarded_map(F&& f)
{
    try
    {
        gwamd::host::last_error().clear();
        return f();
    }
    catch (const std::invalid_argument& e)
    {
        gwamd::host::last_error() = e.what();
        return GWAMD_E_INVALID_ARGUMENT;
    }
    catch (const std::exception& e)
    {
        gwamd::host::last_error() = e.what();
        return std::string(e.what()).rfind("HIP error", 0) == 0 ? GWAMD_E_HIP : GWAMD_E_RUNTIME;
    }
}

inline void check_read_lengths(const int64_t* offsets, int64_t n)
{
    for (int64_t i = 0; i < n; i++)
    {
        if (offsets[i] < 0 || offsets[i] > offsets[i + 1])
            throw std::invalid_argument("read offsets must be non-decreasing");
        // a position and the direction share 32 bits of the sort payload
        if (offsets[i + 1] - offsets[i] >= (int64_t(1) << 31))
            throw std::invalid_argument("reads must be shorter than 2^31 bases");
    }
}

inline void clear_overlap_outputs(gwamd_overlap** overlaps, int64_t* num_overlaps, int64_t* num_anchors = nullptr)
{
    if (overlaps)
        *overlaps = nullptr;
    if (num_overlaps)
        *num_overlaps = 0;
    if (num_anchors)
        *num_anchors = 0;
}

template <typename Record>
void hand_over(const std::vector<Record>& records, gwamd_overlap** overlaps, int64_t* num_overlaps)
{
    static_assert(sizeof(Record) == sizeof(gwamd_overlap), "records are copied as bytes");
    if (records.empty())
        return;
    std::unique_ptr<gwamd_overlap[]> h(new gwamd_overlap[records.size()]);
    std::memcpy(static_cast<void*>(h.get()), static_cast<const void*>(records.data()),
                records.size() * sizeof(gwamd_overlap));
    *num_overlaps = int64_t(records.size());
    *overlaps     = h.release();
}

inline int32_t allocator_is_null(gwamd_overlap** overlaps, int64_t* num_overlaps, int64_t* num_anchors = nullptr)
{
    clear_overlap_outputs(overlaps, num_overlaps, num_anchors);
    gwamd::host::last_error() = "allocator is NULL";
    return GWAMD_E_INVALID_ARGUMENT;
}

} // namespace mapper
} // namespace gwamd
