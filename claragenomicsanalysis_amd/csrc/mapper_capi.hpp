// What the C ABI entry points of include/gwamd_cudamapper.h and
// include/gwamd_polish.h share (mapper_batch.cpp, mapper_rescue_host.cpp,
// mapper_reads.cpp, mapper_batcher.cpp, mapper_index_cache.cpp,
// overlap_align.cpp, paf_format.cpp, polish_windows_host.cpp): the error
// convention, the checks of packed reads, overlaps copied as bytes between
// their three types and the hand-over of records in a library-owned array.
#pragma once

#include <claraparabricks/genomeworks/cudamapper/types.hpp>

#include "../../include/gwamd_cudamapper.h"
#include "mapper_common.hpp"

#include <cstddef>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <type_traits>
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

// n >= 0 packed texts (reads or names): offsets there, from 0 or more, not falling
inline void check_offsets(const int64_t* off, int32_t n, const char* what)
{
    if (n < 0 || (n > 0 && !off))
        throw std::invalid_argument(std::string(what) + ": bad read count or offsets");
    for (int32_t i = 0; i < n; i++)
        if (off[i] > off[i + 1] || off[i] < 0)
            throw std::invalid_argument(std::string(what) + ": offsets must be non-decreasing");
}

inline void check_rescue_numbers(int32_t extension, float required_similarity)
{
    if (extension < 0 || extension > kMaxRescueExtension)
        throw std::invalid_argument("extension must be between 0 and " + std::to_string(kMaxRescueExtension) +
                                    ", got " + std::to_string(extension));
    if (required_similarity != required_similarity)
        throw std::invalid_argument("required_similarity is not a number");
}

// cudamapper::Overlap, gwamd_overlap and OverlapRecord are one layout: the
// fields before the strand are 32-bit words in all three
using CppOverlap = claraparabricks::genomeworks::cudamapper::Overlap;
static_assert(sizeof(CppOverlap) == sizeof(OverlapRecord) &&
                  offsetof(CppOverlap, relative_strand) == offsetof(OverlapRecord, relative_strand) &&
                  offsetof(CppOverlap, num_residues_) == offsetof(OverlapRecord, num_residues) &&
                  offsetof(CppOverlap, overlap_complete) == offsetof(OverlapRecord, overlap_complete),
              "OverlapRecord must match cudamapper::Overlap");
static_assert(sizeof(gwamd_overlap) == sizeof(OverlapRecord) &&
                  offsetof(gwamd_overlap, relative_strand) == offsetof(OverlapRecord, relative_strand) &&
                  offsetof(gwamd_overlap, num_residues) == offsetof(OverlapRecord, num_residues) &&
                  offsetof(gwamd_overlap, overlap_complete) == offsetof(OverlapRecord, overlap_complete),
              "gwamd_overlap must match cudamapper::Overlap");

template <typename T>
constexpr bool is_overlap_type = std::is_same<T, gwamd_overlap>::value || std::is_same<T, OverlapRecord>::value ||
                                 std::is_same<T, CppOverlap>::value;

// (the copies below are static: an instantiation on a type of the C ABI stays
// out of the library's dynamic symbols)

// one overlap as another of the three types
template <typename To, typename From>
static To overlap_as(const From& overlap)
{
    static_assert(is_overlap_type<To> && is_overlap_type<From>, "overlaps are copied as bytes");
    To out;
    std::memcpy(static_cast<void*>(&out), static_cast<const void*>(&overlap), sizeof(To));
    return out;
}

// n >= 0 overlaps of any of the three types as records, and back
template <typename T>
static std::vector<OverlapRecord> to_records(const T* overlaps, int64_t n)
{
    static_assert(is_overlap_type<T>, "overlaps are copied as bytes");
    std::vector<OverlapRecord> records(static_cast<size_t>(n));
    if (n > 0)
        std::memcpy(static_cast<void*>(records.data()), static_cast<const void*>(overlaps),
                    size_t(n) * sizeof(OverlapRecord));
    return records;
}

template <typename T>
static void from_records(const std::vector<OverlapRecord>& records, T* overlaps)
{
    static_assert(is_overlap_type<T>, "overlaps are copied as bytes");
    if (!records.empty())
        std::memcpy(static_cast<void*>(overlaps), static_cast<const void*>(records.data()),
                    records.size() * sizeof(OverlapRecord));
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

// `count` records of the same size as T, in host memory or on the current
// device, in an array the library owns; none: the outputs stay as they are
template <typename T, typename Record>
static void hand_over(const Record* records, size_t count, T** out, int64_t* num_out, bool from_device = false)
{
    static_assert(sizeof(Record) == sizeof(T), "records are copied as bytes");
    if (count == 0)
        return;
    std::unique_ptr<T[]> h(new T[count]);
    if (from_device)
        GWAMD_HIP_CHECK(hipMemcpy(h.get(), records, count * sizeof(T), hipMemcpyDeviceToHost));
    else
        std::memcpy(static_cast<void*>(h.get()), static_cast<const void*>(records), count * sizeof(T));
    *num_out = int64_t(count);
    *out     = h.release();
}

template <typename T, typename Record>
static void hand_over(const std::vector<Record>& records, T** out, int64_t* num_out)
{
    hand_over(records.data(), records.size(), out, num_out);
}

inline int32_t allocator_is_null(gwamd_overlap** overlaps, int64_t* num_overlaps, int64_t* num_anchors = nullptr)
{
    clear_overlap_outputs(overlaps, num_overlaps, num_anchors);
    gwamd::host::last_error() = "allocator is NULL";
    return GWAMD_E_INVALID_ARGUMENT;
}

} // namespace mapper
} // namespace gwamd

// the texts a call hands back (CIGARs, PAF lines, names, sequences)
struct gwamd_text_list
{
    std::vector<std::string> items;
};
