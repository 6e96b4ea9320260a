// The reads of a parser resident on a device.  The reference has no such
// class: its rescue_overlap_ends and align_overlaps read the parser on the host
// for every call (cudamapper/src/overlapper.cpp:295-365, main.cu:48-175).  A
// caller that runs those stages once per pair of indices uploads the reads once
// with DeviceReads::create and passes the object to
// Overlapper::rescue_overlap_ends (overlapper.hpp) and align_overlaps
// (overlap_alignment.hpp), which then move only the overlaps.
#pragma once

#include <claraparabricks/genomeworks/io/fasta_parser.hpp>
#include <claraparabricks/genomeworks/types.hpp>
#include <claraparabricks/genomeworks/utils/allocator.hpp>

#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <memory>

namespace claraparabricks
{
namespace genomeworks
{
namespace cudamapper
{

class DeviceReads
{
public:
    /// Every read of parser, in parser order, on the current device: the
    /// packed bases and number_of_reads() + 1 offsets.  The device bytes are
    /// counted against the allocator's pool for the object's lifetime.
    /// Throws std::invalid_argument for a read of 2^31 bases or more.
    static std::unique_ptr<DeviceReads> create(DefaultDeviceAllocator allocator, const io::FastaParser& parser,
                                               hipStream_t stream = 0);
    /// The same with the parser's quality strings (FastaParser::get_quality_by_id)
    /// in a second device array of the bases' layout, for
    /// cudapolish::add_poa_group_resident's base weights.  Throws
    /// std::invalid_argument unless every record has one quality character in
    /// 33..126 per base (a FASTA record has none).
    struct with_qualities_t
    {
    };
    static std::unique_ptr<DeviceReads> create(DefaultDeviceAllocator allocator, const io::FastaParser& parser,
                                               with_qualities_t, hipStream_t stream = 0);
    ~DeviceReads();
    DeviceReads(const DeviceReads&) = delete;
    DeviceReads& operator=(const DeviceReads&) = delete;

    number_of_reads_t number_of_reads() const;
    std::int64_t number_of_basepairs() const;
    /// The device the reads are on.
    std::int32_t device_id() const;
    bool has_qualities() const;

    struct Impl;
    const Impl& impl() const { return *impl_; }

private:
    DeviceReads();
    std::unique_ptr<Impl> impl_;
};

} // namespace cudamapper
} // namespace genomeworks
} // namespace claraparabricks

namespace claragenomics = claraparabricks::genomeworks;
