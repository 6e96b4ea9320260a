// The reads of one parser resident on a device (mapper_reads.cpp): packed bases
// and n + 1 offsets, uploaded once and then read in place by the overlap-end
// rescue (mapper_rescue.hip) and by the gather of overlap regions into the
// aligner's sequence buffer (mapper_gather.hip).  Also what every caller checks
// its reads and overlaps with, on the host, before any device call.
#pragma once

#include <claraparabricks/genomeworks/cudamapper/device_reads.hpp>

#include "mapper_common.hpp"

#include <cstdint>
#include <memory>
#include <string>
#include <vector>

namespace gwamd
{
namespace mapper
{

// Bytes allocated, and zeroed, before the first base and after the last one.
// gather_overlap_regions_kernel reads the bases as aligned 32-bit words, five
// per 16 bytes it writes: a word may begin up to 3 bytes before a region and
// end up to 4 bytes after it, so both ends of the buffer are padded.
constexpr size_t kReadsPad = 16;

struct DeviceReads
{
    DevBuf<uint8_t> storage;      // kReadsPad, the bases, up to 15 bytes to a multiple of 16, kReadsPad
    DevBuf<int64_t> d_offsets;    // num_reads + 1
    std::vector<int64_t> offsets; // the host's copy: lengths are checked without a device call
    int device_id = 0;

    const uint8_t* bases() const { return storage.data() + kReadsPad; }
    int64_t num_reads() const { return int64_t(offsets.size()) - 1; }
    int64_t num_bases() const { return offsets.back(); }
    int64_t read_length(uint32_t id) const { return offsets[size_t(id) + 1] - offsets[id]; }
};

// The reads on the current device, which is device_id.  The arguments are
// validated by the caller (check_read_set).
std::unique_ptr<DeviceReads> make_device_reads(const ReadSet& reads, int device_id, const Budget& budget,
                                               hipStream_t stream);

// Throws std::invalid_argument for a negative count, a NULL array with
// something to read, offsets that fall and a read of 2^31 bases or more.
void check_read_set(const char* side, const ReadSet& reads);

// Throws std::invalid_argument for a count outside [0, 2^31) and for NULL overlaps with n > 0.
void check_overlap_count(const void* overlaps, int64_t n);

// The above, and throws std::invalid_argument unless every overlap names reads
// of the two sets (their n + 1 offsets and counts, checked by the caller), has
// start <= end <= read length on both and a strand of '+' or '-'.
void check_overlaps(const int64_t* query_offsets, int64_t num_queries, const int64_t* target_offsets,
                    int64_t num_targets, const OverlapRecord* overlaps, int64_t n);
inline void check_overlaps(const ReadSet& query, const ReadSet& target, const OverlapRecord* overlaps, int64_t n)
{
    check_overlaps(query.offsets, query.num_reads, target.offsets, target.num_reads, overlaps, n);
}
inline void check_overlaps(const DeviceReads& query, const DeviceReads& target, const OverlapRecord* overlaps, int64_t n)
{
    check_overlaps(query.offsets.data(), query.num_reads(), target.offsets.data(), target.num_reads(), overlaps, n);
}

// The last check of a call on resident reads, the only one that asks the
// runtime: throws std::invalid_argument unless both are on the current device.
void check_on_current_device(const DeviceReads& query, const DeviceReads& target);

// The reads [first, past_the_last) of a parser (all of them by default) packed
// into bases and n + 1 offsets that begin at 0
struct PackedReads
{
    std::string bases;
    std::vector<int64_t> offsets;
    explicit PackedReads(const claraparabricks::genomeworks::io::FastaParser& parser);
    PackedReads(const claraparabricks::genomeworks::io::FastaParser& parser, uint32_t first, uint32_t past_the_last);
    ReadSet view() const { return {bases.data(), offsets.data(), int64_t(offsets.size()) - 1}; }
};

// rescue_overlap_ends on reads that are resident: only the overlaps travel.
void rescue_overlap_ends(OverlapRecord* overlaps, int64_t n, const DeviceReads& query, const DeviceReads& target,
                         int extension, float required_similarity, const Budget& budget, hipStream_t stream);

// Overlap i of the n device records: query[qs, qe) to seqs + 2i * stride,
// target[ts, te) to seqs + (2i + 1) * stride, reverse-complemented as the
// aligner does it (A<->T, C<->G, every position) when the strand is '-', and
// the two lengths to lens[2i] and lens[2i + 1].  Asynchronous on stream.  The
// caller has checked the overlaps and that no region is longer than stride.
void gather_overlap_regions(char* seqs, int32_t* lens, const OverlapRecord* d_overlaps, int64_t n, int64_t stride,
                            const DeviceReads& query, const DeviceReads& target, hipStream_t stream);

} // namespace mapper
} // namespace gwamd

// what the public class (device_reads.hpp) and the C handle (gwamd_cudamapper.h) hold
struct claraparabricks::genomeworks::cudamapper::DeviceReads::Impl
{
    std::unique_ptr<gwamd::mapper::DeviceReads> reads;
};

struct gwamd_device_reads
{
    std::unique_ptr<gwamd::mapper::DeviceReads> reads;
};
