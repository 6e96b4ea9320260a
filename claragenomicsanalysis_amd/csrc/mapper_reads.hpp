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
// gather_overlap_regions_kernel and gather_poa_slices_kernel read the bases
// (the latter the qualities too) as aligned 32-bit words, five per 16 bytes
// they write: a word may begin up to 3 bytes before a region and end up to 4
// bytes after it, so both ends of each buffer are padded.
constexpr size_t kReadsPad = 16;

struct DeviceReads
{
    DevBuf<uint8_t> storage;      // kReadsPad, the bases, up to 15 bytes to a multiple of 16, kReadsPad
    DevBuf<uint8_t> qual_storage; // the quality characters in the same layout, when the set has them
    DevBuf<int64_t> d_offsets;    // num_reads + 1
    std::vector<int64_t> offsets; // the host's copy: lengths are checked without a device call
    int device_id      = 0;
    bool has_qualities = false;

    const uint8_t* bases() const { return storage.data() + kReadsPad; }
    // quality character of base i at qualities()[i]; null for a set without qualities
    const uint8_t* qualities() const { return has_qualities ? qual_storage.data() + kReadsPad : nullptr; }
    int64_t num_reads() const { return int64_t(offsets.size()) - 1; }
    int64_t num_bases() const { return offsets.back(); }
    int64_t read_length(uint32_t id) const { return offsets[size_t(id) + 1] - offsets[id]; }
};

// The reads on the current device, which is device_id, with their quality
// characters (one per base, at the base's own offset) unless qualities is
// null.  The arguments are validated by the caller (check_read_set,
// check_qualities).
std::unique_ptr<DeviceReads> make_device_reads(const ReadSet& reads, const char* qualities, int device_id,
                                               const Budget& budget, hipStream_t stream);
inline std::unique_ptr<DeviceReads> make_device_reads(const ReadSet& reads, int device_id, const Budget& budget,
                                                      hipStream_t stream)
{
    return make_device_reads(reads, nullptr, device_id, budget, stream);
}

// Throws std::invalid_argument for a negative count, a NULL array with
// something to read, offsets that fall and a read of 2^31 bases or more.
void check_read_set(const char* side, const ReadSet& reads);

// Throws std::invalid_argument unless every quality character of the checked
// reads, qualities[offsets[0], offsets[num_reads]), is a printable 33..126
// (Phred + 33), and for NULL qualities with a base to describe.
void check_qualities(const ReadSet& reads, const char* qualities);

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
    std::string qualities; // filled by pack_qualities
    explicit PackedReads(const claraparabricks::genomeworks::io::FastaParser& parser);
    PackedReads(const claraparabricks::genomeworks::io::FastaParser& parser, uint32_t first, uint32_t past_the_last);
    ReadSet view() const { return {bases.data(), offsets.data(), int64_t(offsets.size()) - 1}; }
    // The parser's quality strings packed like the bases.  Throws std::invalid_argument
    // for a record whose quality string has not its sequence's length.
    void pack_qualities(const claraparabricks::genomeworks::io::FastaParser& parser);
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
