// Overlap regions gathered on the device into the aligner's sequence buffer
// (the layout AlignerGlobalHip::add_alignment fills on the host,
// aligner_batch.cpp): for overlap i, query[qs, qe) at seqs + 2i * stride and
// target[ts, te) at seqs + (2i + 1) * stride, the target reverse-complemented
// for a Reverse overlap as the aligner does it (genomeutils::reverse_complement:
// A<->T, C<->G, every other byte kept, every position complemented, the middle
// base of an odd length too, unlike the rescue), and the two lengths in lens.
//
// A byte mover.  The destination of a sequence, [A, A + len) with
// A = slot * stride, is cut into the 16-byte chunks of the buffer's own
// alignment, so a chunk that lies wholly inside the sequence is one aligned
// 16-byte store whatever the stride is.  Its 16 source bytes begin at any byte:
// they are taken as five aligned 32-bit words and brought into place with
// v_alignbyte, and for a Reverse target turned round with a byte swap and
// complemented four bytes at a time.  The first and last chunk of a sequence,
// where they stick out of it, are written byte by byte, so nothing outside
// [A, A + len) is ever written and neighbouring slots never meet.  The word
// loads reach at most 3 bytes before and 4 bytes after the region, which
// DeviceReads pads for (kReadsPad).  The chunk helpers are shared with the POA
// input gather (mapper_gather.hpp).
//
// One wave owns one piece of kPieceChunks chunks (4 KiB) of one sequence, a
// lane one chunk per step, so a 50 kb region is spread over a dozen waves and
// does not serialise a launch of 200-base ones.  A wave whose piece begins past
// its sequence's end leaves at once.  No LDS, no barrier.
#include "mapper_gather.hpp"
#include "mapper_prims.hpp"
#include "mapper_reads.hpp"

namespace gwamd
{
namespace mapper
{
namespace
{

constexpr uint32_t kWaves       = kThreads / 64;
constexpr uint32_t kOverlapWords = sizeof(OverlapRecord) / sizeof(uint32_t);

__global__ __launch_bounds__(kThreads) void gather_overlap_regions_kernel(
    const uint8_t* __restrict__ query_bases, const int64_t* __restrict__ query_offsets,
    const uint8_t* __restrict__ target_bases, const int64_t* __restrict__ target_offsets,
    const uint32_t* __restrict__ overlaps, uint32_t n, uint32_t stride, uint32_t pieces, uint8_t* __restrict__ seqs,
    int32_t* __restrict__ lens)
{
    const uint32_t lane  = threadIdx.x & 63;
    const uint64_t wave  = uint64_t(blockIdx.x) * kWaves + (threadIdx.x >> 6);
    const uint32_t slot  = uniform(uint32_t(wave / pieces)); // 2i: the query of overlap i, 2i + 1: its target
    const uint32_t piece = uniform(uint32_t(wave % pieces));
    if (slot >= 2 * n)
        return;
    const uint32_t* record = overlaps + size_t(slot >> 1) * kOverlapWords;
    const bool is_target   = slot & 1;
    const uint32_t read_id = uniform(record[is_target ? 1 : 0]);
    const uint32_t start   = uniform(record[is_target ? 3 : 2]);
    const uint32_t end     = uniform(record[is_target ? 5 : 4]);
    const bool reverse     = is_target && (uniform(record[6]) & 0xff) == '-';
    const uint32_t len     = end - start;
    const int64_t* offsets = is_target ? target_offsets : query_offsets;
    const uint32_t off_lo  = uniform(uint32_t(uint64_t(offsets[read_id])));
    const uint32_t off_hi  = uniform(uint32_t(uint64_t(offsets[read_id]) >> 32));
    const uint8_t* src = (is_target ? target_bases : query_bases) + ((uint64_t(off_hi) << 32) | off_lo) + start;

    if (piece == 0 && lane == 0)
        lens[slot] = int32_t(len);

    uint8_t* dst          = seqs + uint64_t(slot) * stride;      // byte j of the sequence goes to dst[j]
    const uint32_t lead   = uint32_t(reinterpret_cast<uintptr_t>(dst) & (kChunk - 1));
    const uint32_t chunks = (lead + len + kChunk - 1) / kChunk;  // chunk c holds bytes [16c - lead, 16c - lead + 16)
    for (uint32_t c = piece * kPieceChunks + lane; c < min(chunks, (piece + 1) * kPieceChunks); c += 64)
    {
        const int64_t j0 = int64_t(c) * kChunk - lead;
        if (j0 >= 0 && j0 + kChunk <= int64_t(len))
        {
            const uint32_t j = uint32_t(j0);
            uint4 v;
            if (!reverse)
                v = load16(src + j);
            else
            {
                // bytes j .. j + 15 of the reverse complement are source bytes len - 1 - j down to len - 16 - j
                const uint4 s = reverse16(load16(src + (len - kChunk - j)));
                v             = uint4{complement4(s.x), complement4(s.y), complement4(s.z), complement4(s.w)};
            }
            *reinterpret_cast<uint4*>(dst + j) = v;
        }
        else
        {
            const int64_t first = j0 < 0 ? 0 : j0;
            const int64_t last  = j0 + kChunk < int64_t(len) ? j0 + kChunk : int64_t(len);
            for (int64_t j = first; j < last; j++)
                dst[j] = reverse ? complement(src[len - 1 - uint32_t(j)]) : src[j];
        }
    }
}

} // namespace

void gather_overlap_regions(char* seqs, int32_t* lens, const OverlapRecord* d_overlaps, int64_t n, int64_t stride,
                            const DeviceReads& query, const DeviceReads& target, hipStream_t stream)
{
    if (n == 0)
        return;
    // a sequence of `stride` bytes that begins at any byte touches this many chunks at most
    const int64_t pieces = (stride + (kChunk - 1) + int64_t(kPieceChunks) * kChunk - 1) / (int64_t(kPieceChunks) * kChunk);
    const int64_t waves  = 2 * n * std::max<int64_t>(pieces, 1);
    const int64_t blocks = (waves + kWaves - 1) / kWaves;
    if (n >= (int64_t(1) << 31) || stride >= (int64_t(1) << 31) || blocks >= (int64_t(1) << 31))
        throw std::invalid_argument("gather_overlap_regions: too many overlaps for one launch");
    gather_overlap_regions_kernel<<<unsigned(blocks), kThreads, 0, stream>>>(
        query.bases(), query.d_offsets.data(), target.bases(), target.d_offsets.data(),
        reinterpret_cast<const uint32_t*>(d_overlaps), uint32_t(n), uint32_t(stride),
        uint32_t(std::max<int64_t>(pieces, 1)), reinterpret_cast<uint8_t*>(seqs), lens);
    check_launch();
}

} // namespace mapper
} // namespace gwamd
