// Slices of resident reads gathered into a POA batch's packed input arrays
// (polish_gather.hpp): for sequence i, bases[dst, dst + len) and
// wts[dst, dst + len) with dst its seq_off.  Sequences are packed back to back,
// so two of them routinely share a 16-byte chunk.
//
// A byte mover, the sibling of gather_overlap_regions_kernel (mapper_gather.hip)
// and built from the same parts (mapper_gather.hpp).  The destination
// [A, A + len) is cut into the 16-byte chunks of the buffer's own alignment; a
// chunk that lies wholly inside the sequence is one aligned 16-byte store to
// each array, its 16 source bytes taken as five aligned 32-bit words and
// brought into place with v_alignbyte.  The first and last chunk, where they
// stick out of the sequence, are written byte by byte: no byte outside
// [A, A + len) is ever written, so the neighbour that owns the rest of such a
// chunk, whichever wave or copy writes it and whenever, is not disturbed.  The
// word loads reach at most 3 bytes before and 4 bytes after the slice, which
// DeviceReads pads for in both of its arrays (kReadsPad).
//
// Bases are copied, or for a reverse slice turned round and complemented four
// bytes at a time.  Weights are quality - 33: a whole chunk holds 16 quality
// characters, each at least 33 (checked when the reads were made), so one
// 32-bit subtraction of 0x21212121 does four of them without a borrow between
// bytes; for a reverse slice they are turned round, not complemented.  A slice
// of a set without qualities gets the constant 1.
//
// One wave owns one piece of kPieceChunks chunks (4 KiB) of one sequence, a
// lane one chunk per step.  A wave whose piece begins past its sequence's end,
// or whose slice is empty, leaves at once.  No LDS, no barrier.
#include "mapper_gather.hpp"
#include "mapper_prims.hpp"
#include "polish_gather.hpp"

namespace gwamd
{
namespace polish
{
namespace
{

using namespace gwamd::mapper;

constexpr uint32_t kWaves    = kThreads / 64;
constexpr uint32_t kJobWords = sizeof(SliceJob) / sizeof(uint32_t);
constexpr uint32_t kQualZero = 0x21212121u; // '!' in every byte

__device__ inline uint4 minus_qual_zero(uint4 v)
{
    return uint4{v.x - kQualZero, v.y - kQualZero, v.z - kQualZero, v.w - kQualZero};
}

__global__ __launch_bounds__(kThreads) void gather_poa_slices_kernel(const uint32_t* __restrict__ jobs, uint32_t n,
                                                                     uint32_t pieces, uint8_t* __restrict__ seqs,
                                                                     uint8_t* __restrict__ wts)
{
    const uint32_t lane  = threadIdx.x & 63;
    const uint64_t wave  = uint64_t(blockIdx.x) * kWaves + (threadIdx.x >> 6);
    const uint32_t seq   = uniform(uint32_t(wave / pieces));
    const uint32_t piece = uniform(uint32_t(wave % pieces));
    if (seq >= n)
        return;
    const uint32_t* job = jobs + size_t(seq) * kJobWords;
    const uint8_t* src  = reinterpret_cast<const uint8_t*>((uint64_t(uniform(job[1])) << 32) | uniform(job[0]));
    const uint8_t* qual = reinterpret_cast<const uint8_t*>((uint64_t(uniform(job[3])) << 32) | uniform(job[2]));
    const uint64_t at   = (uint64_t(uniform(job[5])) << 32) | uniform(job[4]);
    const uint32_t len  = uniform(job[6]);
    const bool reverse  = uniform(job[7]) != 0;

    uint8_t* dst          = seqs + at; // byte j of the sequence goes to dst[j] and its weight to wdst[j]
    uint8_t* wdst         = wts + at;
    const uint32_t lead   = uint32_t(at & (kChunk - 1)); // both arrays are 16-byte aligned
    const uint32_t chunks = len ? (lead + len + kChunk - 1) / kChunk : 0; // chunk c holds bytes [16c - lead, 16c - lead + 16)
    for (uint32_t c = piece * kPieceChunks + lane; c < min(chunks, (piece + 1) * kPieceChunks); c += 64)
    {
        const int64_t j0 = int64_t(c) * kChunk - lead;
        if (j0 >= 0 && j0 + kChunk <= int64_t(len))
        {
            const uint32_t j = uint32_t(j0);
            // bytes j .. j + 15 of a reverse slice are source bytes len - 1 - j down to len - 16 - j
            const uint32_t from = reverse ? len - kChunk - j : j;
            uint4 v             = load16(src + from);
            if (reverse)
            {
                v = reverse16(v);
                v = uint4{complement4(v.x), complement4(v.y), complement4(v.z), complement4(v.w)};
            }
            *reinterpret_cast<uint4*>(dst + j) = v;
            uint4 w = uint4{0x01010101u, 0x01010101u, 0x01010101u, 0x01010101u};
            if (qual)
            {
                w = minus_qual_zero(load16(qual + from));
                if (reverse)
                    w = reverse16(w);
            }
            *reinterpret_cast<uint4*>(wdst + j) = w;
        }
        else
        {
            const int64_t first = j0 < 0 ? 0 : j0;
            const int64_t last  = j0 + kChunk < int64_t(len) ? j0 + kChunk : int64_t(len);
            for (int64_t j = first; j < last; j++)
            {
                const uint32_t from = reverse ? len - 1 - uint32_t(j) : uint32_t(j);
                dst[j]              = reverse ? complement(src[from]) : src[from];
                wdst[j]             = qual ? uint8_t(qual[from] - 33) : uint8_t(1);
            }
        }
    }
}

} // namespace

void gather_poa_slices(uint8_t* seqs, int8_t* wts, const SliceJob* d_jobs, int64_t n, int64_t max_len,
                       hipStream_t stream)
{
    if (n == 0)
        return;
    if ((reinterpret_cast<uintptr_t>(seqs) | reinterpret_cast<uintptr_t>(wts)) & (kChunk - 1))
        throw std::invalid_argument("gather_poa_slices: the input arrays are not 16-byte aligned");
    // a sequence of max_len bytes that begins at any byte touches this many chunks at most
    const int64_t piece_bytes = int64_t(kPieceChunks) * kChunk;
    const int64_t pieces      = std::max<int64_t>((max_len + (kChunk - 1) + piece_bytes - 1) / piece_bytes, 1);
    const int64_t waves       = n * pieces;
    const int64_t blocks      = (waves + kWaves - 1) / kWaves;
    if (n >= (int64_t(1) << 31) || max_len < 0 || max_len >= (int64_t(1) << 31) || blocks >= (int64_t(1) << 31))
        throw std::invalid_argument("gather_poa_slices: too many sequences for one launch");
    gather_poa_slices_kernel<<<unsigned(blocks), kThreads, 0, stream>>>(
        reinterpret_cast<const uint32_t*>(d_jobs), uint32_t(n), uint32_t(pieces), seqs, reinterpret_cast<uint8_t*>(wts));
    check_launch();
}

} // namespace polish
} // namespace gwamd
