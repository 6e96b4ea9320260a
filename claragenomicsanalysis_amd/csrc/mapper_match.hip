// Anchor matcher on the GPU (reference cudamapper/src/matcher_gpu.cu,
// matcher_gpu.cuh:60-176; interface include/.../cudamapper/matcher.hpp).
//
// Every unique query representation is looked up in the target's unique
// representations by binary search; a match contributes (query count x target
// count) anchors.  An exclusive scan of those counts in 64 bits gives each
// representation's first anchor and the total, which the host checks against
// the caller's cap before anything of that size is allocated.  The expansion
// kernel gives every output anchor to one thread, which finds its
// representation by binary search over the starts.  The anchors are then
// sorted by their whole 128-bit value in two stable radix-sort passes over two
// 64-bit keys: (query_position, target_position) first, then (query_read_id,
// target_read_id).
#include "mapper_prims.hpp"

namespace gwamd
{
namespace mapper
{
namespace
{

constexpr uint32_t kNoMatch = 0xFFFFFFFFu;

// counts[i]: anchors of query representation i; counts[nq] = 0
__global__ void match_count_kernel(const uint64_t* __restrict__ q_unique, const uint32_t* __restrict__ q_first,
                                   uint32_t nq, const uint64_t* __restrict__ t_unique,
                                   const uint32_t* __restrict__ t_first, uint32_t nt, uint32_t* __restrict__ match,
                                   uint64_t* __restrict__ counts)
{
    for (uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x; i <= nq; i += uint64_t(gridDim.x) * kThreads)
    {
        if (i == nq)
        {
            counts[i] = 0;
            continue;
        }
        const uint64_t rep = q_unique[i];
        uint32_t lo = 0, hi = nt; // first target representation >= rep
        while (lo < hi)
        {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (t_unique[mid] < rep)
                lo = mid + 1;
            else
                hi = mid;
        }
        const bool found = lo < nt && t_unique[lo] == rep;
        match[i]         = found ? lo : kNoMatch;
        counts[i]        = found ? uint64_t(q_first[i + 1] - q_first[i]) * uint64_t(t_first[lo + 1] - t_first[lo]) : 0;
    }
}

__global__ void expand_kernel(const uint64_t* __restrict__ starts, uint32_t nq, const uint32_t* __restrict__ match,
                              const uint32_t* __restrict__ q_first, const uint32_t* __restrict__ t_first,
                              const uint32_t* __restrict__ q_read, const uint32_t* __restrict__ q_pos,
                              const uint32_t* __restrict__ t_read, const uint32_t* __restrict__ t_pos, uint64_t total,
                              uint64_t* __restrict__ key_reads, uint64_t* __restrict__ key_positions)
{
    for (uint64_t a = uint64_t(blockIdx.x) * kThreads + threadIdx.x; a < total; a += uint64_t(gridDim.x) * kThreads)
    {
        // the last representation whose start is <= a: starts[0] = 0 and
        // starts[nq] = total > a, and representations without anchors share
        // their start with the next one
        uint32_t lo = 0, hi = nq; // first index in [0, nq] with starts[index] > a
        while (lo < hi)
        {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (starts[mid] <= a)
                lo = mid + 1;
            else
                hi = mid;
        }
        const uint32_t i     = lo - 1;
        const uint32_t tj    = match[i];
        const uint32_t tc    = t_first[tj + 1] - t_first[tj];
        const uint64_t r     = a - starts[i];
        const uint32_t qe    = q_first[i] + uint32_t(r / tc);
        const uint32_t te    = t_first[tj] + uint32_t(r % tc);
        key_reads[a]     = (uint64_t(q_read[qe]) << 32) | t_read[te];
        key_positions[a] = (uint64_t(q_pos[qe]) << 32) | t_pos[te];
    }
}

__global__ void pack_kernel(const uint64_t* __restrict__ key_reads, const uint64_t* __restrict__ key_positions,
                            uint64_t total, AnchorRecord* __restrict__ anchors)
{
    for (uint64_t a = uint64_t(blockIdx.x) * kThreads + threadIdx.x; a < total; a += uint64_t(gridDim.x) * kThreads)
    {
        const uint64_t r = key_reads[a], p = key_positions[a];
        anchors[a]       = AnchorRecord{uint32_t(r >> 32), uint32_t(r), uint32_t(p >> 32), uint32_t(p)};
    }
}

} // namespace

void match_anchors(DevBuf<AnchorRecord>& out, const IndexData& query, const IndexData& target, int64_t max_anchors,
                   const Budget& budget, hipStream_t stream)
{
    out.free();
    const uint32_t nq = uint32_t(query.unique_representations.size());
    const uint32_t nt = uint32_t(target.unique_representations.size());
    if (nq == 0 || nt == 0)
        return;

    DevBuf<uint32_t> match(nq, budget);
    DevBuf<uint64_t> starts(size_t(nq) + 1, budget);
    {
        DevBuf<uint64_t> counts(size_t(nq) + 1, budget);
        match_count_kernel<<<blocks_for(uint64_t(nq) + 1), kThreads, 0, stream>>>(
            query.unique_representations.data(), query.first_occurrence_of_representations.data(), nq,
            target.unique_representations.data(), target.first_occurrence_of_representations.data(), nt, match.data(),
            counts.data());
        check_launch();
        exclusive_sum(counts.data(), starts.data(), size_t(nq) + 1, budget, stream);
    }
    const uint64_t total = read_back(starts.data() + nq, stream);
    if (total > uint64_t(max_anchors))
        throw std::runtime_error("matching gives " + std::to_string(total) + " anchors, more than max_anchors = " +
                                 std::to_string(max_anchors));
    if (total == 0)
        return;

    DevBuf<uint64_t> key_reads(total, budget), key_positions(total, budget);
    expand_kernel<<<blocks_for(total), kThreads, 0, stream>>>(
        starts.data(), nq, match.data(), query.first_occurrence_of_representations.data(),
        target.first_occurrence_of_representations.data(), query.read_ids.data(), query.positions_in_reads.data(),
        target.read_ids.data(), target.positions_in_reads.data(), total, key_reads.data(), key_positions.data());
    check_launch();
    {
        DevBuf<uint64_t> reads_tmp(total, budget), positions_tmp(total, budget);
        // least significant key first; both passes are stable
        sort_pairs(key_positions.data(), positions_tmp.data(), key_reads.data(), reads_tmp.data(), total,
                   32 + bit_length(query.number_of_basepairs_in_longest_read), budget, stream);
        sort_pairs(reads_tmp.data(), key_reads.data(), positions_tmp.data(), key_positions.data(), total,
                   32 + bit_length(query.largest_read_id), budget, stream);
    }
    out.alloc(total, budget);
    pack_kernel<<<blocks_for(total), kThreads, 0, stream>>>(key_reads.data(), key_positions.data(), total, out.data());
    check_launch();
    GWAMD_HIP_CHECK(hipStreamSynchronize(stream));
}

} // namespace mapper
} // namespace gwamd
