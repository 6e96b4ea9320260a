// Overlapper on the GPU: sorted anchors to Overlap records (reference
// cudamapper/src/overlapper_triggered.cu; interface
// include/.../cudamapper/overlapper.hpp).
//
// The reference run-length encodes the anchors under a non-transitive
// "equality", selects the runs of three or more, reduces them by key under a
// second such equality and filters the result.  Here every step that compares
// compares an element with its left neighbour and nothing else, which is what
// those library calls do in practice and what the model pins:
//
//   level 1  anchors -> chain starts.  chain_flag_kernel reads every anchor
//            once (16 bytes) and leaves one 64-bit head ballot per 64 anchors
//            and a head count per tile of kOverlapTile; after an exclusive
//            sum over the tiles chain_start_kernel turns the ballots (1/128 of
//            the anchors' bytes) into the compacted chain_start[].
//   level 2  chains -> kept chains: those of three anchors or more.
//   level 3  kept chains -> groups -> overlaps: a kept chain starts a group
//            unless its first anchor fuses with the first anchor of the kept
//            chain before it; one Overlap per group, filtered, in order.
//
// Levels 2 and 3 are three instances of one count / exclusive sum / write
// compaction (count_kernel, write_kernel) over one item per thread.  The host
// reads back three numbers: the chain count (with the bad-input word), the
// group count and the overlap count.
#include "mapper_prims.hpp"

namespace gwamd
{
namespace mapper
{
namespace
{

constexpr uint32_t kTile         = kOverlapTile;
constexpr uint32_t kWaves        = kThreads / 64;
constexpr uint32_t kWaveAnchors  = kTile / kWaves; // contiguous anchors of one wave
constexpr uint32_t kWaveLoads    = kWaveAnchors / 64;
constexpr uint32_t kTileBallots  = kTile / 64;
constexpr uint32_t kBadOrder     = 1; // an adjacent pair is out of order
constexpr uint32_t kBadPosition  = 2; // a position of 2^31 or more
constexpr uint32_t kChainTail    = 3; // tail_length_for_chain
constexpr uint32_t kChainReach   = 150;
constexpr uint32_t kFuseReach    = 300;
static_assert(kTile % (64 * kWaves) == 0, "a tile is whole wave loads");
static_assert(kTileBallots == 32, "chain_start_kernel scans a tile's ballots in 32 lanes");

// an anchor as one 16-byte load: x query read, y target read, z query position, w target position
using Anchor4 = uint4;

__device__ inline uint32_t abs_diff(uint32_t a, uint32_t b)
{
    const int32_t d = int32_t(a - b);
    return d < 0 ? 0u - uint32_t(d) : uint32_t(d);
}

// the reference's operator==(Anchor, Anchor) with a the left neighbour of b
__device__ inline bool same_chain(const Anchor4& a, const Anchor4& b)
{
    return a.x == b.x && a.y == b.y && uint32_t(b.z - a.z) < kChainReach && abs_diff(b.w, a.w) < kChainReach;
}

// the reference's operator==(cuOverlapKey, cuOverlapKey) on two chains' first anchors
__device__ inline bool same_group(const Anchor4& a, const Anchor4& b)
{
    return a.x == b.x && a.y == b.y && abs_diff(abs_diff(a.z, b.z), abs_diff(a.w, b.w)) < kFuseReach;
}

__device__ inline bool ordered(const Anchor4& a, const Anchor4& b) // a <= b
{
    if (a.x != b.x)
        return a.x < b.x;
    if (a.y != b.y)
        return a.y < b.y;
    if (a.z != b.z)
        return a.z < b.z;
    return a.w <= b.w;
}

__device__ inline Anchor4 lane_above(const Anchor4& v, int src_lane)
{
    return Anchor4{uint32_t(__shfl(int(v.x), src_lane)), uint32_t(__shfl(int(v.y), src_lane)),
                   uint32_t(__shfl(int(v.z), src_lane)), uint32_t(__shfl(int(v.w), src_lane))};
}

// Each wave owns kWaveAnchors contiguous anchors and loads them 64 at a time,
// all loads in flight before the first compare.  An anchor's left neighbour is
// the lane below; lane 0 takes it from lane 63 of the load before, and for the
// wave's first load from anchors[first - 1]: 16 more bytes per 8 KiB, so that
// no wave waits for another before it compares.
__global__ __launch_bounds__(kThreads) void chain_flag_kernel(const Anchor4* __restrict__ anchors, uint32_t n,
                                                              uint64_t* __restrict__ ballots,
                                                              uint32_t* __restrict__ tile_counts,
                                                              uint32_t* __restrict__ bad)
{
    __shared__ uint32_t wave_heads[kWaves];
    const uint32_t lane  = threadIdx.x & 63;
    const uint32_t wave  = threadIdx.x >> 6;
    const uint32_t first = blockIdx.x * kTile + wave * kWaveAnchors;

    Anchor4 v[kWaveLoads];
#pragma unroll
    for (uint32_t j = 0; j < kWaveLoads; j++)
    {
        const uint32_t i = first + j * 64 + lane;
        v[j]             = i < n ? anchors[i] : Anchor4{0, 0, 0, 0};
    }
    Anchor4 carry = first > 0 && first < n ? anchors[first - 1] : Anchor4{0, 0, 0, 0};

    uint32_t heads = 0, trouble = 0;
#pragma unroll
    for (uint32_t j = 0; j < kWaveLoads; j++)
    {
        const uint32_t i   = first + j * 64 + lane;
        const bool valid   = i < n;
        Anchor4 left       = lane_above(v[j], int(lane) - 1);
        if (lane == 0)
            left = carry;
        carry              = lane_above(v[j], 63);
        const bool head    = valid && (i == 0 || !same_chain(left, v[j]));
        if (valid && i > 0 && !ordered(left, v[j]))
            trouble |= kBadOrder;
        if (valid && ((v[j].z | v[j].w) >> 31))
            trouble |= kBadPosition;
        const uint64_t ballot = __ballot(head);
        if (lane == 0 && valid)
            ballots[i / 64] = ballot;
        heads += uint32_t(__popcll(ballot));
    }
    const uint32_t seen = (__ballot(trouble & kBadOrder) ? kBadOrder : 0) |
                          (__ballot(trouble & kBadPosition) ? kBadPosition : 0);
    if (lane == 0)
    {
        if (seen)
            atomicOr(bad, seen);
        wave_heads[wave] = heads;
    }
    __syncthreads();
    if (threadIdx.x == 0)
    {
        uint32_t sum = 0;
        for (uint32_t w = 0; w < kWaves; w++)
            sum += wave_heads[w];
        tile_counts[blockIdx.x] = sum;
    }
}

// One thread per ballot word; the 32 words of a tile share half a wave, which
// scans their head counts.  tile_first[t]: chains before tile t.
__global__ __launch_bounds__(kThreads) void chain_start_kernel(const uint64_t* __restrict__ ballots,
                                                               uint32_t num_ballots,
                                                               const uint32_t* __restrict__ tile_first,
                                                               uint32_t* __restrict__ chain_start)
{
    const uint32_t g     = blockIdx.x * kThreads + threadIdx.x;
    uint64_t ballot      = g < num_ballots ? ballots[g] : 0;
    const uint32_t count = uint32_t(__popcll(ballot));
    uint32_t before      = count; // inclusive over the tile's words up to this one
    for (int d = 1; d < int(kTileBallots); d *= 2)
    {
        const uint32_t below = uint32_t(__shfl_up(int(before), d, kTileBallots));
        if (int(threadIdx.x % kTileBallots) >= d)
            before += below;
    }
    if (ballot == 0)
        return;
    uint32_t dst = tile_first[g / kTileBallots] + before - count;
    while (ballot)
    {
        chain_start[dst++] = g * 64 + uint32_t(__ffsll((long long)ballot) - 1);
        ballot &= ballot - 1;
    }
}

// ---- count / exclusive sum / write compaction, one item per thread ----------
//
// Op has flag(i, n): whether item i of n survives, and emit(i, n, dst): write
// survivor i as output dst.  n is read from device memory: it is the total of
// the level before.

__device__ inline uint32_t rank_in_block(bool flag, uint32_t& block_total)
{
    __shared__ uint32_t wave_total[kWaves];
    const uint32_t lane   = threadIdx.x & 63;
    const uint32_t wave   = threadIdx.x >> 6;
    const uint64_t ballot = __ballot(flag);
    if (lane == 0)
        wave_total[wave] = uint32_t(__popcll(ballot));
    __syncthreads();
    uint32_t rank = uint32_t(__popcll(ballot & ((uint64_t(1) << lane) - 1)));
    block_total   = 0;
    for (uint32_t w = 0; w < kWaves; w++)
    {
        if (w < wave)
            rank += wave_total[w];
        block_total += wave_total[w];
    }
    return rank;
}

template <typename Op>
__global__ __launch_bounds__(kThreads) void count_kernel(Op op, const uint32_t* __restrict__ n_ptr,
                                                         uint32_t* __restrict__ block_counts)
{
    const uint32_t n = *n_ptr;
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    uint32_t total;
    rank_in_block(i < n && op.flag(i, n), total);
    if (threadIdx.x == 0)
        block_counts[blockIdx.x] = total;
}

template <typename Op>
__global__ __launch_bounds__(kThreads) void write_kernel(Op op, const uint32_t* __restrict__ n_ptr,
                                                         const uint32_t* __restrict__ block_first)
{
    const uint32_t n = *n_ptr;
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    const bool flag  = i < n && op.flag(i, n);
    uint32_t total;
    const uint32_t rank = rank_in_block(flag, total);
    if (flag)
        op.emit(i, n, block_first[blockIdx.x] + rank);
}

struct KeepChain
{
    const uint32_t* __restrict__ chain_start;
    uint32_t num_anchors;
    uint32_t* __restrict__ kept_start;
    uint32_t* __restrict__ kept_len;

    __device__ uint32_t length(uint32_t c, uint32_t n) const
    {
        return (c + 1 < n ? chain_start[c + 1] : num_anchors) - chain_start[c];
    }
    __device__ bool flag(uint32_t c, uint32_t n) const { return length(c, n) >= kChainTail; }
    __device__ void emit(uint32_t c, uint32_t n, uint32_t dst) const
    {
        kept_start[dst] = chain_start[c];
        kept_len[dst]   = length(c, n);
    }
};

struct GroupHead
{
    const Anchor4* __restrict__ anchors;
    const uint32_t* __restrict__ kept_start;
    uint32_t* __restrict__ group_first;

    __device__ bool flag(uint32_t k, uint32_t) const
    {
        return k == 0 || !same_group(anchors[kept_start[k - 1]], anchors[kept_start[k]]);
    }
    __device__ void emit(uint32_t k, uint32_t, uint32_t dst) const { group_first[dst] = k; }
};

struct BuildOverlap
{
    const Anchor4* __restrict__ anchors;
    const uint32_t* __restrict__ kept_start;
    const uint32_t* __restrict__ kept_len;
    const uint32_t* __restrict__ kept_len_before; // exclusive sum of kept_len, one entry past the last chain
    const uint32_t* __restrict__ group_first;
    const uint32_t* __restrict__ num_kept;
    uint64_t min_residues, min_overlap_len, min_bases_per_residue;
    float min_overlap_fraction;
    uint32_t* __restrict__ out; // nine words per overlap

    // words of the OverlapRecord of group g; whether it passes the filter
    __device__ bool build(uint32_t g, uint32_t n, uint32_t (&w)[9]) const
    {
        const uint32_t first = group_first[g];
        const uint32_t next  = g + 1 < n ? group_first[g + 1] : *num_kept;
        const Anchor4 s      = anchors[kept_start[first]];
        const Anchor4 e      = anchors[kept_start[next - 1] + kept_len[next - 1] - 1];
        const uint32_t residues = kept_len_before[next] - kept_len_before[first];
        uint32_t target_start = s.w, target_end = e.w;
        const bool reverse = target_start > target_end;
        if (reverse)
        {
            target_start = e.w;
            target_end   = s.w;
        }
        w[0] = e.x;
        w[1] = e.y;
        w[2] = s.z;
        w[3] = target_start;
        w[4] = e.z;
        w[5] = target_end;
        w[6] = reverse ? '-' : '+';
        w[7] = residues;
        w[8] = 1; // overlap_complete
        const uint32_t target_len = target_end - target_start;
        const uint32_t query_len  = e.z - s.z;
        const uint32_t len        = max(target_len, query_len);
        // IEEE float32 quotients; 0 / 0 is NaN and fails
        return uint64_t(residues) >= min_residues && uint64_t(len / residues) < min_bases_per_residue &&
               uint64_t(query_len) >= min_overlap_len && uint64_t(target_len) >= min_overlap_len && e.x != e.y &&
               float(target_len) / float(len) > min_overlap_fraction &&
               float(query_len) / float(len) > min_overlap_fraction;
    }
    __device__ bool flag(uint32_t g, uint32_t n) const
    {
        uint32_t w[9];
        return build(g, n, w);
    }
    __device__ void emit(uint32_t g, uint32_t n, uint32_t dst) const
    {
        uint32_t w[9];
        build(g, n, w);
        for (int k = 0; k < 9; k++)
            out[size_t(dst) * 9 + k] = w[k];
    }
};

// Survivors of the first *n_ptr (at most cap) items, written by op in order.
// Returns the device address of their number.
template <typename Op>
const uint32_t* compact(const Op& op, const uint32_t* n_ptr, uint32_t cap, DevBuf<uint32_t>& block_first,
                        const Budget& budget, hipStream_t stream)
{
    const unsigned blocks = blocks_for(cap, uint64_t(1) << 31);
    block_first.alloc(size_t(blocks) + 1, budget);
    GWAMD_HIP_CHECK(hipMemsetAsync(block_first.data() + blocks, 0, sizeof(uint32_t), stream));
    count_kernel<<<blocks, kThreads, 0, stream>>>(op, n_ptr, block_first.data());
    check_launch();
    exclusive_sum(block_first.data(), block_first.data(), size_t(blocks) + 1, budget, stream);
    write_kernel<<<blocks, kThreads, 0, stream>>>(op, n_ptr, block_first.data());
    check_launch();
    return block_first.data() + blocks;
}

} // namespace

void get_overlaps(std::vector<OverlapRecord>& out, const AnchorRecord* anchors, int64_t n64, const OverlapParams& params,
                  const Budget& budget, hipStream_t stream, OverlapCounts* counts)
{
    out.clear();
    if (counts)
        *counts = OverlapCounts{};
    if (n64 == 0)
        return;
    const uint32_t n    = uint32_t(n64); // at most 2^31
    const auto* anchor4 = reinterpret_cast<const Anchor4*>(anchors);

    // level 1
    const uint32_t tiles       = uint32_t((n64 + kTile - 1) / kTile);
    const uint32_t num_ballots = uint32_t((n64 + 63) / 64);
    DevBuf<uint32_t> chain_start;
    uint32_t num_chains = 0;
    {
        DevBuf<uint64_t> ballots(num_ballots, budget);
        DevBuf<uint32_t> tile_first(size_t(tiles) + 2, budget); // [tiles]: the chain count, [tiles + 1]: bad input
        GWAMD_HIP_CHECK(hipMemsetAsync(tile_first.data() + tiles, 0, 2 * sizeof(uint32_t), stream));
        chain_flag_kernel<<<tiles, kThreads, 0, stream>>>(anchor4, n, ballots.data(), tile_first.data(),
                                                          tile_first.data() + tiles + 1);
        check_launch();
        exclusive_sum(tile_first.data(), tile_first.data(), size_t(tiles) + 1, budget, stream);
        uint32_t tail[2] = {0, 0};
        GWAMD_HIP_CHECK(
            hipMemcpyAsync(tail, tile_first.data() + tiles, sizeof(tail), hipMemcpyDeviceToHost, stream));
        GWAMD_HIP_CHECK(hipStreamSynchronize(stream));
        if (tail[1] & kBadPosition)
            throw std::invalid_argument("an anchor's position in its read is 2^31 or more");
        if (tail[1] & kBadOrder)
            throw std::invalid_argument("anchors are not sorted by (query_read_id, target_read_id, "
                                        "query_position_in_read, target_position_in_read)");
        num_chains = tail[0];
        chain_start.alloc(num_chains, budget);
        chain_start_kernel<<<blocks_for(num_ballots), kThreads, 0, stream>>>(ballots.data(), num_ballots,
                                                                             tile_first.data(), chain_start.data());
        check_launch();
        GWAMD_HIP_CHECK(hipStreamSynchronize(stream)); // ballots and tile_first are freed here
    }
    if (counts)
        counts->chains = num_chains;
    const uint32_t cap = std::min(num_chains, n / kChainTail); // no more kept chains than this
    if (cap == 0)
        return;

    // level 2
    DevBuf<uint32_t> num_chains_d(1, budget), kept_start(cap, budget), kept_len(size_t(cap) + 1, budget);
    DevBuf<uint32_t> kept_len_before(size_t(cap) + 1, budget), kept_blocks, head_blocks, group_first(cap, budget);
    GWAMD_HIP_CHECK(hipMemcpyAsync(num_chains_d.data(), &num_chains, sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    GWAMD_HIP_CHECK(hipMemsetAsync(kept_len.data(), 0, (size_t(cap) + 1) * sizeof(uint32_t), stream));
    const uint32_t* num_kept_d = compact(KeepChain{chain_start.data(), n, kept_start.data(), kept_len.data()},
                                         num_chains_d.data(), num_chains, kept_blocks, budget, stream);
    exclusive_sum(kept_len.data(), kept_len_before.data(), size_t(cap) + 1, budget, stream);

    // level 3
    const uint32_t* num_groups_d = compact(GroupHead{anchor4, kept_start.data(), group_first.data()}, num_kept_d, cap,
                                           head_blocks, budget, stream);
    uint32_t num_kept = 0, num_groups = 0;
    GWAMD_HIP_CHECK(hipMemcpyAsync(&num_kept, num_kept_d, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    GWAMD_HIP_CHECK(hipMemcpyAsync(&num_groups, num_groups_d, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    GWAMD_HIP_CHECK(hipStreamSynchronize(stream));
    if (counts)
    {
        counts->kept_chains = num_kept;
        counts->groups      = num_groups;
    }
    if (num_groups == 0)
        return;

    DevBuf<OverlapRecord> overlaps(num_groups, budget);
    DevBuf<uint32_t> overlap_blocks;
    const BuildOverlap build{anchor4,
                             kept_start.data(),
                             kept_len.data(),
                             kept_len_before.data(),
                             group_first.data(),
                             num_kept_d,
                             uint64_t(params.min_residues),
                             uint64_t(params.min_overlap_len),
                             uint64_t(params.min_bases_per_residue),
                             params.min_overlap_fraction,
                             reinterpret_cast<uint32_t*>(overlaps.data())};
    const uint32_t num_overlaps = read_back(compact(build, num_groups_d, num_groups, overlap_blocks, budget, stream),
                                            stream);
    if (counts)
        counts->overlaps = num_overlaps;
    out.resize(num_overlaps);
    if (num_overlaps > 0)
        GWAMD_HIP_CHECK(hipMemcpyAsync(out.data(), overlaps.data(), size_t(num_overlaps) * sizeof(OverlapRecord),
                                       hipMemcpyDeviceToHost, stream));
    GWAMD_HIP_CHECK(hipStreamSynchronize(stream));
}

} // namespace mapper
} // namespace gwamd
