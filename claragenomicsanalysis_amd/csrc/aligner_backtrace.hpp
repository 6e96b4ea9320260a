// The backtrace walk shared by the aligner kernels (myers_kernel,
// myers_banded_kernel, ukkonen_kernel, ukkonen_wide_kernel): path emission,
// the move out of a cell with the reference's tie order, the next-lane link
// walk of a window, the per-step walk on lanes 0..2, and the staged copy that
// refills a backtrace tile.
#pragma once

#include "aligner_device.hpp"

namespace gwamd
{
namespace aln
{

// Path emission: 64 states buffered one per lane, stored 64 at a time.
struct PathWriter
{
    int8_t* path;
    int cap;
    int pos = 0;
    int buf = 0;
    bool overflow = false;
    __device__ void put(int8_t r, int lane)
    {
        if (lane == (pos & 63))
            buf = r;
        if ((pos & 63) == 63)
            flush_full(lane);
        ++pos;
    }
    __device__ void flush_full(int lane)
    {
        const int at = (pos & ~63) + lane;
        if (at < cap)
            path[at] = int8_t(buf);
        else
            overflow = true;
    }
    __device__ void finish(int lane)
    {
        const int at = (pos & ~63) + lane;
        if (lane < (pos & 63))
        {
            if (at < cap)
                path[at] = int8_t(buf);
        }
        overflow = overflow || pos > cap;
    }
    // n copies of r (lane-parallel), after finish()
    __device__ void fill(int8_t r, int n, int lane)
    {
        for (int k = lane; k < n; k += kWave)
            if (pos + k < cap)
                path[pos + k] = r;
        pos += n;
        overflow = overflow || pos > cap;
    }
};

// The move out of a cell of value v with neighbours up (i-1, j), dg
// (i-1, j-1) and lf (i, j-1), in the reference's tie order: insertion (left),
// deletion (above), then match or mismatch.  ins / del are the two indel
// codes (Ukkonen exchanges them when it swaps the sequences).
struct CellMove
{
    int move;
    bool ins, del;
    // the chosen neighbour's one of three per-neighbour values
    __device__ __forceinline__ int pick(int lf, int up, int dg) const { return ins ? lf : (del ? up : dg); }
};
__device__ __forceinline__ CellMove cell_move(int v, int up, int dg, int lf, int ins, int del)
{
    const bool mi = lf + 1 == v;
    const bool md = !mi && up + 1 == v;
    return {mi ? ins : (md ? del : (dg == v ? int(kMatch) : int(kMismatch))), mi, md};
}

// The walk through an 8 x 8 window (lane 8a + b) whose lanes have each decided
// their cell's move: nxt is the lane that move leads to, or the lane itself
// where the walk has to stop.  From lane 0 the links are followed (one
// v_readlane per step) until a self-link, lane `end` (not visited).  sums
// holds the a + b of the `steps` visited lanes; a + b grows by 1 or 2 per
// step, so a visited cell's position on the path is rank_of(a + b), the
// number of visited cells with a smaller one.
struct LinkWalk
{
    int end, steps;
    uint64_t visited;
    uint32_t sums;
    __device__ __forceinline__ bool on(int lane) const { return (visited >> lane) & 1ull; }
    __device__ __forceinline__ int rank_of(int ab) const { return __builtin_popcount(sums & ((1u << ab) - 1u)); }
};
__device__ __forceinline__ LinkWalk link_walk(int nxt)
{
    LinkWalk w{0, 0, 0, 0};
    while (true)
    {
        const int nx = uni(__builtin_amdgcn_readlane(nxt, w.end));
        if (nx == w.end)
            break;
        w.sums |= 1u << ((w.end >> 3) + (w.end & 7));
        w.visited |= 1ull << w.end;
        ++w.steps;
        w.end = nx;
    }
    return w;
}

// One step of the per-step walk: lanes 0, 1 and 2 hold the values of the
// cell above, the diagonal one and the left one in v; s is the walk's running
// score.  Returns the move and replaces s by the chosen neighbour's value;
// the caller moves (i, j).
__device__ __forceinline__ CellMove three_lane_step(int v, int& s, int ins, int del)
{
    const int above  = uni(__builtin_amdgcn_readlane(v, 0));
    const int dg     = uni(__builtin_amdgcn_readlane(v, 1));
    const int left   = uni(__builtin_amdgcn_readlane(v, 2));
    const CellMove m = cell_move(s, above, dg, left, ins, del);
    s                = m.pick(left, above, dg);
    return m;
}

// Copy of n elements through registers, lane-parallel: kInFlight loads per
// lane are issued before the first store waits for one (a loop of single
// loads waits one HBM latency per 64 elements).  load(e, v) fills v with
// element e or, where the caller's predicate says so, leaves it; store(e, v)
// stores it.  The caller brackets the copy with its wave_sync() pair.
constexpr int kInFlight = 8;
template <typename V, typename Load, typename Store>
__device__ __forceinline__ void staged_copy(int n, int lane, Load load, Store store)
{
    // (e0 carries the lane: a uniform e0 keeps the offsets u * kWave + lane in
    // registers for the whole kernel.  Eight variables, not an array: an array
    // becomes one vector, zeroed and carried around the caller's loop)
    static_assert(kInFlight == 8, "eight staging variables");
    for (int e0 = lane; e0 - lane < n; e0 += kInFlight * kWave)
    {
        V v0, v1, v2, v3, v4, v5, v6, v7;
        const auto ld = [&](int u, V& v) {
            if (e0 + u * kWave < n)
                load(e0 + u * kWave, v);
        };
        const auto st = [&](int u, const V& v) {
            if (e0 + u * kWave < n)
                store(e0 + u * kWave, v);
        };
        ld(0, v0), ld(1, v1), ld(2, v2), ld(3, v3), ld(4, v4), ld(5, v5), ld(6, v6), ld(7, v7);
        st(0, v0), st(1, v1), st(2, v2), st(3, v3), st(4, v4), st(5, v5), st(6, v6), st(7, v7);
    }
}

} // namespace aln
} // namespace gwamd
